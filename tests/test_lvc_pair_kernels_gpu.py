"""qd_lvc_pair_observe and qd_lvc_pair_rk4 (each admitted path, forced) member by member against the restatement of
tests/lvc_pair_models.py in extended precision (tests/test_lvc_pair_host.py earns it its role on the host).

Inputs: dense random complex Hel and W, not Hermitian (lm.random_model); ket random and normalised, bra = normalise(ket
+ 0.5 noise), so that no block of the record is a near-cancellation; dt = 0.5 / lm.h_bound; 5 steps with a record every
2 (the fifth step takes none); P in {1, 3}; every block 0 .. M. Asserted: max over members of the relative error <
1e-12, the bound of tests/test_lvc_kernels_gpu.py for the same kind of run, for the records of qd_lvc_pair_observe, the
in-run records and the final states. With these inputs the float64 restatement is within 1e-13 of the extended one
(tests/test_lvc_pair_host.py; 3e-16 at all but the largest shape), so the bound is the kernels' alone. Bit for bit: on
the staged path the final states equal lvc_rk4(path="staged") of the same 2 P states; the in-run records equal
lvc_pair_observe of the states; single- block calls equal the slices of the all-block call; with bra = ket the blocks
equal the rho and X parts of lvc_observe; an identical call and a graph replay agree. The path noted is the plan's; a
forced resident call past the limit is refused with psi unchanged. Where np.longdouble is not extended the float64
restatement is the reference and the output says so.

Shapes (nel; dims): the smallest models; (4; 3, 5) and (5; 4, 3), the two sides of the split between all rows in
registers and one pass per row; nel = 8; a fastest axis past the tile and a slow one; inert axes; six modes; one below,
at and one above the tile extent, the neighbours of the pair resident limit at nel = 1, 3 and 8 in one mode and at nel =
3 for every other mode count's own limit, from the plan library; and (1; 256 LVC_OBS_MAX_GRID + 1), staged, P = 1, where
a partial workgroup sums more than one tile."""
import functools

import numpy as np
import pytest

import lvc_models as lm
import lvc_pair_models as pm
from conftest import took
from oracle import highprec as hp
from test_lvc_plan_host import RESIDENT, STAGED
from test_lvc_pair_plan_host import build_pair_plan_lib, pair_plan_of

pytestmark = pytest.mark.gpu
BOUND = 1e-12
NSTEPS, SE = pm.NSTEPS, pm.SE
PATH_NAME = {STAGED: "lvc_pair_staged", RESIDENT: "lvc_pair_resident"}
PATH_ARG = {STAGED: "staged", RESIDENT: "resident"}


@functools.lru_cache(maxsize=None)
def _plan_lib():
    import tempfile
    return build_pair_plan_lib(tempfile.mkdtemp(prefix="lvc_pair_plan_"))


def _shapes():
    """pm.FIXED, then the shapes the plan's constants give.  Collected without the plan library where there is no host
    compiler (the tests skip then)."""
    try:
        lib = _plan_lib()
    except BaseException:   # pytest.skip raises outside the Exception tree
        return pm.FIXED
    return pm.gpu_cases(lib.TILE, lib.limit)


def _t(a):
    import torch
    return torch.from_numpy(np.array(a)).to(torch.device("cuda", 0))   # a copy: the shared inputs are read-only


def _bits(x):
    import torch
    return x.contiguous().view(torch.float64)


@functools.lru_cache(maxsize=None)
def _case(nel, dims, P):
    """Inputs and the reference of one (shape, P), computed once and shared by the tests; never written to."""
    omega, Hel, W, pairs, dt = pm.gpu_inputs(nel, dims, P)
    dtype = np.clongdouble if hp.EXTENDED_OK else np.complex128
    if not hp.EXTENDED_OK:
        print("np.longdouble is not extended here: float64 restatement as the reference")
    blocks = tuple(range(1 + len(dims)))
    ref = pm.pair_rk4(pairs, nel, dims, omega, Hel, W, dt, NSTEPS, SE, blocks, dtype=dtype)
    for a in (omega, Hel, W, pairs) + ref:
        a.setflags(write=False)
    return omega, Hel, W, pairs, dt, blocks, ref


def _check(label, errs):
    print(f"{label}: " + ", ".join(f"{k} {e:.2e}" for k, e in errs.items()))
    bad = {k: e for k, e in errs.items() if not e < BOUND}
    assert not bad, (label, bad)


def _admitted(nel, dims, P):
    lib = _plan_lib()
    auto = pair_plan_of(lib, P, nel, dims)
    assert not auto.refused
    paths = [STAGED] + ([RESIDENT] if not pair_plan_of(lib, P, nel, dims, path=RESIDENT).refused else [])
    return auto.base.path, paths


def _run(nel, dims, P, path, blocks=None, pairs=None):
    from pyqed_amd.mol import lvc_pair_rk4
    omega, Hel, W, pairs0, dt, all_blocks, _ = _case(nel, dims, P)
    psi = _t(pairs0 if pairs is None else pairs)
    took("")
    rec = lvc_pair_rk4(psi, nel, dims, omega, _t(Hel), _t(W), dt, NSTEPS, save_every=SE,
                       blocks=all_blocks if blocks is None else blocks, path=path)
    return psi, rec, took("")[1]


@pytest.mark.parametrize("P", [1, 3])
@pytest.mark.parametrize("nel,dims", _shapes())
def test_pair_observe(nel, dims, P):
    import torch
    from pyqed_amd.mol import lvc_observe, lvc_pair_observe
    _, _, _, pairs, _, blocks, (_, rrec) = _case(nel, dims, P)
    M = len(dims)
    rec = lvc_pair_observe(_t(pairs), nel, dims, blocks)
    assert rec.shape == (P, 1 + M, nel, nel)
    assert torch.equal(_bits(rec), _bits(lvc_pair_observe(_t(pairs), nel, dims, blocks)))
    _check(f"lvc pair nel={nel} dims={dims} P={P}", {"observe": hp.worst_member(rec.cpu().numpy(), rrec[:, 0])})
    # a single block has the bits of its slice of the all-block call, whatever stands beside it
    for r in sorted({0, 1, M}):
        one = lvc_pair_observe(_t(pairs), nel, dims, [r])
        assert one.shape == (P, 1, nel, nel) and torch.equal(_bits(one[:, 0]), _bits(rec[:, r])), r
    rev = lvc_pair_observe(_t(pairs), nel, dims, blocks[::-1])
    assert torch.equal(_bits(rev), _bits(rec.flip(1)))
    # bra = ket: the rho and X parts of qd_lvc_observe's record
    same = np.ascontiguousarray(np.stack([pairs[:, 0], pairs[:, 0]], axis=1))
    own = lvc_observe(_t(pairs[:, 0]), nel, dims)[:, :nel * nel * (1 + M)].reshape(P, 1 + M, nel, nel)
    assert torch.equal(_bits(lvc_pair_observe(_t(same), nel, dims, blocks)), _bits(own))


@pytest.mark.parametrize("P", [1, 3])
@pytest.mark.parametrize("nel,dims", _shapes())
def test_pair_rk4_on_each_admitted_path(nel, dims, P):
    import torch
    from pyqed_amd.mol import lvc_observe, lvc_pair_observe, lvc_pair_rk4, lvc_rk4
    omega, Hel, W, pairs, dt, blocks, (rpsi, rrec) = _case(nel, dims, P)
    M, D = len(dims), lm.size(nel, dims)
    auto, paths = _admitted(nel, dims, P)
    for path in paths:
        psi, rec, noted = _run(nel, dims, P, PATH_ARG[path])
        assert noted == [PATH_NAME[path]], noted
        assert rec.shape == (P, NSTEPS // SE + 1, 1 + M, nel, nel) and psi.shape == (P, 2, D)
        _check(f"lvc pair nel={nel} dims={dims} P={P} {PATH_NAME[path]}",
               {"final": hp.worst_member(psi.cpu().numpy(), rpsi), "rec": hp.worst_member(rec.cpu().numpy(), rrec)})
        if path == STAGED:
            flat = _t(pairs).reshape(2 * P, D)
            lvc_rk4(flat, nel, dims, omega, _t(Hel), _t(W), dt, NSTEPS, observe=False, path="staged")
            assert torch.equal(_bits(flat), _bits(psi.reshape(2 * P, D)))
        # the in-run records are qd_lvc_pair_observe of the states, bit for bit: t0, then each save (the run redone in
        # pieces of save_every steps)
        assert torch.equal(_bits(rec[:, 0]), _bits(lvc_pair_observe(_t(pairs), nel, dims, blocks)))
        mid = _t(pairs)
        for k in range(1, NSTEPS // SE + 1):
            lvc_pair_rk4(mid, nel, dims, omega, _t(Hel), _t(W), dt, SE, save_every=SE, blocks=[0],
                         path=PATH_ARG[path])
            assert torch.equal(_bits(rec[:, k]), _bits(lvc_pair_observe(mid, nel, dims, blocks))), (path, k)
        # an identical call agrees bit for bit
        psi2, rec2, _ = _run(nel, dims, P, PATH_ARG[path])
        assert torch.equal(_bits(psi), _bits(psi2)) and torch.equal(_bits(rec), _bits(rec2))
        # single-block calls are the slices of the all-block call
        for r in sorted({0, 1, M}):
            psi1, one, _ = _run(nel, dims, P, PATH_ARG[path], blocks=[r])
            assert torch.equal(_bits(one[:, :, 0]), _bits(rec[:, :, r])) and torch.equal(_bits(psi1), _bits(psi)), r
        # bra = ket: the in-run records at t0 and after the last step are lvc_observe's rho and X parts of those states
        same = np.ascontiguousarray(np.stack([pairs[:, 0], pairs[:, 0]], axis=1))
        last = _t(same)
        srec = lvc_pair_rk4(last, nel, dims, omega, _t(Hel), _t(W), dt, NSTEPS, save_every=NSTEPS, blocks=blocks,
                            path=PATH_ARG[path])
        assert torch.equal(_bits(last[:, 0]), _bits(last[:, 1]))
        own = torch.stack([lvc_observe(_t(same[:, 0]), nel, dims), lvc_observe(last[:, 0].contiguous(), nel, dims)], 1)
        assert torch.equal(_bits(srec), _bits(own[:, :, :nel * nel * (1 + M)].reshape(P, 2, 1 + M, nel, nel)))
    # the plan's own choice is what an unforced call takes
    assert _run(nel, dims, P, "auto")[2] == [PATH_NAME[auto]]
    if RESIDENT not in paths:
        psi = _t(pairs)
        with pytest.raises(ValueError, match="the pair resident path needs D <= "):
            lvc_pair_rk4(psi, nel, dims, omega, _t(Hel), _t(W), dt, NSTEPS, save_every=SE, path="resident")
        assert np.array_equal(psi.cpu().numpy(), pairs)


def test_partial_workgroups_that_sum_several_tiles():
    """(1; 256 LVC_OBS_MAX_GRID + 1), P = 1, staged: one tile more than partial workgroups, so workgroup 0 adds two
    tiles; the record against the oracle and, with bra = ket, lvc_observe's bits."""
    import torch
    from pyqed_amd.mol import lvc_observe, lvc_pair_observe
    lib = _plan_lib()
    nel, dims, P = 1, (lib.TILE * lib.OBS_MAX_GRID + 1,), 1
    p = pair_plan_of(lib, P, nel, dims)
    assert not p.refused and p.base.path == STAGED and p.base.stage.gx == p.part.gx + 1
    psi, rec, noted = _run(nel, dims, P, "staged")
    _, _, _, pairs, _, blocks, (rpsi, rrec) = _case(nel, dims, P)
    assert noted == ["lvc_pair_staged"]
    _check(f"lvc pair nel={nel} dims={dims}", {"final": hp.worst_member(psi.cpu().numpy(), rpsi),
                                               "rec": hp.worst_member(rec.cpu().numpy(), rrec)})
    same = np.ascontiguousarray(np.stack([pairs[:, 0], pairs[:, 0]], axis=1))
    own = lvc_observe(_t(pairs[:, 0]), nel, dims)[:, :2].reshape(P, 2, 1, 1)
    assert torch.equal(_bits(lvc_pair_observe(_t(same), nel, dims, blocks)), _bits(own))


@pytest.mark.parametrize("path", ["staged", "resident"])
def test_call_replays_from_a_graph(path):
    """One qd_lvc_pair_rk4 call captured into a graph and replayed equals the eager call bit for bit."""
    import torch
    from pyqed_amd.mol import lvc_pair_rk4
    nel, dims, P = 3, (3, 5, 7), 3
    omega, Hel, W, pairs, dt, blocks, _ = _case(nel, dims, P)
    dev = torch.device("cuda", 0)
    Hd, Wd = _t(Hel), _t(W)
    psi, rec, _ = _run(nel, dims, P, path)
    x = _t(pairs)
    gr = torch.empty_like(rec)
    s = torch.cuda.Stream(dev)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        lvc_pair_rk4(x, nel, dims, omega, Hd, Wd, dt, NSTEPS, save_every=SE, blocks=blocks, path=path, rec=gr)
    x.copy_(_t(pairs))
    gr.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(_bits(x), _bits(psi)) and torch.equal(_bits(gr), _bits(rec))
