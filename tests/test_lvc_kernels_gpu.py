"""qd_lvc_apply, qd_lvc_rk4 (each admitted path, forced) and qd_lvc_observe (pyqed_amd/csrc/lvc.hip) member by member
against the matrix-free restatement of tests/lvc_models.py in extended precision (tests/test_lvc_host.py earns it its
role on the host).

Inputs: dense random complex Hel and W, not Hermitian (nothing is right by conjugation or by a transposed read), random
normalised states, B in {1, 3}; dt = 0.5 / bound(||H||_1) from the model, so that the comparison is of rounding and not
of RK4 stability; 5 steps saved every 2 (the fifth step is no save).  Asserted: max_b relerr(got[b], ref[b]) < 1e-12,
the bound of tests/test_tdse_tails_gpu.py for the same kind of run, separately for H psi, the final state, every
snapshot and the observable records; the in-run records equal qd_lvc_observe of the snapshots bit for bit; two identical
calls agree bit for bit; the path noted is the plan's.  Where np.longdouble is not extended the float64 restatement is
the reference and the output says so.

Shapes (nel; dims): the smallest models, one mode past a wave, odd extents in two and three modes, nel = 8, six modes,
a fastest axis past the tile (5, 67) and a slow one (65, 3), inert axes (1, 9, 1); one below, at and one above the
plan's tile extent (read from the plan library, not restated); (3; 37, 37), D = 4107, one model past the 4096 at which
the resident LDS would still fit (staged only); and the neighbours of the plan's own limit, the measured crossover,
from the plan."""
import ctypes
import functools

import numpy as np
import pytest

import lvc_models as lm
from conftest import took
from oracle import highprec as hp
from test_lvc_plan_host import RESIDENT, STAGED, build_plan_lib, plan_of

pytestmark = pytest.mark.gpu
BOUND = 1e-12
NSTEPS, SE = 5, 2
PATH_NAME = {STAGED: "lvc_staged", RESIDENT: "lvc_resident"}
PATH_ARG = {STAGED: "staged", RESIDENT: "resident"}
FIXED = [(1, (1,)), (1, (2,)), (3, (70,)), (2, (2, 2)), (3, (3, 5, 7)), (8, (4, 3)), (3, (2, 2, 2, 2, 2, 2)),
         (3, (5, 67)), (3, (65, 3)), (2, (1, 9, 1)), (3, (37, 37))]


@functools.lru_cache(maxsize=None)
def _plan_lib():
    import tempfile
    return build_plan_lib(tempfile.mkdtemp(prefix="lvc_plan_"))


def _shapes():
    """FIXED, then the shapes the plan's constants give.  Collected without the plan library where there is no host
    compiler (the fixture skips then)."""
    try:
        lib = _plan_lib()
    except BaseException:   # pytest.skip raises outside the Exception tree
        return FIXED
    T, L = lib.TILE, lib.RES_MAX_D
    out = list(FIXED)
    out += [(3, (T - 1,)), (3, (T,)), (3, (T + 1,)), (2, (2, T // 2))]            # the tile extent from both sides
    out += [(1, (L,)), (1, (L + 1,)), (3, (L // 3,)), (3, (L // 3 + 1,)), (8, (L // 8,)), (2, (L // 2 // 64, 64))]
    return out


def _t(a):
    import torch
    return torch.from_numpy(np.array(a)).to(torch.device("cuda", 0))   # a copy: the shared inputs are read-only


@functools.lru_cache(maxsize=None)
def _case(nel, dims, B):
    """Inputs and the reference of one (shape, B), computed once and shared by the tests; never written to."""
    omega, Hel, W = lm.random_model(nel, dims)
    psi0 = lm.random_states(B, nel, dims)
    dt = 0.5 / lm.h_bound(dims, omega, Hel, W)
    dtype = np.clongdouble if hp.EXTENDED_OK else np.complex128
    if not hp.EXTENDED_OK:
        print("np.longdouble is not extended here: float64 restatement as the reference")
    ref = lm.rk4(psi0, nel, dims, omega, Hel, W, dt, NSTEPS, SE, dtype=dtype)
    href = lm.apply(psi0, nel, dims, omega, Hel, W, dtype).astype(np.complex128)
    for a in (omega, Hel, W, psi0, href) + ref:
        a.setflags(write=False)
    return omega, Hel, W, psi0, dt, ref, href


def _check(label, errs):
    print(f"{label}: " + ", ".join(f"{k} {e:.2e}" for k, e in errs.items()))
    bad = {k: e for k, e in errs.items() if not e < BOUND}
    assert not bad, (label, bad)


def _admitted(nel, dims, B):
    lib = _plan_lib()
    auto = plan_of(lib, B, nel, dims)
    assert not auto.refused
    paths = [STAGED] + ([RESIDENT] if not plan_of(lib, B, nel, dims, RESIDENT).refused else [])
    return auto.path, paths


def _run(nel, dims, B, path):
    from pyqed_amd.mol import lvc_rk4
    omega, Hel, W, psi0, dt, _, _ = _case(nel, dims, B)
    psi = _t(psi0.copy())
    took("")
    snap, obs = lvc_rk4(psi, nel, dims, omega, _t(Hel), _t(W), dt, NSTEPS, save_every=SE, path=path)
    return psi, snap, obs, took("")[1]


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("nel,dims", _shapes())
def test_apply_and_observe(nel, dims, B):
    from pyqed_amd.mol import lvc_apply, lvc_observe
    omega, Hel, W, psi0, _, ref, href = _case(nel, dims, B)
    got = lvc_apply(_t(psi0), nel, dims, omega, _t(Hel), _t(W)).cpu().numpy()
    rec = lvc_observe(_t(psi0), nel, dims)
    rec2 = lvc_observe(_t(psi0), nel, dims)
    assert rec.shape == (B, lm.nobs(nel, dims))
    import torch
    assert torch.equal(rec.view(torch.float64), rec2.view(torch.float64))
    _check(f"lvc nel={nel} dims={dims} B={B}", {"apply": hp.worst_member(got, href),
                                                 "observe": hp.worst_member(rec.cpu().numpy(), ref[2][:, 0])})


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("nel,dims", _shapes())
def test_rk4_on_each_admitted_path(nel, dims, B):
    import torch
    from pyqed_amd.mol import lvc_observe, lvc_rk4
    omega, Hel, W, psi0, dt, (rpsi, rsnap, robs), _ = _case(nel, dims, B)
    auto, paths = _admitted(nel, dims, B)
    bits = lambda x: x.view(torch.float64)   # noqa: E731
    for path in paths:
        psi, snap, obs, noted = _run(nel, dims, B, PATH_ARG[path])
        assert noted == [PATH_NAME[path]], noted
        assert snap.shape == (B, NSTEPS // SE, lm.size(nel, dims)) and obs.shape == (B, NSTEPS // SE + 1,
                                                                                     lm.nobs(nel, dims))
        errs = {"final": hp.worst_member(psi.cpu().numpy(), rpsi)}
        for k in range(NSTEPS // SE):
            errs[f"snap{k}"] = hp.worst_member(snap[:, k].cpu().numpy(), rsnap[:, k])
        errs["obs"] = hp.worst_member(obs.cpu().numpy(), robs)
        _check(f"lvc nel={nel} dims={dims} B={B} {PATH_NAME[path]}", errs)
        # the in-run records are qd_lvc_observe of the stored states, bit for bit
        assert torch.equal(bits(obs[:, 0]), bits(lvc_observe(_t(psi0), nel, dims)))
        for k in range(NSTEPS // SE):
            assert torch.equal(bits(obs[:, k + 1]), bits(lvc_observe(snap[:, k].contiguous(), nel, dims))), (path, k)
        # an identical call agrees bit for bit
        psi2, snap2, obs2, _ = _run(nel, dims, B, PATH_ARG[path])
        assert torch.equal(bits(psi), bits(psi2)) and torch.equal(bits(snap), bits(snap2))
        assert torch.equal(bits(obs), bits(obs2))
    # the plan's own choice is what an unforced call takes
    assert _run(nel, dims, B, "auto")[3] == [PATH_NAME[auto]]
    if RESIDENT not in paths:
        psi = _t(psi0.copy())
        with pytest.raises(ValueError, match="the resident path needs D <= "):
            lvc_rk4(psi, nel, dims, omega, _t(Hel), _t(W), dt, NSTEPS, save_every=SE, path="resident")
        assert np.array_equal(psi.cpu().numpy(), psi0)


def test_past_the_resident_limit_is_staged_only():
    """(3; 37, 37), D = 4107: the plan goes staged, and forcing the resident path is QD_EINVAL."""
    auto, paths = _admitted(3, (37, 37), 1)
    assert auto == STAGED and paths == [STAGED]


def test_without_snapshots_or_records():
    """snap = NULL and obs = NULL each leave the other output and the state unchanged, on both paths; save_every = 0
    takes no save."""
    import torch
    from pyqed_amd.mol import lvc_rk4
    nel, dims, B = 3, (5, 7), 3
    omega, Hel, W, psi0, dt, _, _ = _case(nel, dims, B)
    bits = lambda x: x.view(torch.float64)   # noqa: E731
    for path in ("staged", "resident"):
        psi, snap, obs, _ = _run(nel, dims, B, path)
        for store, observe in ((False, True), (True, False), (False, False)):
            p = _t(psi0.copy())
            s, o = lvc_rk4(p, nel, dims, omega, _t(Hel), _t(W), dt, NSTEPS, save_every=SE, store=store,
                           observe=observe, path=path)
            assert torch.equal(bits(p), bits(psi)) and (s is None) == (not store) and (o is None) == (not observe)
            assert (s is None or torch.equal(bits(s), bits(snap))) and (o is None or torch.equal(bits(o), bits(obs)))
        p = _t(psi0.copy())
        s, o = lvc_rk4(p, nel, dims, omega, _t(Hel), _t(W), dt, NSTEPS, save_every=0, observe=False, path=path)
        assert s is None and o is None and torch.equal(bits(p), bits(psi))


@pytest.mark.parametrize("path", ["staged", "resident"])
def test_call_replays_from_a_graph(path):
    """One qd_lvc_rk4 call captured into a graph and replayed equals the eager call bit for bit: state, snapshots and
    records."""
    import torch
    from pyqed_amd.mol import lvc_rk4
    nel, dims, B = 3, (3, 5, 7), 3
    omega, Hel, W, psi0, dt, _, _ = _case(nel, dims, B)
    dev = torch.device("cuda", 0)
    Hd, Wd = _t(Hel), _t(W)
    psi, snap, obs, _ = _run(nel, dims, B, path)
    x = _t(psi0.copy())
    gs = torch.empty_like(snap)
    go = torch.empty_like(obs)
    s = torch.cuda.Stream(dev)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        lvc_rk4(x, nel, dims, omega, Hd, Wd, dt, NSTEPS, save_every=SE, path=path, snap=gs, obs=go)
    x.copy_(_t(psi0.copy()))
    gs.zero_()
    go.zero_()
    g.replay()
    torch.cuda.synchronize()
    bits = lambda t: t.view(torch.float64)   # noqa: E731
    assert torch.equal(bits(x), bits(psi)) and torch.equal(bits(gs), bits(snap)) and torch.equal(bits(go), bits(obs))


def test_dims_and_omega_are_read_at_call_time():
    """The host arrays may change right after the call returns: nothing reads them later."""
    import torch
    from pyqed_amd import _lib
    nel, dims, B = 2, (2, 2), 1
    omega, Hel, W, psi0, dt, (rpsi, _, _), _ = _case(nel, dims, B)
    dev = torch.device("cuda", 0)
    _lib.ensure_device(dev)
    d = (ctypes.c_int * 2)(*dims)
    w = (ctypes.c_double * 2)(*omega)
    psi, Hd, Wd = _t(psi0.copy()), _t(Hel), _t(W)
    rc = _lib.load().qd_lvc_rk4(psi.data_ptr(), B, nel, 2, d, w, Hd.data_ptr(), Wd.data_ptr(), dt, NSTEPS, 0, None,
                                None, 0, _lib.stream_ptr(dev))
    d[0], d[1], w[0], w[1] = 999, 999, -1.0, -1.0
    _lib.check(rc, "qd_lvc_rk4")
    assert hp.worst_member(psi.cpu().numpy(), rpsi) < BOUND
