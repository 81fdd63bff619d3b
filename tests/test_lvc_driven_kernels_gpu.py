"""qd_lvc_driven_rk4 (pyqed_amd/csrc/lvc.hip) on each admitted path, forced, member by member against the restatement of
tests/lvc_drive_models.py in extended precision (tests/test_lvc_drive_host.py earns it its role on the host), in the
scheme of tests/test_lvc_kernels_gpu.py.

Inputs: dense random complex Hel, W and A, not Hermitian, random complex fvals, random normalised states, B in {1, 3};
dt = 0.5 / bound with bound = h_bound + sum_d max|f_d| ||mu_d||_1; 5 steps saved every 2.  Asserted: max_b
relerr(got[b], ref[b]) < 1e-12, the project's bound for this kind of run, separately for the final state, every
snapshot and the records; the in-run records equal qd_lvc_observe of the snapshots bit for bit; two identical calls
agree bit for bit; the path noted is the plan's.  Settings: hold 1, 2 (a partial last block), 3 (no multiple of the
save interval), 6 (one row for the whole call), and stage mode.  Shapes and drive sets: lvc_drive_models.gpu_cases, with
the tile extent and the resident limit read from the plan library.  Where np.longdouble is not extended the float64
restatement is the reference and the output says so."""
import ctypes
import functools
import tempfile

import numpy as np
import pytest

import lvc_drive_models as dm
import lvc_models as lm
from conftest import took
from oracle import highprec as hp
from test_lvc_drive_plan_host import AUTO, RESIDENT, STAGED, build_drive_plan_lib, drive_plan_of

pytestmark = pytest.mark.gpu
BOUND = 1e-12
NSTEPS, SE = dm.NSTEPS, dm.SE
PATH_NAME = {STAGED: "lvc_driven_staged", RESIDENT: "lvc_driven_resident"}
PATH_ARG = {STAGED: "staged", RESIDENT: "resident"}
SAMPLE_ARG = {"hold": 0, "stage": 1}


@functools.lru_cache(maxsize=None)
def _plan_lib():
    return build_drive_plan_lib(tempfile.mkdtemp(prefix="lvc_drive_plan_"))


def _cases():
    """Collected without the plan library where there is no host compiler (the tests skip then)."""
    try:
        lib = _plan_lib()
    except BaseException:   # pytest.skip raises outside the Exception tree
        return [(nel, dims, "el") for nel, dims in dm.FIXED]
    return dm.gpu_cases(lib.TILE, lib.RES_MAX_D, lib.limit(6))


def _t(a):
    import torch
    return torch.from_numpy(np.array(a)).to(torch.device("cuda", 0))   # a copy: the shared inputs are read-only


def _bits(x):
    import torch
    return x.view(torch.float64)


@functools.lru_cache(maxsize=None)
def _inputs(nel, dims, name, B):
    out = dm.gpu_inputs(nel, dims, name, B)
    for a in out:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _ref(nel, dims, name, B, sample, hold):
    """The reference of one (case, B, setting), computed once and shared; never written to."""
    omega, Hel, W, A, modes, fvals, psi0, dt = _inputs(nel, dims, name, B)
    dtype = np.clongdouble if hp.EXTENDED_OK else np.complex128
    if not hp.EXTENDED_OK:
        print("np.longdouble is not extended here: float64 restatement as the reference")
    ref = dm.driven_rk4(psi0, nel, dims, omega, Hel, W, A, modes, fvals, dt, NSTEPS, hold, sample, SE, dtype=dtype)
    for a in ref:
        a.setflags(write=False)
    return ref


def _check(label, errs):
    print(f"{label}: " + ", ".join(f"{k} {e:.2e}" for k, e in errs.items()))
    bad = {k: e for k, e in errs.items() if not e < BOUND}
    assert not bad, (label, bad)


def _admitted(nel, dims, B, modes, sample, hold):
    lib = _plan_lib()
    s = SAMPLE_ARG[sample]
    auto = drive_plan_of(lib, B, nel, dims, modes, s, hold)
    assert not auto.refused
    res = drive_plan_of(lib, B, nel, dims, modes, s, hold, path=RESIDENT)
    return auto.base.path, [STAGED] + ([] if res.refused else [RESIDENT])


def _run(nel, dims, name, B, sample, hold, path, drives=True, **kw):
    from pyqed_amd.mol import lvc_driven_rk4
    omega, Hel, W, A, modes, fvals, psi0, dt = _inputs(nel, dims, name, B)
    psi = _t(psi0.copy())
    took("")
    args = (_t(A), modes, _t(fvals)) if drives else (None, [], None)
    snap, obs = lvc_driven_rk4(psi, nel, dims, omega, _t(Hel), _t(W), *args, dt, NSTEPS, hold=hold, sample=sample,
                               save_every=SE, path=path, **kw)
    return psi, snap, obs, took("")[1]


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("nel,dims,name", _cases())
def test_driven_rk4_on_each_admitted_path(nel, dims, name, B):
    import torch
    from pyqed_amd.mol import lvc_driven_rk4, lvc_observe
    omega, Hel, W, A, modes, fvals, psi0, dt = _inputs(nel, dims, name, B)
    for sample, hold in dm.SETTINGS:
        rpsi, rsnap, robs = _ref(nel, dims, name, B, sample, hold)
        auto, paths = _admitted(nel, dims, B, modes, sample, hold)
        for path in paths:
            psi, snap, obs, noted = _run(nel, dims, name, B, sample, hold, PATH_ARG[path])
            assert noted == [PATH_NAME[path]], noted
            assert snap.shape == (B, NSTEPS // SE, lm.size(nel, dims))
            assert obs.shape == (B, NSTEPS // SE + 1, lm.nobs(nel, dims))
            errs = {"final": hp.worst_member(psi.cpu().numpy(), rpsi)}
            for k in range(NSTEPS // SE):
                errs[f"snap{k}"] = hp.worst_member(snap[:, k].cpu().numpy(), rsnap[:, k])
            errs["obs"] = hp.worst_member(obs.cpu().numpy(), robs)
            _check(f"lvc driven nel={nel} dims={dims} {name} B={B} {sample} hold={hold} {PATH_NAME[path]}", errs)
            # the in-run records are qd_lvc_observe of the stored states, bit for bit
            assert torch.equal(_bits(obs[:, 0]), _bits(lvc_observe(_t(psi0), nel, dims)))
            for k in range(NSTEPS // SE):
                assert torch.equal(_bits(obs[:, k + 1]), _bits(lvc_observe(snap[:, k].contiguous(), nel, dims))), \
                    (path, k)
            # an identical call agrees bit for bit
            psi2, snap2, obs2, _ = _run(nel, dims, name, B, sample, hold, PATH_ARG[path])
            assert torch.equal(_bits(psi), _bits(psi2)) and torch.equal(_bits(snap), _bits(snap2))
            assert torch.equal(_bits(obs), _bits(obs2))
        # the plan's own choice is what an unforced call takes
        assert _run(nel, dims, name, B, sample, hold, "auto")[3] == [PATH_NAME[auto]]
        if RESIDENT not in paths:
            psi = _t(psi0.copy())
            with pytest.raises(ValueError, match="qd_lvc_driven_rk4: the resident path needs D <= "):
                lvc_driven_rk4(psi, nel, dims, omega, _t(Hel), _t(W), _t(A), modes, _t(fvals), dt, NSTEPS, hold=hold,
                               sample=sample, save_every=SE, path="resident")
            assert np.array_equal(psi.cpu().numpy(), psi0)


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("nel,dims", [(3, (3, 5, 7)), (3, (65, 3)), (8, (4, 3)), (3, (37, 37)), (1, (2,))])
def test_no_drive_in_hold_mode_is_lvc_rk4_bit_for_bit(nel, dims, B):
    """nd = 0 (A, drive_mode and fvals NULL): state, snapshots and records of qd_lvc_rk4 on the same path."""
    import torch
    from pyqed_amd.mol import lvc_rk4
    omega, Hel, W, _, modes, _, psi0, dt = _inputs(nel, dims, "el", B)
    _, paths = _admitted(nel, dims, B, (), "hold", 1)
    for path in paths:
        for hold in (1, 3):
            psi, snap, obs, noted = _run(nel, dims, "el", B, "hold", hold, PATH_ARG[path], drives=False)
            assert noted == [PATH_NAME[path]]
            ref = _t(psi0.copy())
            rsnap, robs = lvc_rk4(ref, nel, dims, omega, _t(Hel), _t(W), dt, NSTEPS, save_every=SE, path=PATH_ARG[path])
            assert torch.equal(_bits(psi), _bits(ref)), (path, hold)
            assert torch.equal(_bits(snap), _bits(rsnap)) and torch.equal(_bits(obs), _bits(robs)), (path, hold)


def test_a_drive_on_an_inert_axis_changes_nothing():
    """x_j of an axis of extent 1 is zero: a drive on it leaves the run what it is without the drive, on both paths and
    in both modes."""
    nel, dims, B = 2, (1, 9, 1), 3
    for sample, hold in (("hold", 2), ("stage", 1)):
        for path in ("staged", "resident"):
            a = _run(nel, dims, "inert", B, sample, hold, path)
            b = _run(nel, dims, "inert", B, sample, hold, path, drives=False)
            errs = {"final": hp.worst_member(a[0].cpu().numpy(), b[0].cpu().numpy()),
                    "snap": hp.worst_member(a[1].cpu().numpy(), b[1].cpu().numpy()),
                    "obs": hp.worst_member(a[2].cpu().numpy(), b[2].cpu().numpy())}
            _check(f"inert drive {sample} {path}", errs)


def test_past_the_resident_limit_is_staged_only():
    """(3; 37, 37), D = 4107: the plan goes staged, and forcing the resident path is QD_EINVAL."""
    auto, paths = _admitted(3, (37, 37), 1, (-1,), "hold", 1)
    assert auto == STAGED and paths == [STAGED]
    assert _admitted(3, (5, 7), 1, (-1,), "stage", 1) == (RESIDENT, [STAGED, RESIDENT])


@pytest.mark.parametrize("sample,hold", [("hold", 2), ("stage", 1)])
def test_without_snapshots_or_records(sample, hold):
    """snap = NULL and obs = NULL each leave the other output and the state unchanged, on both paths; save_every = 0
    takes no save."""
    import torch
    nel, dims, B, name = 3, (5, 7), 3, "ends"
    for path in ("staged", "resident"):
        psi, snap, obs, _ = _run(nel, dims, name, B, sample, hold, path)
        for store, observe in ((False, True), (True, False), (False, False)):
            p, s, o, _ = _run(nel, dims, name, B, sample, hold, path, store=store, observe=observe)
            assert torch.equal(_bits(p), _bits(psi)) and (s is None) == (not store) and (o is None) == (not observe)
            assert (s is None or torch.equal(_bits(s), _bits(snap))) and (o is None or torch.equal(_bits(o), _bits(obs)))


@pytest.mark.parametrize("sample,hold", [("hold", 2), ("stage", 1)])
@pytest.mark.parametrize("path", ["staged", "resident"])
def test_call_replays_from_a_graph_with_the_field_of_the_moment(path, sample, hold):
    """One call captured into a graph and replayed equals the eager call bit for bit; after fvals is overwritten in
    place a replay equals the eager call with the new field: fvals is read when the kernels run."""
    import torch
    from pyqed_amd.mol import lvc_driven_rk4
    nel, dims, B, name = 3, (3, 5, 7), 3, "eight"
    omega, Hel, W, A, modes, fvals, psi0, dt = _inputs(nel, dims, name, B)
    dev = torch.device("cuda", 0)
    Hd, Wd, Ad, fd = _t(Hel), _t(W), _t(A), _t(fvals)
    f2 = np.ascontiguousarray(fvals[::-1] * (0.5 + 0.25j))      # the same bound holds
    kw = dict(hold=hold, sample=sample, save_every=SE, path=path)

    def eager(f):
        p = _t(psi0.copy())
        s, o = lvc_driven_rk4(p, nel, dims, omega, Hd, Wd, Ad, modes, _t(f), dt, NSTEPS, **kw)
        return p, s, o

    e1, e2 = eager(fvals), eager(f2)
    assert not torch.equal(_bits(e1[0]), _bits(e2[0]))
    x = _t(psi0.copy())
    gs, go = torch.empty_like(e1[1]), torch.empty_like(e1[2])
    s = torch.cuda.Stream(dev)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        lvc_driven_rk4(x, nel, dims, omega, Hd, Wd, Ad, modes, fd, dt, NSTEPS, snap=gs, obs=go, **kw)
    for f, want in ((None, e1), (f2, e2)):
        x.copy_(_t(psi0.copy()))
        gs.zero_()
        go.zero_()
        if f is not None:
            fd.copy_(_t(f))
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(_bits(x), _bits(want[0])) and torch.equal(_bits(gs), _bits(want[1]))
        assert torch.equal(_bits(go), _bits(want[2]))


def test_host_arrays_are_read_at_call_time():
    """drive_mode, dims and omega may change right after the call returns: nothing reads them later."""
    import torch
    from pyqed_amd import _lib
    nel, dims, B, name = 3, (5, 7), 1, "ends"
    omega, Hel, W, A, modes, fvals, psi0, dt = _inputs(nel, dims, name, B)
    dev = torch.device("cuda", 0)
    _lib.ensure_device(dev)
    for sample, hold, path in (("hold", 2, 1), ("stage", 1, 2)):
        rpsi = _ref(nel, dims, name, B, sample, hold)[0]
        d = (ctypes.c_int * 2)(*dims)
        w = (ctypes.c_double * 2)(*omega)
        md = (ctypes.c_int * 2)(*modes)
        psi, Hd, Wd, Ad, fd = _t(psi0.copy()), _t(Hel), _t(W), _t(A), _t(fvals)
        rc = _lib.load().qd_lvc_driven_rk4(psi.data_ptr(), B, nel, 2, d, w, Hd.data_ptr(), Wd.data_ptr(), 2,
                                           Ad.data_ptr(), md, fd.data_ptr(), fvals.shape[0], SAMPLE_ARG[sample], hold,
                                           dt, NSTEPS, 0, None, None, path, _lib.stream_ptr(dev))
        d[0], d[1], w[0], w[1], md[0], md[1] = 999, 999, -1.0, -1.0, -1, -1
        _lib.check(rc, "qd_lvc_driven_rk4")
        assert hp.worst_member(psi.cpu().numpy(), rpsi) < BOUND
