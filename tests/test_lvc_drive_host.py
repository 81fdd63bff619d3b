"""Laser-driven LVC runs on the host (no GPU): the restatement of qd_lvc_driven_rk4 in tests/lvc_drive_models.py in both
sampling modes against a dense propagation with dense_h(...) - sum_d f_d mu_d from Kronecker products; the float64
restatement against the long-double one on every case of tests/test_lvc_driven_kernels_gpu.py (what the 1e-12 of that
test leaves to the kernels); the order of both modes on one fixed model; every refusal of the class surface and of the
C entry's argument checks that needs no device."""
import ctypes
import functools
import tempfile

import numpy as np
import pytest

import lvc_drive_models as dm
import lvc_models as lm
from oracle import highprec as hp
from test_lvc_drive_plan_host import build_drive_plan_lib


@pytest.mark.parametrize("sample,hold", [("hold", 1), ("hold", 2), ("hold", 4), ("stage", 1)])
@pytest.mark.parametrize("nel,dims,modes", [(2, (3, 4), [-1, 1]), (2, (3, 4), [0, -1, 0]), (3, (2, 2, 2), [2, -1, 0]),
                                            (3, (2, 2, 2), [-1, 1, -1, -1])])
def test_restatement_against_dense_propagation(nel, dims, modes, sample, hold):
    """Condon and Herzberg-Teller drives, several on one table, non-Hermitian everything, complex field."""
    nsteps = 5
    omega, Hel, W = lm.random_model(nel, dims)
    A, fvals = dm.random_drives(nel, dims, modes, 2 * nsteps + 1)
    psi0 = lm.random_states(2, nel, dims)
    dt = 0.5 / dm.drive_bound(dims, omega, Hel, W, A, modes, fvals)
    H0 = lm.dense_h(nel, dims, omega, Hel, W)
    mus = [dm.dense_mu(nel, dims, A[d], k) for d, k in enumerate(modes)]
    ref = dm.dense_driven_rk4(psi0, H0, mus, fvals, dt, nsteps, hold, sample)
    dtypes = (np.complex128, np.clongdouble) if hp.EXTENDED_OK else (np.complex128,)
    for dtype in dtypes:
        psi, snap, obs = dm.driven_rk4(psi0, nel, dims, omega, Hel, W, A, modes, fvals, dt, nsteps, hold, sample, 2,
                                       dtype=dtype)
        assert hp.worst_member(psi, ref) < 1e-14, (dtype, hp.worst_member(psi, ref))
        assert snap.shape == (2, 2, lm.size(nel, dims)) and obs.shape == (2, 3, lm.nobs(nel, dims))
        assert np.array_equal(obs[:, 1], lm.record(snap[:, 0], nel, dims, np.complex128)) or dtype != np.complex128
    # the field matters: without it the answer is another one
    free = dm.dense_driven_rk4(psi0, H0, [], fvals, dt, nsteps, hold, sample)
    assert hp.worst_member(free, ref) > 1e-3
    # with no drive, hold mode is lvc_models.rk4 itself
    a, b = dm.driven_rk4(psi0, nel, dims, omega, Hel, W, A[:0], [], None, dt, nsteps, hold)[0], \
        lm.rk4(psi0, nel, dims, omega, Hel, W, dt, nsteps)[0]
    assert np.array_equal(a, b)


@functools.lru_cache(maxsize=None)
def _plan_lib():
    return build_drive_plan_lib(tempfile.mkdtemp(prefix="lvc_drive_plan_"))


def test_float64_restatement_on_the_gpu_cases():
    """On every case of the GPU kernel test the float64 restatement is within 1e-12 of the long-double one: the
    bound of that test is about the kernels, not about the conditioning of the cases."""
    if not hp.EXTENDED_OK:
        pytest.skip("np.longdouble is not extended here")
    lib = _plan_lib()
    worst = (0.0, None)
    for nel, dims, name in dm.gpu_cases(lib.TILE, lib.RES_MAX_D, lib.limit(6)):
        omega, Hel, W, A, modes, fvals, psi0, dt = dm.gpu_inputs(nel, dims, name, 3)
        for sample, hold in dm.SETTINGS:
            lo = dm.driven_rk4(psi0, nel, dims, omega, Hel, W, A, modes, fvals, dt, dm.NSTEPS, hold, sample, dm.SE)
            hi = dm.driven_rk4(psi0, nel, dims, omega, Hel, W, A, modes, fvals, dt, dm.NSTEPS, hold, sample, dm.SE,
                               dtype=np.clongdouble)
            e = max(hp.worst_member(a, b) for a, b in zip(lo, hi))
            worst = max(worst, (e, (nel, dims, name, sample, hold)))
    print(f"float64 against long double, worst over the GPU cases: {worst[0]:.2e} at {worst[1]}")
    assert worst[0] < 1e-12, worst


def test_orders_of_the_two_sampling_modes():
    """nel = 2, one mode of 8 levels, mu = sigma_x (x) 1, a Gaussian pulse over T = 20 from |0, 0>; the reference is
    stage mode at 6400 steps.  From 100 to 200 steps the stage-mode error falls by more than 12 (order 4: 16), the
    hold-mode error by between 1.7 and 2.4 (order 1: 2)."""
    ref = dm.order_run("stage", dm.ORDER["nref"])
    err = {(s, n): float(np.linalg.norm(dm.order_run(s, n) - ref)) for s in ("stage", "hold") for n in (100, 200)}
    r_stage = err["stage", 100] / err["stage", 200]
    r_hold = err["hold", 100] / err["hold", 200]
    print(f"stage {err['stage', 100]:.2e} -> {err['stage', 200]:.2e} ratio {r_stage:.2f}; "
          f"hold {err['hold', 100]:.2e} -> {err['hold', 200]:.2e} ratio {r_hold:.2f}")
    assert r_stage > 12 and 1.7 < r_hold < 2.4


class _VecPulse:
    def E(self, t):
        return np.array([0.1, 0.0, 0.2]) * np.cos(t)

    def efield(self, t):
        return 0.1 * np.cos(t)


def test_class_refusals_before_any_device_work():
    from pyqed_amd import LVC, LVCOp, Mode
    mol = LVC([0.0, 1.0], [Mode(0.1, [], truncate=3), Mode(0.2, [], truncate=2)])
    sol = mol.wavepacket_dynamics()
    p = _VecPulse()
    kw = dict(dt=0.1, Nt=4)
    with pytest.raises(ValueError, match="sample='midpoint', expected 'hold' or 'stage'"):
        sol.run(pulse=p, edip=mol.buildop(0, 1), sample="midpoint", **kw)
    with pytest.raises(ValueError, match="sample='x', expected 'hold' or 'stage'"):
        sol.run_batch(np.zeros((1, 12)), pulse=p, edip=mol.buildop(0, 1), sample="x", **kw)
    with pytest.raises(ValueError, match="edip is an LVCOp of another space"):
        sol.run(pulse=p, edip=LVCOp(np.eye(2), (3, 3)), **kw)
    with pytest.raises(ValueError, match="edip is an LVCOp of another space"):
        sol.run(pulse=p, edip=LVCOp(np.eye(3), (2, 2)), **kw)
    with pytest.raises(ValueError, match=r"edip\[1\] is an LVCOp of another space"):
        sol.run(pulse=[p, p], edip=[mol.buildop(0, 1), LVCOp(np.eye(2), (2, 3))], **kw)
    with pytest.raises(ValueError, match="a list of pulses needs a list of as many dipoles"):
        sol.run(pulse=[p, p], edip=[mol.buildop(0, 1)], **kw)
    with pytest.raises(ValueError, match=r"edip has shape \(3, 3\)"):
        sol.run(pulse=p, edip=np.eye(3), **kw)
    with pytest.raises(ValueError, match=r"edip has shape \(3, 3, 3\)"):
        sol.run(pulse=p, edip=np.zeros((3, 3, 3)), **kw)
    with pytest.raises(ValueError, match="Electric dipole must be provided"):
        sol.run(pulse=p, **kw)
    with pytest.raises(ValueError, match="sample='stage' needs the dipole as factors"):
        sol.run(pulse=p, edip=np.eye(12), sample="stage", **kw)
    with pytest.raises(ValueError, match="a D x D dipole has no matrix-free form"):
        sol.run_batch(np.zeros((1, 12)), pulse=p, edip=np.eye(12), **kw)
    from pyqed_amd.mol import lvc_driven_rk4
    with pytest.raises(ValueError, match="sample='rk2'"):
        lvc_driven_rk4(None, 2, (3, 2), (0.1, 0.2), None, None, None, [], None, 0.1, 1, sample="rk2")


def test_c_refusals_before_any_device_work():
    """QD_EINVAL with the entry point's message; no pointer is read and no device call is made (this runs without a
    GPU).  The plan's messages are enumerated in tests/test_lvc_drive_plan_host.py."""
    from pyqed_amd import _lib
    lib = _lib.load()
    one = ctypes.c_void_p(16)    # never dereferenced
    ints = lambda *v: (ctypes.c_int * len(v))(*v)   # noqa: E731
    om = (ctypes.c_double * 6)(*([1.0] * 6))

    def run(B=1, nel=3, M=2, dims=ints(4, 4), nd=2, A=one, modes=ints(-1, 1), fvals=one, nf=11, sample=0, hold=1,
            nsteps=5, se=1, obs=None, path=0, psi=one, omega=om, Hel=one, W=one):
        return lib.qd_lvc_driven_rk4(psi, B, nel, M, dims, omega, Hel, W, nd, A, modes, fvals, nf, sample, hold, 0.1,
                                     nsteps, se, None, obs, path, None)

    F = "qd_lvc_driven_rk4: "
    cases = ((dict(nd=-1), "nd=-1 outside [0, 8]"), (dict(nd=9), "nd=9 outside [0, 8]"),
             (dict(modes=ints(-1, 2)), "drive_mode[1]=2 outside [-1, 2)"),
             (dict(modes=ints(-2, 0)), "drive_mode[0]=-2 outside [-1, 2)"),
             (dict(modes=None), "null drive_mode"),
             (dict(sample=2), "sample=2 outside {0, 1}"), (dict(hold=0), "hold=0 must be at least 1"),
             (dict(nf=2, hold=2), "fvals holds 2 rows, 3 are needed (ceil(nsteps / hold))"),
             (dict(nf=10, sample=1), "fvals holds 10 rows, 11 are needed (2 nsteps + 1)"),
             (dict(A=None), "null A or fvals with nd=2"), (dict(fvals=None), "null A or fvals with nd=2"),
             (dict(psi=None), "null pointer"), (dict(omega=None), "null pointer"), (dict(Hel=None), "null pointer"),
             (dict(W=None), "null pointer"), (dict(dims=None), "null dims"),
             (dict(nel=0), "nel=0 outside [1, 8]"), (dict(nel=9), "nel=9 outside [1, 8]"),
             (dict(M=0), "M=0 outside [1, 6]"), (dict(M=7), "M=7 outside [1, 6]"),
             (dict(dims=ints(2, 0)), "dims[1]=0 must be at least 1"),
             (dict(nel=2, M=3, dims=ints(1024, 1024, 1024)), "D = nel * prod(dims) must stay below 2^31"),
             (dict(B=0), "B=0 outside [1, 65535]"), (dict(B=65536), "B=65536 outside [1, 65535]"),
             (dict(path=3), "path=3 outside [0, 2]"),
             (dict(nsteps=-1), "nsteps=-1 and save_every=1 must not be negative"),
             (dict(se=0, obs=one), "observables need save_every > 0"),
             (dict(dims=ints(37, 37), path=2), "the resident path needs D <= 2048 with 2 modes (D = 4107)"),
             (dict(M=6, dims=ints(1, 1, 1, 1, 1, 513), path=2, modes=ints(-1, 5)),
              "the resident path needs D <= 1536 with 6 modes (D = 1539)"))
    for kw, msg in cases:
        assert run(**kw) == _lib.QD_EINVAL and _lib.last_error() == F + msg, (kw, _lib.last_error())
