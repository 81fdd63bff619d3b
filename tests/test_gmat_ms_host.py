"""Coupled-surface curvilinear propagation without a GPU: the numpy restatement of tests/gmat_ms_models.py against
the single-surface restatement and against the dense propagator, the argument checks of qd_wp2_gmat_ms_apply /
qd_wp2_gmat_ms_rk4, and the Python refusals, all of which happen before any device call."""
import numpy as np
import pytest
import scipy.linalg

from conftest import relerr
import gmat_models as gm
import gmat_ms_models as gms
from test_gmat_host import APPLY_OK, BAD_COMMON, RK4_OK


def test_one_state_is_the_single_surface_restatement():
    m = gm.model(16, 16)
    one = gms.model_ms(16, 16, 1)
    assert np.array_equal(one["V"][..., 0, 0], m["v"]) and np.array_equal(one["psi0"][..., 0], m["psi0"])
    got = gms.run_ms_ref(m["psi0"][..., None], m["dt"], 3, m["kx"], m["ky"], m["v"][..., None, None], m["G"])
    assert np.array_equal(got[..., 0], gm.run_ref(m["psi0"], m["dt"], 3, m["kx"], m["ky"], m["v"], m["G"]))
    got = gms.run_ms_ref(one["psi0"], m["dt"], 3, m["kx"], m["ky"], one["V"], m["G"])
    assert np.array_equal(got[..., 0], gm.run_ref(m["psi0"], m["dt"], 3, m["kx"], m["ky"], m["v"], m["G"]))


def test_uncoupled_states_follow_their_own_surfaces():
    m = gms.model_ms(32, 16, 3)
    V = gms.block_diagonal(m["V"])
    assert np.count_nonzero(m["V"][..., 0, 1]) and not np.count_nonzero(V[..., 0, 1])
    got = gms.run_ms_ref(m["psi0"], m["dt"], 4, m["kx"], m["ky"], V, m["G"])
    for a in range(3):
        ref = gm.run_ref(m["psi0"][..., a], m["dt"], 4, m["kx"], m["ky"], V[..., a, a], m["G"])
        assert relerr(got[..., a], ref) <= 1e-14, a


def test_model_time_step_bounds_the_operator():
    """dt = 1 / lam with lam >= ||H||: the largest |eigenvalue| of the dense H of a small model is below lam."""
    m = gms.model_ms(8, 8, 2)
    n = m["psi0"].size
    H = np.empty((n, n), dtype=complex)
    for k in range(n):
        e = np.zeros(n, dtype=complex)
        e[k] = 1.0
        H[:, k] = 1j * gms.hpsi_ms_ref(e.reshape(m["psi0"].shape), m["kx"], m["ky"], m["V"], m["G"]).ravel()
    assert np.abs(np.linalg.eigvals(H)).max() <= m["lam"] and np.isclose(m["dt"] * m["lam"], 1.0)


def test_restatement_integrates_the_coupled_equation():
    """16 x 16, ns = 2, symmetric G, Hermitian V: H built from hpsi_ms_ref on unit vectors is Hermitian to rounding, and
    nt = 8 steps of dt = 0.05 / lam match expm(-i H nt dt) psi0 within nt theta^5 / 120 e^theta + 1e-12, theta = 0.05:
    RK4's Taylor remainder per step, summed for a unitary propagator (about 2e-8)."""
    m = gms.model_ms(16, 16, 2)
    G = m["G"].copy()
    G[..., 1, 0] = G[..., 0, 1]
    theta, nt = 0.05, 8
    dt = theta / m["lam"]
    shape, n = m["psi0"].shape, m["psi0"].size
    assert n == 512
    H = np.empty((n, n), dtype=complex)
    for k in range(n):
        e = np.zeros(n, dtype=complex)
        e[k] = 1.0
        H[:, k] = 1j * gms.hpsi_ms_ref(e.reshape(shape), m["kx"], m["ky"], m["V"], G).ravel()
    scale = np.abs(H).max()
    assert np.abs(H - H.conj().T).max() <= 1e-13 * scale
    assert np.linalg.norm(H, 2) <= m["lam"]
    exact = scipy.linalg.expm(-1j * H * (nt * dt)) @ m["psi0"].ravel()
    got = gms.run_ms_ref(m["psi0"], dt, nt, m["kx"], m["ky"], m["V"], G)[-1].ravel()
    bound = nt * theta ** 5 / 120.0 * np.exp(theta) + 1e-12
    err = relerr(got, exact)
    print(f"restatement vs expm: err {err:.3e} bound {bound:.3e}")
    assert err <= bound
    # the coupling moves population: the restatement is not two uncoupled runs
    assert relerr(got, gms.run_ms_ref(m["psi0"], dt, nt, m["kx"], m["ky"], gms.block_diagonal(m["V"]), G)[-1].ravel()) \
        > 100 * bound


# the argument lists of test_gmat_host.py with ns after B
def _ms(args, **extra):
    out = {}
    for k, v in {**args, **extra}.items():
        out[k] = v
        if k == "B":
            out["ns"] = extra.get("ns", args.get("ns", 2))
    return out


BAD_MS = BAD_COMMON + [dict(ns=0), dict(ns=-1), dict(B=4, ns=2, nx=16384, ny=16384), dict(ns=4, nx=16384, ny=16384)]


@pytest.mark.parametrize("bad", BAD_MS + [dict(out=None), dict(out=APPLY_OK["psi"])], ids=str)
def test_ms_apply_rejects_invalid_arguments(bad):
    from pyqed_amd import _lib
    lib = _lib.load()
    assert hasattr(lib, "qd_wp2_gmat_ms_apply")
    rc = lib.qd_wp2_gmat_ms_apply(*_ms(APPLY_OK, **bad).values())
    assert rc == _lib.QD_EINVAL
    assert "qd_wp2_gmat_ms_apply" in _lib.last_error()


@pytest.mark.parametrize("bad", BAD_MS + [dict(nout=0), dict(nsteps=-1)], ids=str)
def test_ms_rk4_rejects_invalid_arguments(bad):
    from pyqed_amd import _lib
    lib = _lib.load()
    assert hasattr(lib, "qd_wp2_gmat_ms_rk4")
    rc = lib.qd_wp2_gmat_ms_rk4(*_ms(RK4_OK, **bad).values())
    assert rc == _lib.QD_EINVAL
    assert "qd_wp2_gmat_ms_rk4" in _lib.last_error()


def test_ms_argument_lists_are_in_abi_order():
    assert list(_ms(APPLY_OK)) == ["psi", "B", "ns", "G", "v", "kx", "ky", "nx", "ny", "out", "stream"]
    assert list(_ms(RK4_OK, ns=0))[:3] == ["psi", "B", "ns"] and _ms(RK4_OK, ns=0)["ns"] == 0


def test_ms_rk4_zero_steps_is_a_no_op_without_a_device():
    from pyqed_amd import _lib
    assert _lib.load().qd_wp2_gmat_ms_rk4(*_ms(RK4_OK, nsteps=0).values()) == _lib.QD_OK


def test_ms_operator_refusals_need_no_device():
    import torch
    from pyqed_amd.wpd import curvilinear_run, hpsi
    m = gms.model_ms(16, 16, 2)
    x, y, psi, V, G = m["x"], m["y"], m["psi0"], m["V"], m["G"]
    for wrong in (V[:8], V[:, :8], V[..., :1], np.zeros((16, 16, 2, 3))):
        with pytest.raises(ValueError, match=r"v must be \[nx, ny, ns, ns\]"):
            hpsi(psi, m["kx"], m["ky"], wrong, G)
        with pytest.raises(ValueError, match=r"v must be \[nx, ny, ns, ns\]"):
            curvilinear_run(x, y, psi, wrong, G, m["dt"], 2)
    for wrong in (psi[..., :1], psi[..., 0], np.zeros((3, 16, 16, 3), complex), np.zeros((1, 3, 16, 16, 2), complex)):
        with pytest.raises(ValueError, match=r"psi \[nx, ny, ns\] or a batch \[B, nx, ny, ns\]"):
            hpsi(wrong, m["kx"], m["ky"], V, G)
        with pytest.raises(ValueError, match=r"psi \[nx, ny, ns\] or a batch \[B, nx, ny, ns\]"):
            curvilinear_run(x, y, torch.from_numpy(np.ascontiguousarray(wrong)), V, G, m["dt"], 2)
    with pytest.raises(ValueError, match="metric G"):
        hpsi(psi, m["kx"], m["ky"], V, None)
    with pytest.raises(ValueError, match="G must be"):
        hpsi(psi, m["kx"], m["ky"], V, G[:, :8])
    with pytest.raises(ValueError, match="real"):
        curvilinear_run(x, y, psi, V, G + 0.01j, m["dt"], 2)
    with pytest.raises(ValueError, match="lengths"):
        hpsi(psi, m["kx"][:4], m["ky"], V, G)
    with pytest.raises(ValueError, match="nout"):
        curvilinear_run(x, y, psi, V, G, m["dt"], 2, nout=0)


def test_spo2_curvilinear_refusals_need_no_device():
    from pyqed_amd.wpd import SPO2, SPO2NH, SPO3
    m = gms.model_ms(16, 16, 2)
    x, y, G = m["x"], m["y"], m["G"]
    for bad, msg in ((None, "metric G"), (G + 0.01j, "real"), (G[:, :8], "G must be"), (G[..., 0], "G must be")):
        sol = SPO2(x, y, nstates=2, coords="curvilinear", G=bad)
        sol.set_dpes(m["V"])
        with pytest.raises(ValueError, match=msg):
            sol.build(m["dt"])
        with pytest.raises(ValueError, match=msg):
            sol.run(m["psi0"], dt=m["dt"], nt=2)
    sol = SPO2(x, y, nstates=2, coords="curvilinear", G=G)
    sol.build(m["dt"])   # forms kx, ky and checks G; no propagators
    assert np.array_equal(sol.kx, m["kx"]) and np.array_equal(sol.ky, m["ky"])
    assert sol.exp_K is None and sol.exp_V is None and sol.exp_V_half is None
    with pytest.raises(ValueError, match="PES is not specified"):
        sol.run(m["psi0"], dt=m["dt"], nt=2)
    sol.set_dpes(m["V"])
    with pytest.raises(ValueError, match=r"psi0s must be \[B, 16, 16, 2\]"):
        sol.run(m["psi0"][..., :1], dt=m["dt"], nt=2)
    with pytest.raises(ValueError, match=r"psi0s must be \[B, 16, 16, 2\]"):
        sol.run_batch(m["psi0"], dt=m["dt"], nt=2)
    with pytest.raises(ValueError, match="unknown coordinates"):
        SPO2(x, y, nstates=2, coords="polar", G=G).build(m["dt"])
    nh = SPO2NH(x, y, nstates=2, coords="curvilinear", G=G)
    nh.set_dpes(m["V"])
    with pytest.raises(NotImplementedError, match="non-Hermitian class is not covered"):
        nh.build(m["dt"])
    with pytest.raises(NotImplementedError, match="non-Hermitian class is not covered"):
        nh.run(m["psi0"], dt=m["dt"], nt=2)
    s3 = SPO3(x, y, y, [1, 1, 1], nstates=2, coords="curvilinear", G=G)
    with pytest.raises(NotImplementedError, match="3-D metric"):
        s3.build(m["dt"])
    with pytest.raises(NotImplementedError, match="3-D metric"):
        s3.run(np.zeros((16, 16, 16, 2), complex), dt=m["dt"], nt=2)
