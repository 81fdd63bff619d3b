"""Three-dimensional curvilinear propagation without a GPU: the numpy restatement of tests/gmat3_models.py against an
emulation of the kernels' arithmetic and against closed forms, the argument checks of the four qd_wp3_gmat_* entry
points, and the Python refusals (KEO3, hpsi3, curvilinear_run3, SPO3(coords='curvilinear')), all of which happen
before any device call.

Bounds, in units of fft_cases.tol(n), n the longest axis (test_gmat3_gpu.py states them): 6 for one application of the
operator, nt * 24 for a run."""
import numpy as np
import pytest

from conftest import relerr
import fft_cases as fc
import gmat3_models as g3

SHAPES = [(16, 16, 16), (16, 32, 64), (24, 20, 18), (67, 5, 3), (1, 8, 8)]


def _noise(shape, seed):
    w = fc.noise(np.random.default_rng(seed), shape)
    return w / np.linalg.norm(w)


@pytest.mark.parametrize("shape", SHAPES, ids=str)
@pytest.mark.parametrize("ns", [1, 2])
def test_restatement_against_the_emulation(shape, ns):
    m = g3.model3(*shape, ns=ns)
    nt = 4
    w = _noise(shape + (ns,), 7 + sum(shape) + ns)
    planes, Vp = np.moveaxis(w, -1, 0), np.moveaxis(m["V"], (-2, -1), (0, 1))
    if ns == 1:
        ref_h = g3.hpsi3_ref(w[..., 0], m["ks"], m["v"], m["G"])[..., None]
        ref = g3.run_ref(w[..., 0], m["dt"], nt, m["ks"], m["v"], m["G"])[..., None]
    else:
        ref_h = g3.hpsi3_ref(w, m["ks"], m["V"], m["G"])
        ref = g3.run_ref(w, m["dt"], nt, m["ks"], m["V"], m["G"])
    got_h = -1j * np.moveaxis(g3.emulate_h(planes, m["ks"], Vp, m["G"]), 0, -1)
    got = np.moveaxis(g3.emulate_run(planes, m["dt"], nt, m["ks"], Vp, m["G"]), 1, -1)
    t = fc.tol(max(shape))
    r_h, r_run = relerr(got_h, ref_h) / (6.0 * t), max(relerr(got[k], ref[k]) for k in (1, 3)) / (nt * 24.0 * t)
    print(f"gmat3 emulation {shape} ns={ns}: err/bound operator {r_h:.3e} run {r_run:.3e}")
    assert fc.within(r_h, r_run), (r_h, r_run)


@pytest.mark.parametrize("shape", [(16, 32, 16), (24, 20, 18)], ids=str)
def test_constant_metric_is_the_taylor_symbol(shape):
    """Constant full symmetric metric, v = 0: the nt-step run is ifftn(R(-i dt E_k)^nt fftn psi); every cross term
    G_rs k_r k_s of E_k enters, so an axis mix-up in the restatement shows."""
    m = g3.model3(*shape)
    G0 = np.array([[1.0, 0.2, -0.1], [0.2, 0.8, 0.15], [-0.1, 0.15, 0.9]])
    G = np.broadcast_to(G0, shape + (3, 3)).copy()
    nt = 5
    got = g3.run_ref(m["psi0"], m["dt"], nt, m["ks"], None, G)[-1]
    ref = g3.taylor_run(m["psi0"], m["dt"], nt, m["ks"], G0)
    assert relerr(got, ref) <= nt * 24.0 * fc.tol(max(shape))
    swapped = G0[[1, 0, 2]][:, [1, 0, 2]]
    assert relerr(g3.taylor_run(m["psi0"], m["dt"], nt, m["ks"], swapped), ref) > 1e-6


def test_restatement_is_hermitian_for_a_symmetric_metric():
    """<a|H b> = <H a|b> to rounding for symmetric G and real v; not for the model's own G."""
    shape = (12, 10, 7)
    m = g3.model3(*shape)
    Gs = 0.5 * (m["G"] + np.swapaxes(m["G"], -1, -2))
    a, b = _noise(shape, 1), _noise(shape, 2)
    H = lambda f, G: 1j * g3.hpsi3_ref(f, m["ks"], m["v"], G)
    lhs, rhs = np.vdot(a, H(b, Gs)), np.vdot(H(a, Gs), b)
    scale = np.linalg.norm(H(b, Gs))
    assert abs(lhs - rhs) <= 1e-13 * scale
    assert abs(np.vdot(a, H(b, m["G"])) - np.vdot(H(a, m["G"]), b)) > 1e-6 * scale


def test_model_metric_entries_all_differ():
    G = g3.model3(12, 10, 7)["G"].reshape(-1, 9)
    for r in range(9):
        for s in range(r + 1, 9):
            assert relerr(G[:, r], G[:, s]) > 1e-2, (r, s)


# a valid argument list for each entry point (pointers are never dereferenced: validation comes first)
P = 0x1000
APPLY_OK = dict(psi=P, B=1, G=P, v=None, kx=P, ky=P, kz=P, nx=16, ny=16, nz=16, out=2 * P, stream=None)
RK4_OK = dict(psi=P, B=1, G=P, v=None, kx=P, ky=P, kz=P, nx=16, ny=16, nz=16, dt=0.1, nsteps=1, nout=1, snap=None,
              stream=None)
BAD = [dict(psi=None), dict(G=None), dict(kx=None), dict(ky=None), dict(kz=None), dict(B=0), dict(nx=0), dict(ny=0),
       dict(nz=0), dict(B=-3), dict(B=8, nx=1024, ny=1024, nz=256), dict(nx=2048, ny=1024, nz=1024)]
BAD_MS = BAD + [dict(ns=0), dict(ns=-1), dict(ns=4, nx=1024, ny=1024, nz=128)]


def _ms(args, **extra):
    """The argument list with ns after B."""
    out = {}
    for k, v in {**args, **extra}.items():
        if k != "ns":
            out[k] = v
        if k == "B":
            out["ns"] = extra.get("ns", 2)
    return out


def test_argument_lists_are_in_abi_order():
    assert list(_ms(APPLY_OK)) == ["psi", "B", "ns", "G", "v", "kx", "ky", "kz", "nx", "ny", "nz", "out", "stream"]
    assert list(_ms(RK4_OK, ns=0))[:3] == ["psi", "B", "ns"] and _ms(RK4_OK, ns=0)["ns"] == 0


@pytest.mark.parametrize("bad", BAD_MS + [dict(out=None), dict(out=P)], ids=str)
def test_apply_rejects_invalid_arguments(bad):
    from pyqed_amd import _lib
    lib = _lib.load()
    assert lib.qd_wp3_gmat_ms_apply(*_ms(APPLY_OK, **bad).values()) == _lib.QD_EINVAL
    assert "qd_wp3_gmat_ms_apply" in _lib.last_error()
    if "ns" not in bad:
        assert lib.qd_wp3_gmat_apply(*{**APPLY_OK, **bad}.values()) == _lib.QD_EINVAL
        assert "qd_wp3_gmat_apply" in _lib.last_error()


@pytest.mark.parametrize("bad", BAD_MS + [dict(nout=0), dict(nsteps=-1)], ids=str)
def test_rk4_rejects_invalid_arguments(bad):
    from pyqed_amd import _lib
    lib = _lib.load()
    assert lib.qd_wp3_gmat_ms_rk4(*_ms(RK4_OK, **bad).values()) == _lib.QD_EINVAL
    assert "qd_wp3_gmat_ms_rk4" in _lib.last_error()
    if "ns" not in bad:
        assert lib.qd_wp3_gmat_rk4(*{**RK4_OK, **bad}.values()) == _lib.QD_EINVAL
        assert "qd_wp3_gmat_rk4" in _lib.last_error()


def test_rk4_zero_steps_is_a_no_op_without_a_device():
    from pyqed_amd import _lib
    assert _lib.load().qd_wp3_gmat_rk4(*{**RK4_OK, "nsteps": 0}.values()) == _lib.QD_OK
    assert _lib.load().qd_wp3_gmat_ms_rk4(*_ms(RK4_OK, nsteps=0).values()) == _lib.QD_OK


def test_operator_refusals_need_no_device():
    import torch
    from pyqed_amd.wpd import KEO3, curvilinear_run3, hpsi3
    m = g3.model3(16, 16, 16, ns=2)
    x, y, z, G, v, V = m["x"], m["y"], m["z"], m["G"], m["v"], m["V"]
    ks = m["ks"]
    one, two = m["psi0"][..., 0], m["psi0"]
    for bad, msg in ((None, "metric G"), (G + 0.01j, "real"), (G[:, :8], "G must be"), (G[..., 0], "G must be"),
                     (G[..., :2, :2], "G must be"), (torch.from_numpy(G) * (1 + 0.5j), "real")):
        with pytest.raises(ValueError, match=msg):
            KEO3(one, *ks, bad)
        with pytest.raises(ValueError, match=msg):
            hpsi3(two, *ks, V, bad)
        with pytest.raises(ValueError, match=msg):
            curvilinear_run3(x, y, z, one, v, bad, m["dt"], 2)
    for wrong in (one[0], np.zeros((2, 2, 16, 16, 16), complex)):
        with pytest.raises(ValueError, match="psi must be"):
            KEO3(wrong, *ks, G)
    with pytest.raises(ValueError, match="v must be"):
        hpsi3(one, *ks, v[:8], G)
    for wrong in (V[:8], V[..., :1], np.zeros((16, 16, 16, 2, 3))):
        with pytest.raises(ValueError, match=r"v must be \[nx, ny, nz, ns, ns\]"):
            hpsi3(two, *ks, wrong, G)
        with pytest.raises(ValueError, match=r"v must be \[nx, ny, nz, ns, ns\]"):
            curvilinear_run3(x, y, z, two, wrong, G, m["dt"], 2)
    for wrong in (two[..., :1], np.zeros((16, 16, 16), complex), np.zeros((1, 3, 16, 16, 16, 2), complex)):
        with pytest.raises(ValueError, match=r"psi \[nx, ny, nz, ns\] or a batch"):
            hpsi3(wrong, *ks, V, G)
    with pytest.raises(ValueError, match="lengths"):
        hpsi3(one, ks[0][:4], ks[1], ks[2], v, G)
    with pytest.raises(ValueError, match="lengths"):
        KEO3(one, ks[0], ks[1], ks[2][:4], G)
    with pytest.raises(ValueError, match="lengths"):
        curvilinear_run3(x, y[:8], z, two, V, G, m["dt"], 2)
    with pytest.raises(ValueError, match="nout"):
        curvilinear_run3(x, y, z, one, v, G, m["dt"], 2, nout=0)


def test_spo3_curvilinear_refusals_need_no_device():
    from pyqed_amd.wpd import SPO3
    m = g3.model3(16, 16, 16, ns=2)
    x, y, z, G = m["x"], m["y"], m["z"], m["G"]
    for bad, msg in ((None, "metric G"), (G + 0.01j, "real"), (G[:, :8], "G must be"), (G[..., :2, :2], "G must be"),
                     (G[..., 0, 0], "G must be")):
        sol = SPO3(x, y, z, [1, 1, 1], nstates=2, coords="curvilinear", G=bad)
        sol.V = m["V"]
        with pytest.raises(ValueError, match=msg):
            sol.build(m["dt"])
        with pytest.raises(ValueError, match=msg):
            sol.run(m["psi0"], dt=m["dt"], nt=2)
    for four in (G[..., 0], G[:, :, 0, :2, :2]):   # a four-dimensional G: two curvilinear coordinates and a third
        sol = SPO3(x, y, z, [1, 1, 1], nstates=2, coords="curvilinear", G=four)
        with pytest.raises(NotImplementedError, match="3-D metric"):
            sol.build(m["dt"])
        with pytest.raises(NotImplementedError, match="3-D metric"):
            sol.run(m["psi0"], dt=m["dt"], nt=2)
    sol = SPO3(x, y, z, [1, 1, 1], nstates=2, coords="curvilinear", G=G)
    sol.build(m["dt"])   # forms kx, ky, kz and checks G; no propagators
    assert all(np.array_equal(a, b) for a, b in zip((sol.kx, sol.ky, sol.kz), m["ks"]))
    assert sol.exp_K is None and sol.exp_V is None and sol.exp_V_half is None
    with pytest.raises(ValueError, match="PES is not specified"):
        sol.run(m["psi0"], dt=m["dt"], nt=2)
    sol.V = m["V"]
    with pytest.raises(ValueError, match=r"psi0 must be \[16, 16, 16, 2\]"):
        sol.run(m["psi0"][..., :1], dt=m["dt"], nt=2)
    with pytest.raises(ValueError, match="nout"):
        sol.run(m["psi0"], dt=m["dt"], nt=2, nout=0)
    with pytest.raises(NotImplementedError, match="jacobi"):
        SPO3(x, y, z, [1, 1, 1], coords="jacobi").build(m["dt"])
    with pytest.raises(ValueError, match="unknown coordinates"):
        SPO3(x, y, z, [1, 1, 1], coords="polar", G=G).build(m["dt"])
