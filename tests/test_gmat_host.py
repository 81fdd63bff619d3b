"""Curvilinear (G-matrix) wavepacket propagation without a GPU: the numpy restatement of tests/gmat_models.py against
the reference's own outputs (tests/golden/gmat2d.npz), the argument checks of the two C-ABI entry points and the
refusals of pyqed_amd.wpd.adiabatic_2d, all of which happen before any device call."""
import numpy as np
import pytest
from scipy.fftpack import fftfreq

from conftest import load_golden, relerr
import gmat_models as gm


def _case(g, tag):
    c = {k[len(tag) + 1:]: v for k, v in g.items() if k.startswith(tag + "_")}
    nx, ny = c["psi0"].shape
    c["kx"] = 2.0 * np.pi * fftfreq(nx, c["x"][1] - c["x"][0])
    c["ky"] = 2.0 * np.pi * fftfreq(ny, c["y"][1] - c["y"][0])
    return c


@pytest.mark.parametrize("tag", ["a", "b", "c"])
def test_restatement_reproduces_the_reference(tag):
    """Two fp64 orderings of the same arithmetic measured <= 6e-16; 1e-14 leaves room for another numpy build."""
    c = _case(load_golden("gmat2d"), tag)
    run = gm.run_ref(c["psi0"], float(c["dt"]), int(c["nt"]), c["kx"], c["ky"], c["v"], c["G"])
    assert relerr(run[-1], c["psi"]) <= 1e-14
    if "noise" in c:
        assert relerr(gm.hpsi_ref(c["noise"], c["kx"], c["ky"], c["v"], c["G"]), c["hpsi"]) <= 1e-14
        assert relerr(gm.keo_ref(c["noise"], c["kx"], c["ky"], c["G"]), c["keo"]) <= 1e-14


def test_fixture_matches_the_model():
    """The stored inputs are the model's (a fixture cannot drift from gmat_models.model unnoticed), up to the last
    bits of another numpy build's exp / cos."""
    g = load_golden("gmat2d")
    for tag, absorb in (("a", 0.0), ("b", 0.0), ("c", 0.1)):
        c = _case(g, tag)
        m = gm.model(*c["psi0"].shape)
        for got, want in ((c["G"], m["G"]), (c["psi0"], m["psi0"]), (c["v"], m["v"] - 1j * absorb), (c["dt"], m["dt"])):
            assert np.allclose(got, want, rtol=1e-13, atol=1e-15)


# a valid argument list for each entry point (pointers are never dereferenced: validation comes first)
P = 0x1000
APPLY_OK = dict(psi=P, B=1, G=P, v=None, kx=P, ky=P, nx=16, ny=16, out=2 * P, stream=None)
RK4_OK = dict(psi=P, B=1, G=P, v=None, kx=P, ky=P, nx=16, ny=16, dt=0.1, nsteps=1, nout=1, snap=None, stream=None)
BAD_COMMON = [dict(psi=None), dict(G=None), dict(kx=None), dict(ky=None), dict(B=0), dict(nx=0), dict(ny=0),
              dict(B=-3), dict(B=8, nx=16384, ny=16384), dict(B=2, nx=32768, ny=32768)]


@pytest.mark.parametrize("bad", BAD_COMMON + [dict(out=None)], ids=str)
def test_apply_rejects_invalid_arguments(bad):
    from pyqed_amd import _lib
    lib = _lib.load()
    assert hasattr(lib, "qd_wp2_gmat_apply")
    rc = lib.qd_wp2_gmat_apply(*{**APPLY_OK, **bad}.values())
    assert rc == _lib.QD_EINVAL
    assert "qd_wp2_gmat_apply" in _lib.last_error()


@pytest.mark.parametrize("bad", BAD_COMMON + [dict(nout=0), dict(nsteps=-1)], ids=str)
def test_rk4_rejects_invalid_arguments(bad):
    from pyqed_amd import _lib
    lib = _lib.load()
    assert hasattr(lib, "qd_wp2_gmat_rk4")
    rc = lib.qd_wp2_gmat_rk4(*{**RK4_OK, **bad}.values())
    assert rc == _lib.QD_EINVAL
    assert "qd_wp2_gmat_rk4" in _lib.last_error()


def test_rk4_zero_steps_is_a_no_op_without_a_device():
    from pyqed_amd import _lib
    assert _lib.load().qd_wp2_gmat_rk4(*{**RK4_OK, "nsteps": 0}.values()) == _lib.QD_OK


def test_adiabatic_2d_refusals_need_no_device():
    from pyqed_amd.wpd import adiabatic_2d
    m = gm.model(16, 16)
    args = (m["x"], m["y"], m["psi0"], m["v"], m["dt"])
    with pytest.raises(NotImplementedError, match=r"SPO2\(.*nstates=1\)"):
        adiabatic_2d(*args, Nt=1, coords="linear", G=m["G"])
    with pytest.raises(NotImplementedError, match="x_evolve_2d"):
        adiabatic_2d(*args)   # the reference's default coords
    with pytest.raises(ValueError, match="coords"):
        adiabatic_2d(*args, Nt=1, coords="polar", G=m["G"])
    with pytest.raises(ValueError, match="real"):
        adiabatic_2d(*args, Nt=1, coords="curvilinear", G=m["G"] + 0.01j)
    with pytest.raises(ValueError, match="G must be"):
        adiabatic_2d(*args, Nt=1, coords="curvilinear", G=m["G"][:, :8])
    with pytest.raises(ValueError, match="G must be"):
        adiabatic_2d(*args, Nt=1, coords="curvilinear", G=m["G"][..., 0])
    with pytest.raises(ValueError, match="v must be"):
        adiabatic_2d(m["x"], m["y"], m["psi0"], m["v"][:8], m["dt"], Nt=1, coords="curvilinear", G=m["G"])
    with pytest.raises(ValueError, match="lengths"):
        adiabatic_2d(m["x"][:8], m["y"], m["psi0"], m["v"], m["dt"], Nt=1, coords="curvilinear", G=m["G"])
    with pytest.raises(ValueError, match="metric G"):
        adiabatic_2d(*args, Nt=1, coords="curvilinear")


def test_operator_refusals_need_no_device():
    from pyqed_amd.wpd import KEO, hpsi
    m = gm.model(16, 16)
    with pytest.raises(ValueError, match="real"):
        KEO(m["psi0"], m["kx"], m["ky"], m["G"] * (1 + 0.5j))
    with pytest.raises(ValueError, match="lengths"):
        hpsi(m["psi0"], m["kx"][:4], m["ky"], m["v"], m["G"])
    with pytest.raises(ValueError, match="psi must be"):
        KEO(m["psi0"][0], m["kx"], m["ky"], m["G"])
