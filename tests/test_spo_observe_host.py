"""SPO observables without a GPU: the argument checks of qd_spo_observe / qd_spo2_run_observed / qd_spo3_run_observed
(all before any HIP call, like every entry point: tests/test_abi.py), the ValueError of population() and the
recorded-array branches of ResultSPO2.get_population / position."""
import ctypes
import os

import numpy as np
import pytest

P = ctypes.c_void_p
ONE = 0x1000   # any non-null address: a call that fails its argument checks dereferences nothing


def _lib():
    from pyqed_amd import _lib
    return _lib, _lib.load()


def _dims(*d):
    return (ctypes.c_int * len(d))(*d)


def _observe(lib, psi=ONE, B=1, dims=(4, 4), ndim=2, ns=2, basis=None, x=(ONE, ONE, None), rdm=ONE, mom=None):
    return lib.qd_spo_observe(psi, B, _dims(*dims) if dims is not None else None, ndim, ns, basis, x[0], x[1], x[2], 1.0,
                              rdm, mom, None)


@pytest.mark.parametrize("kw,word", [
    (dict(psi=None), "null"),
    (dict(rdm=None), "null"),
    (dict(dims=None), "null"),
    (dict(ndim=0), "ndim"),
    (dict(ndim=4, dims=(2, 2, 2, 2)), "ndim"),
    (dict(ns=0), "ns"),
    (dict(B=0), "B"),
    (dict(dims=(4, 0)), "dims"),
    (dict(mom=ONE, x=(ONE, None, None)), "axis"),
    (dict(mom=ONE, x=(None, ONE, None)), "axis"),
    (dict(mom=ONE, ndim=3, dims=(2, 2, 2), x=(ONE, ONE, None)), "axis"),
])
def test_observe_rejects_bad_arguments(kw, word):
    _l, lib = _lib()
    assert _observe(lib, **kw) == _l.QD_EINVAL
    msg = _l.last_error()
    assert msg.startswith("qd_spo_observe") and word in msg, msg


def _run2(lib, psi=ONE, B=1, eVh=ONE, eK=ONE, ns=2, nsteps=4, nout=2, x=ONE, y=ONE, rdm=ONE, mom=None):
    return lib.qd_spo2_run_observed(psi, B, eVh, eK, None, 16, 16, ns, nsteps, nout, None, None, x, y, 1.0, rdm, mom, None)


@pytest.mark.parametrize("kw,word", [
    (dict(psi=None), "null"),
    (dict(eVh=None), "null"),
    (dict(eK=None), "null"),
    (dict(rdm=None), "null"),
    (dict(ns=0), "ns"),
    (dict(B=0), "B"),
    (dict(nout=0), "nout"),
    (dict(nsteps=-1), "nsteps"),
    (dict(mom=ONE, y=None), "axis"),
])
def test_spo2_run_observed_rejects_bad_arguments(kw, word):
    _l, lib = _lib()
    assert _run2(lib, **kw) == _l.QD_EINVAL
    msg = _l.last_error()
    assert msg.startswith("qd_spo2_run_observed") and word in msg, msg


def _run3(lib, psi=ONE, eVh=ONE, eK=ONE, m=(None, None, None), ns=2, nout=1, axes=(ONE, ONE, ONE), rdm=ONE, mom=None):
    return lib.qd_spo3_run_observed(psi, eVh, eK, m[0], m[1], m[2], 16, 16, 16, ns, 2, nout, None, None, axes[0],
                                    axes[1], axes[2], 1.0, rdm, mom, None)


@pytest.mark.parametrize("kw,word", [
    (dict(psi=None), "null"),
    (dict(eVh=None), "null"),
    (dict(rdm=None), "null"),
    (dict(eK=None), "exactly one"),                       # neither kinetic form
    (dict(m=(ONE, ONE, ONE)), "exactly one"),             # both
    (dict(eK=None, m=(ONE, None, ONE)), "exactly one"),   # an incomplete set of axis propagators
    (dict(ns=0), "ns"),
    (dict(nout=0), "nout"),
    (dict(mom=ONE, axes=(ONE, ONE, None)), "axis"),
])
def test_spo3_run_observed_rejects_bad_arguments(kw, word):
    _l, lib = _lib()
    assert _run3(lib, **kw) == _l.QD_EINVAL
    msg = _l.last_error()
    assert msg.startswith("qd_spo3_run_observed") and word in msg, msg


def test_population_rejects_other_representations():
    """The reference's ValueError (wpd.py:684-686), raised before anything touches the device."""
    from pyqed_amd import SPO2, SPO3
    x = np.linspace(-1, 1, 8)
    psi = np.zeros((8, 8, 2), complex)
    with pytest.raises(ValueError, match="diabatic or adiabatic"):
        SPO2(x, x, nstates=2).population(psi, representation='natural')
    with pytest.raises(ValueError, match="diabatic or adiabatic"):
        SPO2(x, x, nstates=2).population([psi], 'Adiabatic')
    with pytest.raises(ValueError, match="diabatic or adiabatic"):
        SPO3(x, x, x, masses=[1, 1, 1], nstates=2).population(np.zeros((8, 8, 8, 2), complex), 'natural')


def _result(nstates_list):
    from pyqed_amd.wpd import ResultSPO2
    x, y = np.linspace(-2, 2, 6), np.linspace(-1, 1, 5)
    rng = np.random.default_rng(3)
    states = [rng.standard_normal((6, 5, 2)) + 1j * rng.standard_normal((6, 5, 2)) for _ in range(nstates_list)]
    r = ResultSPO2(dt=0.1, psi0=states[0], Nt=2 * (nstates_list - 1), nout=2)
    r.x, r.y = x, y
    r.psilist = list(states)
    return r, x, y, states


def test_result_helpers_fall_back_to_psilist(tmp_path, monkeypatch):
    """No recorded arrays: today's host reductions of psilist (wpd.py:104-159)."""
    monkeypatch.chdir(tmp_path)
    r, x, y, states = _result(3)
    w = (x[1] - x[0]) * (y[1] - y[0])
    p = r.get_population()
    ref = np.array([[np.sum(np.abs(s[:, :, n]) ** 2) * w for n in range(2)] for s in states])
    assert np.allclose(p, ref, rtol=1e-14, atol=0)
    xa, ya = r.position()
    assert np.allclose(xa, [np.einsum('ijn,i->', np.abs(s) ** 2, x) * w for s in states], rtol=1e-13, atol=1e-15)
    assert os.path.exists(tmp_path / "xAve.npz")


def test_result_helpers_return_recorded_arrays(tmp_path, monkeypatch):
    """run(observe=..., return_states=False) leaves psilist == [psi0] and the recorded arrays; with states present the
    helpers recompute from the states as before, recorded arrays or not."""
    monkeypatch.chdir(tmp_path)
    r, x, y, states = _result(1)
    pop = np.array([[0.75, 0.25], [0.5, 0.5], [0.25, 0.75]])
    xa, ya = np.array([0.1, 0.2, 0.3]), np.array([-1.0, -2.0, -3.0])
    r._recorded = (pop, xa, ya)
    assert r.get_population() is pop and r.population is pop
    r.get_population(fname=str(tmp_path / "pop"))
    assert np.array_equal(np.load(tmp_path / "pop.npz")["arr_0"], pop)
    gx, gy = r.position()
    assert gx is xa and gy is ya and r.xAve[0] is xa and r.xAve[1] is ya
    f = np.load(tmp_path / "xAve.npz")
    assert np.array_equal(f["arr_0"], xa) and np.array_equal(f["arr_1"], ya)
    r2, x, y, states = _result(3)
    r2._recorded = (pop, xa, ya)
    w = (x[1] - x[0]) * (y[1] - y[0])
    ref = np.array([[np.sum(np.abs(s[:, :, n]) ** 2) * w for n in range(2)] for s in states])
    assert np.allclose(r2.get_population(), ref, rtol=1e-14, atol=0)
    assert not np.allclose(r2.position()[0], xa)
