"""Argument validation of qd_tdse_pair_corr and of the SESolver correlation functions (no GPU: every check
precedes any HIP call / device work)."""
import ctypes

import numpy as np
import pytest


def _call(lib, H, A, Bop, C, psi, B, N, ntau, corr):
    return lib.qd_tdse_pair_corr(H, A, Bop, C, psi, B, N, 0.01, ntau, corr, None)


def test_pair_corr_rejects_bad_arguments():
    from pyqed_amd import _lib
    lib = _lib.load()
    N, B, ntau = 4, 2, 3
    mat = (ctypes.c_double * (2 * N * N))()
    vec = (ctypes.c_double * (2 * B * N))()
    out = (ctypes.c_double * (2 * B * ntau))()
    m, v, o = (ctypes.cast(x, ctypes.c_void_p) for x in (mat, vec, out))
    good = [m, m, m, m, v, B, N, ntau, o]
    for k in (0, 1, 2, 3, 4, 8):          # every pointer in turn
        args = list(good)
        args[k] = None
        assert _call(lib, *args) == _lib.QD_EINVAL
        assert "qd_tdse_pair_corr" in _lib.last_error() and "null" in _lib.last_error()
    for k, bad in ((5, 0), (5, -1), (6, 0), (7, 0), (7, -2)):   # B, N, ntau
        args = list(good)
        args[k] = bad
        assert _call(lib, *args) == _lib.QD_EINVAL
        assert "qd_tdse_pair_corr" in _lib.last_error() and "bad sizes" in _lib.last_error()


def test_sesolver_correlations_reject_bad_arguments(monkeypatch):
    """Wrong-length oplist and Nt / Ntau < 1 raise ValueError before any device is asked for."""
    from pyqed_amd import _util
    from pyqed_amd.mol import SESolver

    def no_device():
        raise AssertionError("device work before the argument checks")

    monkeypatch.setattr(_util, "default_device", no_device)
    N = 3
    sol = SESolver(np.eye(N, dtype=complex))
    psi0 = np.ones(N, complex) / np.sqrt(N)
    ops = [np.eye(N, dtype=complex)] * 4
    with pytest.raises(ValueError):
        sol.correlation_3op_1t(psi0, ops[:2], 0.01, 4)
    with pytest.raises(ValueError):
        sol.correlation_3op_1t(psi0, ops[:3], 0.01, 0)
    with pytest.raises(ValueError):
        sol.correlation_3op_2t(psi0, ops, 0.01, 4, 4)
    with pytest.raises(ValueError):
        sol.correlation_3op_2t(psi0, ops[:3], 0.01, 0, 4)
    with pytest.raises(ValueError):
        sol.correlation_3op_2t(psi0, ops[:3], 0.01, 4, 0)
    with pytest.raises(ValueError):
        sol.correlation_4op_1t(psi0, ops[:3], 0.01, 4)
    with pytest.raises(ValueError):
        sol.correlation_4op_1t(psi0, ops, 0.01, 0)
    with pytest.raises(ValueError):
        sol.correlation_4op_2t(psi0, ops[:3], 0.01, 4, 4)
    with pytest.raises(ValueError):
        sol.correlation_4op_2t(psi0, ops, 0.01, 4, 0)


def test_sesolver_has_no_correlation_2op_1t():
    """The reference's SESolver.correlation_2op_1t is a bare `pass` (mol.py:1472-1473); nothing stands in for it."""
    from pyqed_amd.mol import SESolver
    assert not hasattr(SESolver, "correlation_2op_1t")
    for name in ("propagator", "correlation_3op_1t", "correlation_3op_2t", "correlation_4op_1t",
                 "correlation_4op_2t"):
        assert callable(getattr(SESolver, name))
