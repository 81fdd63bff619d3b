"""Host restatement of the Arnoldi and shifted-Hessenberg kernels of pyqed_amd/csrc/krylov.hip, in plain numpy with
the working precision as a parameter: `dtype` is np.complex128 or np.clongdouble (80-bit extended where the host has
it, eps 1.08e-19).  No torch, no library call: these functions are the reference the kernels are judged by
(tests/test_krylov_kernels_gpu.py) after earning that role on the host (tests/test_krylov_oracle_cpu.py).

Written from the formulas of the comment block above dcgs_project_kernel:

    s = V_j^H u_j, t = V_j^H z, alpha = |u_j|^2, gamma = u_j^H z,
    rho = sqrt(alpha - |s|^2), v_j = (u_j - V_j s) / rho, column j-1 += s, h_{j,j-1} = rho,
    a_r = (t_r - (H_j s)_r) / rho (r < j), a_j = ((gamma - s^H t) / rho - rho s_{j-1}) / rho,
    u_{j+1} = z / rho - V_j c - v_j d,  c = H_j s / rho + a_{<j},  d = s_{j-1} + a_j.
"""
from __future__ import annotations

import numpy as np

# np.clongdouble is the x87 80-bit format on the hosts this suite runs on; where it is only a second name for fp64 the
# matrix-vector products below are summed with mpmath instead (the results are then rounded to fp64 once each)
EXTENDED_OK = bool(np.finfo(np.longdouble).eps < 1e-18)


def _real(dtype):
    return np.empty(0, dtype=dtype).real.dtype


def _matvec_mp(A, x):
    """A @ x with every dot product summed exactly by mpmath and rounded once (the fallback of _matvec)."""
    import mpmath
    A = np.asarray(A)
    x = [mpmath.mpc(complex(c)) for c in np.asarray(x)]
    out = np.empty(A.shape[0], dtype=np.result_type(A.dtype, np.complex128))
    with mpmath.workprec(200):
        for r in range(A.shape[0]):
            out[r] = complex(mpmath.fdot([mpmath.mpc(complex(a)) for a in A[r]], x))
    return out


def _matvec(A, x, dtype):
    if np.dtype(dtype) == np.dtype(np.clongdouble) and not EXTENDED_OK:
        return _matvec_mp(A, x).astype(dtype)
    return A @ x


def project(V, w, dtype=np.clongdouble):
    """h_r = V_r^H w for the rows of V [m, n]."""
    V = np.asarray(V, dtype=dtype)
    w = np.asarray(w, dtype=dtype)
    return _matvec(V.conj(), w, dtype)


def normalize(w, dtype=np.clongdouble):
    """(||w||, w / max(||w||, 1e-300))."""
    w = np.asarray(w, dtype=dtype)
    nrm = np.sqrt(_matvec(w.conj()[None, :], w, dtype)[0].real)
    return nrm, w / max(nrm, _real(dtype).type(1e-300))


def dcgs2_step(V, j, z, H, dtype=np.clongdouble):
    """One delayed-CGS2 Arnoldi step (qd_arnoldi_dcgs2_step).  Entering: V[0..j-1] the final basis rows, V[j] = u_j the
    once-projected candidate, z = P u_j, H's columns 0..j-2 final and column j-1 holding the first-pass coefficients.
    Returns (V', H', info): V'[j] = v_j, V'[j+1] = u_{j+1}, H'[:j, j-1] += s, H'[j, j-1] = rho, H'[:j+1, j] the
    first-pass column j; info holds s, t, alpha, gamma, rho.  rho == 0 (exact breakdown) zeroes v_j, u_{j+1} and
    column j.  V [>= j+2, n] and H [>= j+1, >= j+1] are not modified."""
    real = _real(dtype).type
    Vn = np.array(V, dtype=dtype)
    Hn = np.array(H, dtype=dtype)
    z = np.asarray(z, dtype=dtype)
    Vj = Vn[:j]
    u = Vn[j]
    Vc = np.conj(Vn[:j + 1])
    su = _matvec(Vc, u, dtype)
    tz = _matvec(Vc, z, dtype)
    s, t = su[:j], tz[:j]
    alpha, gamma = su[j].real, tz[j]
    rho2 = alpha - np.sum(s.real * s.real + s.imag * s.imag)
    rho = np.sqrt(rho2) if rho2 > 0 else real(0)
    zero = not rho > real(1e-300)
    inv = real(0) if zero else real(1) / rho
    sl = s[j - 1] if j > 0 else np.zeros((), dtype=dtype)[()]
    if j > 0:
        Hn[:j, j - 1] += s
        # (H_j s)_r over the final columns, summed from column max(r - 1, 0) as the kernel does
        Hs = _matvec(np.triu(Hn[:j, :j], -1), s, dtype)
        Hn[j, j - 1] = rho
    else:
        Hs = np.zeros(0, dtype=dtype)
    if zero:
        a = np.zeros(j, dtype=dtype)
        aj = np.zeros((), dtype=dtype)[()]
        c = np.zeros(j, dtype=dtype)
        d = aj
    else:
        a = (t - Hs) * inv
        sht = np.sum(np.conj(s) * t)
        aj = ((gamma - sht) * inv - rho * sl) * inv
        c = Hs * inv + a
        d = sl + aj
    Hn[:j, j] = a
    Hn[j, j] = aj
    VT = Vj.T
    v = (u - _matvec(VT, s, dtype)) * inv
    Vn[j] = v
    Vn[j + 1] = z * inv - _matvec(VT, c, dtype) - v * d
    return Vn, Hn, {"s": s, "t": t, "alpha": alpha, "gamma": gamma, "rho": rho}


def hess_residual(H, k, beta, shift, y):
    """||(-H_k - s I) y - beta e_1|| / (||-H_k - s I||_F ||y|| + beta) in extended precision: the normwise backward
    error of y as a solution of the shifted system, whatever algorithm produced it."""
    dtype = np.clongdouble
    y = np.asarray(y, dtype=dtype)
    shift = dtype(shift)
    r2 = np.longdouble(0)
    a2 = np.longdouble(0)
    for r0 in range(0, k, 512):   # row blocks: k = 4096 in extended precision is half a gigabyte at once
        r1 = min(k, r0 + 512)
        A = -np.asarray(H[r0:r1, :k], dtype=dtype)
        A[np.arange(r1 - r0), np.arange(r0, r1)] -= shift
        res = _matvec(A, y, dtype)
        if r0 == 0:
            res[0] -= np.longdouble(beta)
        r2 += np.sum(res.real ** 2 + res.imag ** 2)
        a2 += np.sum(A.real ** 2 + A.imag ** 2)
    ny = np.sqrt(np.sum(y.real ** 2 + y.imag ** 2))
    return np.sqrt(r2) / (np.sqrt(a2) * ny + np.longdouble(beta))
