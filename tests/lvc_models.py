"""Helpers of the LVC tests (no test here): a matrix-free numpy restatement of the linear-vibronic-coupling model in
Fock space -- H psi, the Horner RK4 and the observable record of include/qdyn.h (qd_lvc_apply / qd_lvc_rk4 /
qd_lvc_observe) -- with the working precision as a parameter (np.clongdouble or np.complex128), and the dense H of the
same model assembled from explicit np.kron products, against which tests/test_lvc_host.py checks the restatement.

State psi[a, n_1, .., n_M], row-major, electronic index slowest, the last mode fastest; states are rows [B, D].

    (H psi)[a, n] = sum_b Hel[a, b] psi[b, n] + (sum_j omega_j n_j) psi[a, n]
                  + sum_j sum_b W[j][a, b] (sqrt(n_j / 2) psi[b, n - e_j] + sqrt((n_j + 1) / 2) psi[b, n + e_j])
"""
from __future__ import annotations

import numpy as np


def real_of(dtype):
    return np.empty(0, dtype=dtype).real.dtype.type


def size(nel, dims):
    return int(nel * np.prod(dims, dtype=np.int64))


def nobs(nel, dims):
    return nel * nel * (1 + len(dims)) + len(dims)


def random_model(nel, dims, seed=0):
    """omega [M] > 0, Hel [nel, nel] and W [M, nel, nel] dense random complex, not Hermitian."""
    rng = np.random.default_rng([seed, nel, len(dims)] + [int(d) for d in dims])
    c = lambda *sh: rng.standard_normal(sh) + 1j * rng.standard_normal(sh)   # noqa: E731
    return rng.uniform(0.5, 1.5, len(dims)), c(nel, nel), 0.5 * c(len(dims), nel, nel)


def random_states(B, nel, dims, seed=1):
    rng = np.random.default_rng([seed, B, nel] + [int(d) for d in dims])
    D = size(nel, dims)
    psi = rng.standard_normal((B, D)) + 1j * rng.standard_normal((B, D))
    return psi / np.linalg.norm(psi, axis=1, keepdims=True)


def h_bound(dims, omega, Hel, W):
    """An upper bound of ||H||_1 from the model: every column of x_j sums to at most 2 sqrt(N_j / 2)."""
    b = np.abs(Hel).sum(axis=0).max() + sum(w * (N - 1) for w, N in zip(omega, dims))
    return float(b + sum(np.abs(W[j]).sum(axis=0).max() * 2 * np.sqrt(N / 2) for j, N in enumerate(dims)))


def _grid(psi, nel, dims, dtype):
    psi = np.asarray(psi)
    return np.asarray(psi, dtype=dtype).reshape((psi.shape[0], nel) + tuple(int(d) for d in dims))


def x_apply(P, j, dtype):
    """x_j on the grid P [B, nel, *dims]: t[n] = sqrt(n / 2) P[n - 1] + sqrt((n + 1) / 2) P[n + 1] along mode j."""
    real = real_of(dtype)
    ax = 2 + j
    N = P.shape[ax]
    t = np.zeros_like(P)
    if N == 1:
        return t
    shape = [1] * P.ndim
    shape[ax] = N - 1
    c = np.sqrt(np.arange(1, N, dtype=real) / real(2)).reshape(shape)   # c[k] = sqrt((k + 1) / 2) couples k and k + 1
    lo = [slice(None)] * P.ndim
    hi = [slice(None)] * P.ndim
    lo[ax], hi[ax] = slice(0, N - 1), slice(1, N)
    lo, hi = tuple(lo), tuple(hi)
    t[hi] += c * P[lo]
    t[lo] += c * P[hi]
    return t


def _levels(P, j, dtype):
    shape = [1] * P.ndim
    shape[2 + j] = P.shape[2 + j]
    return np.arange(P.shape[2 + j], dtype=real_of(dtype)).reshape(shape)


def apply(psi, nel, dims, omega, Hel, W, dtype=np.complex128):
    """H psi for the rows of psi [B, D], in `dtype`."""
    real = real_of(dtype)
    P = _grid(psi, nel, dims, dtype)
    Hel = np.asarray(Hel, dtype=dtype)
    W = np.asarray(W, dtype=dtype)
    out = np.einsum("ab,Bb...->Ba...", Hel, P)
    for j in range(len(dims)):
        out = out + real(omega[j]) * _levels(P, j, dtype) * P
        out = out + np.einsum("ab,Bb...->Ba...", W[j], x_apply(P, j, dtype))
    return out.reshape(P.shape[0], -1)


def rk4(psi0, nel, dims, omega, Hel, W, dt, nsteps, save_every=0, dtype=np.complex128):
    """qd_lvc_rk4 restated: Horner-form RK4 psi' = psi + dt L (psi + dt/2 L (psi + dt/3 L (psi + dt/4 L psi))),
    L = -iH.  Returns (psi [B, D], snap [B, nsave, D] | None, obs [B, nsave + 1, nobs]) rounded to complex128 once."""
    real = real_of(dtype)
    psi = np.asarray(psi0, dtype=dtype)
    coef = [real(dt) / real(4), real(dt) / real(3), real(dt) / real(2), real(dt)]
    saves, recs = [], [record(psi, nel, dims, dtype)]
    for s in range(nsteps):
        v = psi
        for c in coef:
            v = psi + c * (dtype(-1j) * apply(v, nel, dims, omega, Hel, W, dtype))
        psi = v
        if save_every > 0 and (s + 1) % save_every == 0:
            saves.append(psi.copy())
            recs.append(record(psi, nel, dims, dtype))
    snap = np.stack(saves, axis=1).astype(np.complex128) if saves else None
    return psi.astype(np.complex128), snap, np.stack(recs, axis=1).astype(np.complex128)


def record(psi, nel, dims, dtype=np.complex128):
    """[B, nobs] in `dtype`: rho [nel, nel], X[j] [nel, nel] for every mode, nbar [M]."""
    P = _grid(psi, nel, dims, dtype)
    B = P.shape[0]
    flat = P.reshape(B, nel, -1)
    parts = [np.einsum("Ban,Bbn->Bab", flat, np.conj(flat)).reshape(B, -1)]
    for j in range(len(dims)):
        parts.append(np.einsum("Ban,Bbn->Bab", x_apply(P, j, dtype).reshape(B, nel, -1), np.conj(flat)).reshape(B, -1))
    nbar = [(_levels(P, j, dtype) * (P.real ** 2 + P.imag ** 2)).reshape(B, -1).sum(axis=1) for j in range(len(dims))]
    parts.append(np.stack(nbar, axis=1).astype(dtype))
    return np.concatenate(parts, axis=1)


def split_record(rec, nel, M):
    """(rho [.., nel, nel], X [.., M, nel, nel], nbar [.., M]) of records [.., nobs]."""
    rec = np.asarray(rec)
    nn = nel * nel
    lead = rec.shape[:-1]
    return (rec[..., :nn].reshape(lead + (nel, nel)), rec[..., nn:nn * (1 + M)].reshape(lead + (M, nel, nel)),
            rec[..., nn * (1 + M):])


def x_matrix(N):
    x = np.zeros((N, N))
    for n in range(N - 1):
        x[n, n + 1] = x[n + 1, n] = np.sqrt((n + 1) / 2)
    return x


def _kron(*ms):
    out = np.eye(1)
    for m in ms:
        out = np.kron(out, m)
    return out


def dense_h(nel, dims, omega, Hel, W):
    """The dense H [D, D] from explicit Kronecker products, kron(el, mode_1, .., mode_M) order."""
    eyes = [np.eye(int(N)) for N in dims]
    H = _kron(np.asarray(Hel, dtype=complex), *eyes)
    for j, N in enumerate(dims):
        num = eyes[:j] + [np.diag(omega[j] * np.arange(N))] + eyes[j + 1:]
        xj = eyes[:j] + [x_matrix(int(N))] + eyes[j + 1:]
        H = H + _kron(np.eye(nel), *num) + _kron(np.asarray(W[j], dtype=complex), *xj)
    return H
