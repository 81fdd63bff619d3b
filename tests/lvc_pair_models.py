"""Helpers of the LVC pair tests (no test here), on tests/lvc_models.py: the pair record of include/qdyn.h
(qd_lvc_pair_observe), the pair run (qd_lvc_pair_rk4) as two propagations of lm.rk4's form, and the four correlation
functions of SESolver restated on them, with the working precision as a parameter; the operators as Kronecker products
and the dense-H RK4 the host tests check the restatements against; the inputs and shapes of the GPU kernel tests.

A pair is [2, D] (ket, bra); pairs are [P, 2, D].  Block r of a record: R_r[a, b] = sum_n L_r[a, n] conj(bra[b, n]),
L_0 = ket, L_{j+1} = x_j ket, so <bra| A (x) 1 |ket> = tr(A R_0) and <bra| A (x) x_j |ket> = tr(A R_{j+1}).
"""
from __future__ import annotations

import numpy as np

import lvc_models as lm

NSTEPS, SE = 5, 2


def pair_record(pairs, nel, dims, blocks, dtype=np.complex128):
    """[P, nblk, nel, nel] in `dtype`."""
    pairs = np.asarray(pairs)
    ket = lm._grid(pairs[:, 0], nel, dims, dtype)
    bra = lm._grid(pairs[:, 1], nel, dims, dtype)
    P = ket.shape[0]
    cb = np.conj(bra.reshape(P, nel, -1))
    out = []
    for r in blocks:
        L = ket if r == 0 else lm.x_apply(ket, r - 1, dtype)
        out.append(np.einsum("Pan,Pbn->Pab", L.reshape(P, nel, -1), cb))
    return np.stack(out, axis=1)


def step(psi, nel, dims, omega, Hel, W, dt, dtype):
    """One Horner RK4 step of the rows of psi, lm.rk4's arithmetic."""
    real = lm.real_of(dtype)
    v = psi
    for c in (real(dt) / real(4), real(dt) / real(3), real(dt) / real(2), real(dt)):
        v = psi + c * (dtype(-1j) * lm.apply(v, nel, dims, omega, Hel, W, dtype))
    return v


def pair_rk4(pairs, nel, dims, omega, Hel, W, dt, nsteps, save_every, blocks, dtype=np.complex128):
    """qd_lvc_pair_rk4 restated: both states of every pair by the Horner RK4, a record at t0 and after every save_every
    steps.  Returns (pairs [P, 2, D], rec [P, nsave + 1, nblk, nel, nel]) rounded to complex128 once."""
    pairs = np.asarray(pairs)
    P = pairs.shape[0]
    psi = np.asarray(pairs.reshape(2 * P, -1), dtype=dtype)
    recs = [pair_record(psi.reshape(P, 2, -1), nel, dims, blocks, dtype)]
    for s in range(nsteps):
        psi = step(psi, nel, dims, omega, Hel, W, dt, dtype)
        if (s + 1) % save_every == 0:
            recs.append(pair_record(psi.reshape(P, 2, -1), nel, dims, blocks, dtype))
    return psi.reshape(P, 2, -1).astype(np.complex128), np.stack(recs, axis=1).astype(np.complex128)


# ---------------------------------------------------------------- operators held as factors: (A [nel, nel], block)
def factor_apply(fac, psi, nel, dims, dtype=np.complex128):
    """(A (x) 1) psi (block 0) or (A (x) x_j) psi (block j + 1) for the rows of psi."""
    A, r = fac
    P = lm._grid(psi, nel, dims, dtype)
    if r:
        P = lm.x_apply(P, r - 1, dtype)
    return np.einsum("ab,Bb...->Ba...", np.asarray(A, dtype=dtype), P).reshape(P.shape[0], -1)


def factor_dense(fac, nel, dims):
    A, r = fac
    return lm._kron(np.asarray(A, dtype=complex), *[lm.x_matrix(int(N)) if j == r - 1 else np.eye(int(N))
                                                    for j, N in enumerate(dims)])


def factor_product(b, c):
    if b[1] and c[1]:
        raise NotImplementedError("two coordinate factors")
    return np.asarray(b[0]) @ np.asarray(c[0]), b[1] or c[1]


def corr_3op(psi_t, facs, nel, dims, omega, Hel, W, dt, ntau, dtype=np.complex128):
    """corr [B, ntau] for the rows of psi_t and [a, b, c] = facs: ket = c psi, bra = a^+ psi, corr[j] = tr(A_b R_b(j))."""
    a, b, c = facs
    ket = factor_apply(c, psi_t, nel, dims, dtype)
    bra = factor_apply((np.conj(np.asarray(a[0])).T, a[1]), psi_t, nel, dims, dtype)
    pairs = np.stack([ket, bra], axis=1)
    P = pairs.shape[0]
    psi = pairs.reshape(2 * P, -1)
    out = []
    for j in range(ntau):
        if j:
            psi = step(psi, nel, dims, omega, Hel, W, dt, dtype)
        R = pair_record(psi.reshape(P, 2, -1), nel, dims, [b[1]], dtype)[:, 0]
        out.append(np.einsum("ab,Pba->P", np.asarray(b[0], dtype=dtype), R))
    return np.stack(out, axis=1).astype(np.complex128)


def states_t(psi0, nel, dims, omega, Hel, W, dt, Nt, dtype=np.complex128):
    """psi(t_i), i = 0 .. Nt - 1, as rows."""
    psi = np.asarray(psi0, dtype=dtype).reshape(1, -1)
    rows = [psi]
    for _ in range(Nt - 1):
        psi = step(psi, nel, dims, omega, Hel, W, dt, dtype)
        rows.append(psi)
    return np.concatenate(rows, axis=0)


def correlation_3op_1t(psi0, facs, nel, dims, omega, Hel, W, dt, Nt, dtype=np.complex128):
    return corr_3op(np.asarray(psi0).reshape(1, -1), facs, nel, dims, omega, Hel, W, dt, Nt, dtype)[0]


def correlation_3op_2t(psi0, facs, nel, dims, omega, Hel, W, dt, Nt, Ntau, dtype=np.complex128):
    return corr_3op(states_t(psi0, nel, dims, omega, Hel, W, dt, Nt, dtype), facs, nel, dims, omega, Hel, W, dt, Ntau,
                    dtype)


def correlation_4op_1t(psi0, facs, nel, dims, omega, Hel, W, dt, Nt, dtype=np.complex128):
    a, b, c, d = facs
    return correlation_3op_1t(psi0, [a, factor_product(b, c), d], nel, dims, omega, Hel, W, dt, Nt, dtype)


def correlation_4op_2t(psi0, facs, nel, dims, omega, Hel, W, dt, Nt, Ntau, dtype=np.complex128):
    a, b, c, d = facs
    return correlation_3op_2t(psi0, [a, factor_product(b, c), d], nel, dims, omega, Hel, W, dt, Nt, Ntau, dtype)


# ---------------------------------------------------------------- the dense side
def dense_step(H, psi, dt):
    v = psi
    for c in (dt / 4, dt / 3, dt / 2, dt):
        v = psi + c * (-1j * (H @ v))
    return v


def dense_corr_3op(H, psi_t, ops, dt, ntau):
    """corr [B, ntau] of the rows of psi_t for dense [a, b, c]: the reference's rule with the Horner RK4."""
    a, b, c = ops
    out = np.zeros((len(psi_t), ntau), dtype=complex)
    for i, psi in enumerate(psi_t):
        ket, bra = c @ psi, a.conj().T @ psi
        for j in range(ntau):
            if j:
                ket, bra = dense_step(H, ket, dt), dense_step(H, bra, dt)
            out[i, j] = np.vdot(bra, b @ ket)
    return out


def dense_states_t(H, psi0, dt, Nt):
    rows = [np.asarray(psi0, dtype=complex)]
    for _ in range(Nt - 1):
        rows.append(dense_step(H, rows[-1], dt))
    return np.array(rows)


# ---------------------------------------------------------------- inputs of the GPU kernel tests
def random_pairs(P, nel, dims, seed=2):
    """ket random and normalised, bra = normalise(ket + 0.5 noise) with noise a second random normalised state: no block
    is a near-cancellation."""
    rng = np.random.default_rng([seed, P, nel] + [int(d) for d in dims])
    D = lm.size(nel, dims)

    def unit():
        v = rng.standard_normal((P, D)) + 1j * rng.standard_normal((P, D))
        return v / np.linalg.norm(v, axis=1, keepdims=True)

    ket = unit()
    bra = ket + 0.5 * unit()
    bra /= np.linalg.norm(bra, axis=1, keepdims=True)
    return np.ascontiguousarray(np.stack([ket, bra], axis=1))


FIXED = [(1, (1,)), (2, (2, 2)), (3, (3, 5, 7)), (4, (3, 5)), (5, (4, 3)), (8, (4, 3)), (3, (5, 67)), (3, (65, 3)),
         (2, (1, 9, 1)), (3, (2, 2, 2, 2, 2, 2))]


def gpu_cases(tile, limit):
    """(nel, dims) of tests/test_lvc_pair_kernels_gpu.py: FIXED, one below, at and one above the tile extent, the
    neighbours of the one-mode pair resident limit at nel = 1, 3 and 8, and those of every other mode count's limit at
    nel = 3.  limit(M) is the plan's."""
    out = list(FIXED)
    out += [(3, (tile - 1,)), (3, (tile,)), (3, (tile + 1,))]
    L = limit(1)
    out += [(1, (L,)), (1, (L + 1,)), (3, (L // 3,)), (3, (L // 3 + 1,)), (8, (L // 8,)), (8, (L // 8 + 1,))]
    for M in range(2, 7):
        if (M == 2 or limit(M) != limit(M - 1)) and limit(M) >= 6:
            out += [(3, (1,) * (M - 2) + (2, limit(M) // 6)), (3, (1,) * (M - 2) + (2, limit(M) // 6 + 1))]
    return out


def gpu_inputs(nel, dims, P):
    omega, Hel, W = lm.random_model(nel, dims)
    pairs = random_pairs(P, nel, dims)
    dt = 0.5 / lm.h_bound(dims, omega, Hel, W)
    return omega, Hel, W, pairs, dt
