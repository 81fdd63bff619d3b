"""numpy restatements of the LDR step with a row-dependent kinetic factor along the last axis
(pyqed/ldr/ldr.py:1938-1987 LDR2_Jacobi.run) for the Jacobi tests, in two forms:

  jacobi_rows        the reference's form: one dense matrix per row of the grid along the last axis, applied row by
                     row with the source row's matrix (exp_T[ija, klb] = A[ija, klb] expKx[i, k] expKy[k, j, l]), then
                     the plain axes, around expand / project; complex128
  jacobi_factorised  F along the last axis, times ph, the plain axes, Fb along the last axis: what qd_ldr_jacobi_run
                     computes, in any dtype (np.clongdouble as the extended-precision oracle when EXTENDED_OK)

The step structure is ldr_models': psi * expVh, then nt // nout blocks of nout x (kinetic, * expV), one snapshot per
block.
"""
import numpy as np

from ldr_models import EXTENDED_OK, member_errors  # noqa: F401


def _plain_axes(chi, Ks):
    for d, K in enumerate(Ks):
        chi = np.moveaxis(np.tensordot(K, chi, axes=(1, d + 1)), 0, d + 1)
    return chi


def _stack(out, psi, nt, nout, dtype):
    shape = (psi.shape[0], nt // nout) + psi.shape[1:]
    return np.stack(out, axis=1) if out else np.zeros(shape, dtype=dtype)


def jacobi_rows(psi0s, U, expV, expVh, rows, expK, nt, nout):
    """Snapshots [B, nt // nout, *n, ns] of psi0s [B, *n, ns]; rows [*n[:-1], n_last, n_last] the last-axis matrix of
    every row of the grid, expK the matrices of the axes before the last."""
    psi = np.asarray(psi0s, dtype=complex) * expVh
    out = []
    for _ in range(nt // nout):
        for _ in range(nout):
            chi = np.einsum('...mb,z...b->z...m', U, psi)
            chi = np.einsum('...jl,z...lm->z...jm', rows, chi)     # row by row, the source row's matrix
            chi = _plain_axes(chi, expK)
            psi = expV * np.einsum('...ma,z...m->z...a', U.conj(), chi)
        out.append(psi.copy())
    return _stack(out, psi, nt, nout, complex)


def jacobi_factorised(psi0s, U, expV, expVh, F, Fb, ph, expK, nt, nout, dtype=np.complex128):
    """Snapshots [B, nt // nout, *n, ns]; F, Fb [n_last, n_last] real, ph [*n], every operation in `dtype`."""
    real = np.zeros(0, dtype=dtype).real.dtype
    psi = np.asarray(psi0s, dtype=dtype)
    U, expV, expVh, ph = (np.asarray(a, dtype=dtype) for a in (U, expV, expVh, ph))
    F, Fb = np.asarray(F, dtype=real), np.asarray(Fb, dtype=real)
    Ks = [np.asarray(K, dtype=dtype) for K in expK]
    psi = psi * expVh
    out = []
    for _ in range(nt // nout):
        for _ in range(nout):
            chi = np.einsum('...mb,z...b->z...m', U, psi)
            chi = np.einsum('jl,z...lm->z...jm', F, chi) * ph[..., None]
            chi = _plain_axes(chi, Ks)
            chi = np.einsum('jl,z...lm->z...jm', Fb, chi)
            psi = expV * np.einsum('...ma,z...m->z...a', U.conj(), chi)
        out.append(psi.copy())
    return _stack(out, psi, nt, nout, dtype)


def rows_of(F, Fb, ph):
    """The per-row matrices Fb diag(ph[row]) F the factorised form stands for, [*n[:-1], n_last, n_last]."""
    return np.einsum('jm,...m,ml->...jl', Fb, ph, F)


def random_case(seed, dims, M, ns, B, dt=0.05):
    """White noise everywhere the kernels read, scaled as ldr_models.random_case scales it: orthonormal complex states,
    surfaces in [0, 2), general complex plain-axis matrices of norm about one, B complex states of unit norm; a general
    real F and an independent general real Fb of norm about one (neither symmetric nor orthogonal nor inverse to each
    other, so a transposition or a swap shows), and a general complex ph of the grid's shape with moduli in [0.5, 1.5]
    (so a conjugate, a wrong row or a dropped member offset shows)."""
    rng = np.random.default_rng(seed)
    dims = tuple(dims)
    npts, n = int(np.prod(dims)), dims[-1]
    g = rng.standard_normal((npts, M, M)) + 1j * rng.standard_normal((npts, M, M))
    q, _ = np.linalg.qr(g)
    U = np.ascontiguousarray(q[:, :, :ns]).reshape(dims + (M, ns))
    apes = 2.0 * rng.random(dims + (ns,))
    expK = [(rng.standard_normal((m, m)) + 1j * rng.standard_normal((m, m))) / np.sqrt(2.0 * m) for m in dims[:-1]]
    F = rng.standard_normal((n, n)) / np.sqrt(n)
    Fb = rng.standard_normal((n, n)) / np.sqrt(n)
    ph = (0.5 + rng.random(dims)) * np.exp(2j * np.pi * rng.random(dims))
    psi = rng.standard_normal((B,) + dims + (ns,)) + 1j * rng.standard_normal((B,) + dims + (ns,))
    psi /= np.linalg.norm(psi.reshape(B, -1), axis=1).reshape((B,) + (1,) * (len(dims) + 1))
    return dict(dims=dims, M=M, ns=ns, U=U, apes=apes, expK=expK, F=F, Fb=Fb, ph=ph, psi=psi, dt=dt,
                expV=np.exp(-1j * dt * apes), expVh=np.exp(-1j * 0.5 * dt * apes))
