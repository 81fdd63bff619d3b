"""numpy restatements of the local-diabatic-representation step (pyqed/ldr/ldr.py:1564-1611 LDR2.run, 579-625
LDRN.run) for the LDR tests, in two forms:

  ldr_dense       the reference's arithmetic: A = U^+ U and exp_T = A * prod_d expK_d materialised as (npts ns)^2
                  arrays and applied per step, complex128
  ldr_factorised  expand with U, one mode product per axis, project with U^+: what qd_ldr_run computes, in any dtype
                  (complex128, or np.clongdouble as the extended-precision oracle; oracle/highprec.py says whether the
                  platform's long double is wider than a double and measures the member errors)

Both take the step structure literally: psi * expVh, then nt // nout blocks of nout x (kinetic, * expV), one snapshot
per block; what follows the last snapshot is dropped as the reference drops it.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle.highprec import EXTENDED_OK, member_errors, worst_member  # noqa: E402,F401


# Axis lengths the GPU kernel tests probe: the issue's list, one value on each side of the K-tile edges 32 .. 128 of the
# plan (tests/test_ldr_plan_host.py holds the list against the plan's constants), and lengths of many tiles.
PROBE_LENGTHS = (1, 3, 15, 16, 17, 31, 33, 63, 64, 65, 95, 97, 127, 129, 257, 1023, 1025)


def ldr_dense(psi0, U, expV, expVh, expK, nt, nout):
    """Snapshots [nt // nout, *n, ns] of one state psi0 [*n, ns]; U [*n, M, ns]."""
    dims, ns = psi0.shape[:-1], psi0.shape[-1]
    npts = int(np.prod(dims))
    u = U.reshape(npts, U.shape[-2], ns)
    A = np.einsum('pma,qmb->paqb', u.conj(), u)
    Kfull = np.ones((1, 1), dtype=complex)
    for K in expK:
        Kfull = np.kron(Kfull, K)
    exp_T = (A * Kfull[:, None, :, None]).reshape(npts * ns, npts * ns)
    psi = (expVh * psi0).reshape(-1)
    ev = expV.reshape(-1)
    out = []
    for _ in range(nt // nout):
        for _ in range(nout):
            psi = ev * (exp_T @ psi)
        out.append(psi.reshape(dims + (ns,)).copy())
    return np.array(out).reshape((nt // nout,) + dims + (ns,))


def ldr_factorised(psi0s, U, expV, expVh, expK, nt, nout, dtype=np.complex128):
    """Snapshots [B, nt // nout, *n, ns] of the states psi0s [B, *n, ns], every operation in `dtype`."""
    psi = np.asarray(psi0s, dtype=dtype)
    U, expV, expVh = (np.asarray(a, dtype=dtype) for a in (U, expV, expVh))
    Ks = [np.asarray(K, dtype=dtype) for K in expK]
    ndim = len(Ks)
    psi = psi * expVh
    out = []
    for _ in range(nt // nout):
        for _ in range(nout):
            chi = np.einsum('...mb,z...b->z...m', U, psi)
            for d, K in enumerate(Ks):
                chi = np.moveaxis(np.tensordot(K, chi, axes=(1, d + 1)), 0, d + 1)
            psi = expV * np.einsum('...ma,z...m->z...a', U.conj(), chi)
        out.append(psi.copy())
    shape = (psi.shape[0], nt // nout) + psi.shape[1:]
    return np.stack(out, axis=1) if out else np.zeros(shape, dtype=dtype)


def random_case(seed, dims, M, ns, B, dt=0.05):
    """White noise everywhere the kernel reads: orthonormal complex states U [*dims, M, ns] (the first ns columns of
    a random unitary per point), surfaces in [0, 2), general complex axis matrices K_d of norm about one (neither
    symmetric nor unitary, so a transposed or conjugated operand shows), and B complex states of unit norm."""
    rng = np.random.default_rng(seed)
    dims = tuple(dims)
    npts = int(np.prod(dims))
    g = rng.standard_normal((npts, M, M)) + 1j * rng.standard_normal((npts, M, M))
    q, _ = np.linalg.qr(g)
    U = np.ascontiguousarray(q[:, :, :ns]).reshape(dims + (M, ns))
    apes = 2.0 * rng.random(dims + (ns,))
    expK = [(rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))) / np.sqrt(2.0 * n) for n in dims]
    psi = rng.standard_normal((B,) + dims + (ns,)) + 1j * rng.standard_normal((B,) + dims + (ns,))
    psi /= np.linalg.norm(psi.reshape(B, -1), axis=1).reshape((B,) + (1,) * (len(dims) + 1))
    return dict(dims=dims, M=M, ns=ns, U=U, apes=apes, expK=expK, psi=psi, dt=dt,
                expV=np.exp(-1j * dt * apes), expVh=np.exp(-1j * 0.5 * dt * apes))
