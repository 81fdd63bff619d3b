"""Extended-precision reference for the two batched dense propagators, qd_superop_rk4 (pyqed_amd/csrc/superop.hip) and
qd_tdse_rk4 / qd_tdse_driven_rk4 (pyqed_amd/csrc/tdse.hip): the classical RK4 of dV/dt = L V in plain numpy, with the
working precision as a parameter.  `dtype` is np.clongdouble (the x87 80-bit format on the hosts this suite runs on,
eps 1.08e-19) or np.complex128, which gives a float64 restatement of the same arithmetic for shapes at which extended
precision would take too long (numpy multiplies long doubles without a BLAS: 3 steps of N2 = 515 with 8 vectors take
0.4 s, N2 = 4096 with one vector 2.9 s).  No torch, no library call.  Every member, every save and every observable
is returned, in the layouts of the device entry points, rounded to complex128 once at the end.

    k1 = L v, k2 = L (v + dt/2 k1), k3 = L (v + dt/2 k2), k4 = L (v + dt k3), v += dt/6 (k1 + 2 k2 + 2 k3 + k4)

The kernels evaluate the same polynomial of dt L in Horner form; in exact arithmetic the two agree.  The functions earn
their role on the host first (tests/test_highprec_oracle_cpu.py)."""
from __future__ import annotations

import numpy as np

# where np.longdouble is only a second name for float64 the extended results below are plain float64 ones; the host
# test refuses to pass there
EXTENDED_OK = bool(np.finfo(np.longdouble).eps < 1e-18)


def _real(dtype):
    return np.empty(0, dtype=dtype).real.dtype.type


def _step(L, V, dt, dtype):
    real = _real(dtype)
    h, h2 = real(dt), real(dt) / real(2)
    k1 = L @ V
    k2 = L @ (V + k1 * h2)
    k3 = L @ (V + k2 * h2)
    k4 = L @ (V + k3 * h)
    return V + (k1 + real(2) * k2 + real(2) * k3 + k4) * (h / real(6))


def rk4_linear(L, V, dt, nsteps, save_every=0, dtype=np.clongdouble):
    """nsteps RK4 steps of dV/dt = L V on the columns of V [n, B] in `dtype`.  Returns (V_end [n, B], saves): saves[k]
    is the state after (k + 1) * save_every steps, k < nsteps // save_every (none for save_every = 0), so a last step
    that is no multiple of save_every is in V_end only.  Both stay in `dtype`."""
    L = np.asarray(L, dtype=dtype)
    V = np.array(V, dtype=dtype)
    saves = []
    for s in range(nsteps):
        V = _step(L, V, dt, dtype)
        if save_every > 0 and (s + 1) % save_every == 0:
            saves.append(V.copy())
    return V, saves


def _stack(saves, B, n):
    """[B, nsave, n] complex128 from a list of [n, B] states."""
    out = np.zeros((B, len(saves), n), dtype=np.complex128)
    for k, S in enumerate(saves):
        out[:, k, :] = S.T.astype(np.complex128)
    return out


def superop(L, v0, dt, nsteps, W=None, save_every=0, dtype=np.clongdouble):
    """qd_superop_rk4: v0 [B, N2] rows are the members.  Returns (v [B, N2], snap [B, nsteps // save_every, N2] | None,
    obs [B, nsteps + 1, ne] | None) with obs[b, s, m] = sum_k W[m, k] v_b[k] after s steps, s = 0 .. nsteps (every
    step, whatever save_every is), evaluated in `dtype`."""
    v0 = np.asarray(v0)
    B, n = v0.shape
    V0 = np.asarray(v0.T, dtype=dtype)
    Vend, every = rk4_linear(L, V0, dt, nsteps, 1, dtype)
    nsave = nsteps // save_every if save_every > 0 else 0
    snap = _stack([every[(k + 1) * save_every - 1] for k in range(nsave)], B, n) if nsave else None
    obs = None
    if W is not None:
        Wd = np.asarray(W, dtype=dtype)
        obs = np.zeros((B, nsteps + 1, Wd.shape[0]), dtype=np.complex128)
        for s, S in enumerate([V0] + every):
            obs[:, s, :] = (Wd @ S).T.astype(np.complex128)
    return Vend.T.astype(np.complex128), snap, obs


def expect(E, Psi, dtype=np.clongdouble):
    """<psi_b| E_m |psi_b> for the columns of Psi [N, B]: [B, ne] in `dtype`."""
    E = np.asarray(E, dtype=dtype)
    Psi = np.asarray(Psi, dtype=dtype)
    return np.stack([np.sum(np.conj(Psi) * (E[m] @ Psi), axis=0) for m in range(E.shape[0])], axis=1)


def tdse(H, psi0, dt, nsteps, save_every=0, E=None, dtype=np.clongdouble):
    """qd_tdse_rk4: rk4_linear with L = -iH, psi0 [B, N].  Returns (psi [B, N], snap [B, nsave, N] | None,
    obs [B, nsave + 1, ne] | None), nsave = nsteps // save_every, obs[b, 0] at t0 and obs[b, k + 1] with save k."""
    psi0 = np.asarray(psi0)
    B, N = psi0.shape
    L = np.asarray(H, dtype=dtype) * dtype(-1j)
    P0 = np.asarray(psi0.T, dtype=dtype)
    Pend, saves = rk4_linear(L, P0, dt, nsteps, save_every, dtype)
    snap = _stack(saves, B, N) if saves else None
    obs = None
    if E is not None:
        obs = np.stack([expect(E, S, dtype) for S in [P0] + saves], axis=1).astype(np.complex128)
    return Pend.T.astype(np.complex128), snap, obs


def tdse_driven(H0, Hd, fvals, psi0, dt, nout, E=None, dtype=np.clongdouble):
    """qd_tdse_driven_rk4: block k of nout steps runs with H = H0 - sum_d fvals[k, d] Hd[d] (Hd None or [nd, N, N],
    fvals [nblocks, nd]).  Returns (psi [B, N], snap [B, nblocks, N] | None, obs [B, nblocks + 1, ne] | None): one save
    after every block, obs[b, 0] at t0."""
    psi0 = np.asarray(psi0)
    B, N = psi0.shape
    fv = np.asarray(fvals, dtype=dtype)
    nblocks = fv.shape[0]
    nd = 0 if Hd is None else len(Hd)
    fv = fv.reshape(nblocks, nd)
    H0 = np.asarray(H0, dtype=dtype)
    P = np.asarray(psi0.T, dtype=dtype)
    states = [P]
    for k in range(nblocks):
        Ht = H0.copy()
        for d in range(nd):
            Ht = Ht - fv[k, d] * np.asarray(Hd[d], dtype=dtype)
        P, _ = rk4_linear(Ht * dtype(-1j), P, dt, nout, 0, dtype)
        states.append(P)
    snap = _stack(states[1:], B, N) if nblocks else None
    obs = None
    if E is not None:
        obs = np.stack([expect(E, S, dtype) for S in states], axis=1).astype(np.complex128)
    return P.T.astype(np.complex128), snap, obs


def member_errors(got, ref):
    """Relative L2 error of every member (leading index) of got against ref."""
    got = np.asarray(got)
    ref = np.asarray(ref)
    B = ref.shape[0]
    d = np.linalg.norm((got - ref).reshape(B, -1), axis=1)
    return d / np.maximum(np.linalg.norm(ref.reshape(B, -1), axis=1), 1e-300)


def worst_member(got, ref):
    """max_b relerr(got[b], ref[b]): one wrong member shows at full size however many right ones stand beside it."""
    assert np.shape(got) == np.shape(ref), (np.shape(got), np.shape(ref))
    return float(member_errors(got, ref).max())
