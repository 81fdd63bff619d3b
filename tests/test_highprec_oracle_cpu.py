"""oracle/highprec.py, the extended-precision RK4 that judges qd_superop_rk4 and qd_tdse_rk4 / qd_tdse_driven_rk4
(tests/test_superop_tails_gpu.py, tests/test_tdse_tails_gpu.py), against three things that share no code with it: the
project's float64 oracles, the exact propagator at a dt where RK4's truncation is below 1e-12, and a diagonal 2 x 2
case whose every saved value is known in closed form."""
import numpy as np
import scipy.linalg

from conftest import relerr
from oracle import highprec as hp
from oracle import lindblad as olb
from oracle import tdse as otd

assert np.finfo(np.longdouble).eps < 1e-18, "np.longdouble is not an extended format on this host"


def _cplx(rng, *shape):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


def test_tdse_matches_the_float64_oracle():
    """Every member, save and observable against oracle.tdse._rk4 / _obs (the restatement of the reference's loop) for
    a non-Hermitian H at N = 130, B = 3, 5 steps saved every 2.  Measured: 1.1e-15 at worst."""
    rng = np.random.default_rng(1)
    N, B, steps, se, dt = 130, 3, 5, 2, 0.1
    H = _cplx(rng, N, N) / np.sqrt(N)
    E = _cplx(rng, 2, N, N)
    psi0 = _cplx(rng, B, N)
    psi, snap, obs = hp.tdse(H, psi0, dt, steps, se, E)
    assert psi.dtype == snap.dtype == obs.dtype == np.complex128
    assert snap.shape == (B, 2, N) and obs.shape == (B, 3, 2)
    worst = 0.0
    for b in range(B):
        p = psi0[b].copy()
        assert relerr(obs[b, 0], [otd._obs(p, e) for e in E]) < 1e-14
        for s in range(steps):
            p = otd._rk4(p, H, dt)
            if (s + 1) % se == 0:
                k = (s + 1) // se
                worst = max(worst, relerr(snap[b, k - 1], p), relerr(obs[b, k], [otd._obs(p, e) for e in E]))
        worst = max(worst, relerr(psi[b], p))
    print(f"highprec.tdse vs oracle.tdse: {worst:.2e}")
    assert worst < 1e-14


def test_superop_matches_the_float64_lindblad_oracle():
    """vec(rho) under the kron-assembled Lindblad generator against oracle.lindblad.lindblad_batch (commutator form) at
    N = 6 (N2 = 36), B = 3, 4 steps; the trace observable W = vec(I) stays 1 at every step.  Measured: 1.2e-16."""
    N, B, steps, dt = 6, 3, 4, 0.05
    H, cs = olb.synthetic_lindblad(N, nc=2, gamma=0.5)
    rho0 = olb.random_pure_states(B, N, seed=4)
    I = np.eye(N)
    L = -1j * (np.kron(H, I) - np.kron(I, H.T))   # row-major vec: A rho -> kron(A, I), rho A -> kron(I, A^T)
    for c in cs:
        cdc = c.conj().T @ c
        L = L + np.kron(c, c.conj()) - 0.5 * (np.kron(cdc, I) + np.kron(I, cdc.T))
    v, snap, obs = hp.superop(L, rho0.reshape(B, N * N), dt, steps, W=I.reshape(1, N * N).astype(complex), save_every=1)
    assert snap.shape == (B, steps, N * N) and obs.shape == (B, steps + 1, 1)
    worst = 0.0
    for s in range(1, steps + 1):
        ref = olb.lindblad_batch(H, cs, rho0, dt, s)
        worst = max(worst, hp.worst_member(snap[:, s - 1].reshape(B, N, N), ref))
    worst = max(worst, hp.worst_member(v.reshape(B, N, N), ref))
    print(f"highprec.superop vs oracle.lindblad: {worst:.2e}")
    assert worst < 1e-14
    assert np.abs(obs - 1).max() < 1e-15


def test_against_the_exact_propagator():
    """dt = 1e-3 with ||L|| ~ 2.8: RK4's truncation is (||L|| dt)^5 / 120 = 1.4e-15 per step, so 10 steps sit within
    1e-12 of expm(10 dt L) v (scipy's Pade expm in float64), for a dense L and for a driven TDSE whose exact propagator
    is the ordered product of one expm per block.  Measured: 6.3e-16 and 1.5e-15."""
    rng = np.random.default_rng(2)
    n, B, dt = 40, 3, 1e-3
    L = _cplx(rng, n, n) / np.sqrt(n)
    v0 = _cplx(rng, B, n)
    v, _, _ = hp.superop(L, v0, dt, 10)
    e1 = hp.worst_member(v, (scipy.linalg.expm(10 * dt * L) @ v0.T).T)
    H0 = _cplx(rng, n, n) / np.sqrt(n)
    Hd = _cplx(rng, 2, n, n) / np.sqrt(n)
    fv = 0.4 * _cplx(rng, 3, 2)
    psi, snap, _ = hp.tdse_driven(H0, Hd, fv, v0, dt, 4)
    U = np.eye(n)
    e2 = 0.0
    for k in range(3):
        U = scipy.linalg.expm(-1j * 4 * dt * (H0 - fv[k, 0] * Hd[0] - fv[k, 1] * Hd[1])) @ U
        e2 = max(e2, hp.worst_member(snap[:, k], (U @ v0.T).T))
    assert np.array_equal(snap[:, -1], psi)
    print(f"vs expm: dense {e1:.2e}, driven {e2:.2e}")
    assert e1 < 1e-12 and e2 < 1e-12


def test_saved_index_layout_on_a_diagonal_2x2():
    """L = diag(a, b): one RK4 step multiplies component i by p(z_i) = 1 + z + z^2/2 + z^3/6 + z^4/24, z_i = dt L_ii,
    so the state after s steps is p^s v0, whatever the code does.  5 steps saved every 2: two saves (after 2 and 4
    steps), the fifth step in the final state only; superop observables after every step (6 rows), TDSE observables with
    the saves (3 rows); driven blocks of nout = 2 switch the generator between blocks."""
    a, b, dt = -0.3 + 0.7j, 0.2 - 0.5j, 0.2
    L = np.diag([a, b])
    p = lambda z: 1 + z + z ** 2 / 2 + z ** 3 / 6 + z ** 4 / 24   # noqa: E731
    g = np.array([p(a * dt), p(b * dt)])
    v0 = np.array([[1.0 + 0j, 2.0], [0.5j, -1.0]])                # two members
    W = np.array([[1.0, 1j], [2.0, 0.0], [0.0, -1.0]])
    v, snap, obs = hp.superop(L, v0, dt, 5, W=W, save_every=2)
    assert snap.shape == (2, 2, 2) and obs.shape == (2, 6, 3)
    for m in range(2):
        assert relerr(v[m], g ** 5 * v0[m]) < 1e-15
        assert relerr(snap[m, 0], g ** 2 * v0[m]) < 1e-15 and relerr(snap[m, 1], g ** 4 * v0[m]) < 1e-15
        for s in range(6):
            assert relerr(obs[m, s], W @ (g ** s * v0[m])) < 1e-15
    assert hp.superop(L, v0, dt, 5)[1:] == (None, None)
    assert hp.superop(L, v0, dt, 1, save_every=2)[1] is None      # fewer steps than one save
    # TDSE with H = iL so that -iH = L
    E = np.array([[[1.0, 2j], [0.5, -1.0]]])
    psi, snap, obs = hp.tdse(1j * L, v0, dt, 5, 2, E)
    assert snap.shape == (2, 2, 2) and obs.shape == (2, 3, 1)
    for m in range(2):
        assert relerr(psi[m], g ** 5 * v0[m]) < 1e-15
        for k in range(3):
            x = g ** (2 * k) * v0[m]
            assert relerr(obs[m, k, 0], np.conj(x) @ E[0] @ x) < 1e-15
            if k:
                assert relerr(snap[m, k - 1], x) < 1e-15
    # driven: H0 = iL, one drive Hd = i diag(1, -1): block k runs with L - f_k diag(1, -1)
    f = np.array([[0.3 + 0.1j], [-0.2j], [0.0]])
    psi, snap, obs = hp.tdse_driven(1j * L, np.array([1j * np.diag([1.0, -1.0])]), f, v0, dt, 2, E)
    assert snap.shape == (2, 3, 2) and obs.shape == (2, 4, 1)
    x = v0.copy()
    for k in range(3):
        gk = np.array([p((a - f[k, 0]) * dt), p((b + f[k, 0]) * dt)]) ** 2
        x = x * gk
        for m in range(2):
            assert relerr(snap[m, k], x[m]) < 1e-15
            assert relerr(obs[m, k + 1, 0], np.conj(x[m]) @ E[0] @ x[m]) < 1e-15
    assert relerr(psi, x) < 1e-15
    # no drive and no block: the t0 row only
    psi, snap, obs = hp.tdse_driven(1j * L, None, np.zeros((0, 0)), v0, dt, 2, E)
    assert snap is None and obs.shape == (2, 1, 1) and np.array_equal(psi, v0)


def test_float64_restatement_sits_at_rounding_of_the_extended_one():
    """The floor under the 1e-12 the kernels are held to: the same code in complex128 against np.clongdouble, dense L
    at N2 = 515 with 8 members of growing scale, dt = 0.2, 3 steps.  Measured: 5.6e-16 per member at worst."""
    rng = np.random.default_rng(3)
    n, B = 515, 8
    L = _cplx(rng, n, n) / np.sqrt(n)
    v0 = _cplx(rng, B, n) * (1 + np.arange(B))[:, None]
    W = _cplx(rng, 3, n)
    lo = hp.superop(L, v0, 0.2, 3, W=W, save_every=1, dtype=np.complex128)
    hi = hp.superop(L, v0, 0.2, 3, W=W, save_every=1)
    errs = [hp.worst_member(x, y) for x, y in zip(lo, hi)]
    print(f"complex128 vs clongdouble at N2 = 515: {max(errs):.2e}")
    assert max(errs) < 1e-14
    assert hp.member_errors(hi[0] * np.array([1, 1, 1, 1 + 1e-9, 1, 1, 1, 1])[:, None], hi[0]).argmax() == 3
