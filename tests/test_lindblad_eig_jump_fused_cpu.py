"""lindblad_eig_jump_kernel's schedule restated in NumPy (glf_eig_jump_kernel.hpp, cg_dma_ksteps_xh in
cgemm_dma128.hpp), no GPU: k = X + X^+ formed tile by tile on the 36 16 x 16 tiles on and above the diagonal.  Per tile
of the kernel's table the first sum and, above the diagonal, the swapped and conjugated sum, both in the 3-product form
(the swapped one with the difference operands); the diagonal tiles' own dagger; the elementwise term carried in the
accumulators, T = M o v left by the tail of the pass before (half of it on a diagonal tile, which the dagger doubles); the
mirror written as the conjugate and the diagonal's imaginary part dropped.  Held to the oracle on the benchmark's seeded
operators within the project's bound, and the table to its partition and balance."""
import numpy as np

from conftest import relerr

TOL = 1e-10   # the project's bound against the oracle (test_lindblad_eig_jump_gpu.py)
DT = 1e-3
NP = 128

COLS = (0x3210, 0x7654, 0x4321, 0x7650, 0x7432, 0x6510, 0x7632, 0x5410)   # jump_ctile


def rtile(w, mi):
    return w >> 1 if mi == 0 else 7 - (w >> 1)


def ctile(w, nj):
    return (COLS[w] >> (4 * nj)) & 15


def wave_tiles(w):
    return [(rtile(w, mi), ctile(w, nj)) for mi in range(2) for nj in range(4)]


def test_table_partition_and_balance():
    """Every one of the 64 tiles has one owner; each SIMD's waves (w, w + 4) hold two diagonal and seven off-diagonal
    tiles on and above the diagonal (16 units of MFMA work); no wave holds more than five live tiles; the tiles whose
    rows or mirrors feed L.b[0] and L.b[1] are row tile mi == 0 of waves 0 .. 3."""
    owners = {}
    for w in range(8):
        for t in wave_tiles(w):
            assert t not in owners, (t, w, owners[t])
            owners[t] = w
    assert sorted(owners) == [(R, C) for R in range(8) for C in range(8)]
    for s in range(4):
        live = [t for w in (s, s + 4) for t in wave_tiles(w) if t[0] <= t[1]]
        assert sum(R == C for R, C in live) == 2 and sum(R < C for R, C in live) == 7
    for w in range(8):
        assert sum(R <= C for R, C in wave_tiles(w)) <= 5
        for mi in range(2):
            for nj in range(4):
                R, C = rtile(w, mi), ctile(w, nj)
                if R <= C and (R < 2 or C < 2):
                    assert w < 4 and mi == 0


def three_product(ar, ai, br, bi, sign):
    """(P1, P2, P3) of sum_k a b (sign = +1) or of sum_k conj(a) conj(b) (sign = -1): the third operand pair is the sum
    or the difference of the parts."""
    return ar @ br, ai @ bi, (ar + sign * ai) @ (br + sign * bi)


def fused_pass(A, Bm, base, mu, T, a, hc, gn):
    """rn = a base + hc (A Bm + (A Bm)^+ + T) by the kernel's per-tile schedule, T the elementwise term the pass before
    left in the accumulators ({(R, C): tile}, None = zero).  Returns rn and the T this pass leaves: gn M o rn,
    M_ij = mu_i conj(mu_j), on the tiles on and above the diagonal, halved on the diagonal ones."""
    rn = np.full((NP, NP), np.nan + 0j)
    Tn = {}
    for w in range(8):
        for R, C in wave_tiles(w):
            if R > C:
                continue
            rs, cs = slice(16 * R, 16 * R + 16), slice(16 * C, 16 * C + 16)
            t = T[(R, C)] if T is not None else np.zeros((16, 16), complex)
            p1, p2, p3 = t.real.copy(), np.zeros((16, 16)), t.real + t.imag   # (T_re, 0, T_re + T_im)
            fa, fb = A[rs, :], Bm[:, cs]                         # first sum: A rows R, B columns C
            q1, q2, q3 = three_product(fa.real, fa.imag, fb.real, fb.imag, +1)
            p1, p2, p3 = p1 + q1, p2 + q2, p3 + q3
            if R < C:                                            # swapped: B columns R as the A fragment, A rows C as B
                sa, sb = Bm[:, rs].T, A[cs, :].T
                q1, q2, q3 = three_product(sa.real, sa.imag, sb.real, sb.imag, -1)
                p1, p2, p3 = p1 + q1, p2 + q2, p3 + q3
            k = (p1 - p2) + 1j * ((p3 - p1) - p2)                # cg_dma_finalise
            if R == C:
                k = k + k.conj().T                               # the in-wave dagger
            v = a * base[rs, cs] + hc * k
            if R == C:
                v[np.diag_indices(16)] = v[np.diag_indices(16)].real
                u = np.triu(v)
                rn[rs, cs] = u + np.triu(u, 1).conj().T
            else:
                rn[rs, cs] = v
                rn[cs, rs] = v.conj().T
            Tn[(R, C)] = (0.5 if R == C else 1.0) * gn * np.outer(mu[rs], mu[cs].conj()) * v   # every lane's own v
    assert not np.isnan(rn).any()
    return rn, Tn


def fused_call(plan, rho0, dt, steps):
    """One call of the kernel on one padded matrix: change of basis, the Horner stages, change back.  A Y pass zeroes
    the accumulators; pass 1 leaves T for the first stage and the last stage leaves zero."""
    Wdh, Widh = plan.W.conj().T / 2, plan.Winv.conj().T / 2
    rho = np.zeros((NP, NP), complex)
    rho[:plan.N, :plan.N] = rho0
    rho, T = fused_pass(plan.Winv @ rho, Widh, rho, plan.mu, None, 0.0, 1.0, 1.0 if steps else 0.0)
    for n in range(steps):
        s = rho
        for m in range(4):
            last = n == steps - 1 and m == 3
            s, T = fused_pass(plan.At, s, rho, plan.mu, T, 1.0, dt / (4 - m), 0.0 if last else 1.0)
        rho = s
    assert all(not t.any() for t in T.values())   # zero ahead of the change back
    rho, _ = fused_pass(plan.W @ rho, Wdh, rho, plan.mu, None, 0.0, 1.0, 0.0)
    return rho[:plan.N, :plan.N]


def test_schedule_against_oracle():
    """The benchmark's seeded operators at N = 128, two steps, against the oracle; every result exactly Hermitian with
    an exactly real diagonal."""
    from oracle import lindblad as olb
    from pyqed_amd.oqs import build_eig_jump_plan
    N, B, steps = 128, 2, 2
    H, cs = olb.synthetic_lindblad(N, nc=1)
    rho0 = olb.random_pure_states(B, N, seed=1)
    plan = build_eig_jump_plan(H, np.array(cs))
    assert plan.ok, plan.reason
    got = np.array([fused_call(plan, rho0[b], DT, steps) for b in range(B)])
    err = relerr(got, olb.lindblad_batch(H, list(cs), rho0, DT, steps))
    print(f"fused schedule, N={N} B={B} steps={steps}: rel err {err:.3e}")
    assert err < TOL
    assert np.array_equal(got, got.conj().swapaxes(-1, -2))
    assert np.all(np.diagonal(got, axis1=-2, axis2=-1).imag == 0.0)


def test_swapped_sum_identity():
    """The 3-product form with the difference operands is conj(sum_k a b): A r + r A^+ for a Hermitian r."""
    rng = np.random.default_rng(0)
    A = rng.standard_normal((NP, NP)) + 1j * rng.standard_normal((NP, NP))
    r = rng.standard_normal((NP, NP)) + 1j * rng.standard_normal((NP, NP))
    r = r + r.conj().T
    k, T = fused_pass(A, r, r, np.ones(NP, complex), None, 0.0, 1.0, 0.0)
    assert all(not t.any() for t in T.values())
    ref = A @ r + r @ A.conj().T
    assert relerr(k, ref) < 1e-14
