"""The kernels of pyqed_amd/csrc/krylov.hip called directly through the C ABI, each against the extended-precision
host restatement oracle/krylov.py (which tests/test_krylov_oracle_cpu.py holds to 1e-14 of itself first), at the sizes
where their dispatch changes: the unrolled loops (8 loads in flight from n = 2048 in cgs_project_kernel, 6 from a
1536-column slice in dcgs_project_kernel), the column slices S = min(8, 1024 / (j + 1)), the row slices
G = min(16, j / 32), the 256-row and 64-lane strides of dcgs_coef_kernel, the 64 * 256 stride of the norm's partial
sums, the 256-thread stride of hess_shift_kernel and the two dynamic-LDS attribute thresholds (j > 3072, k > 2048).
Leading dimensions are wider than the data everywhere, the padding and every row a call must not write hold NaN
before the call and the same bits after it."""
import math

import numpy as np
import pytest
import torch

from conftest import relerr
from oracle import krylov as ok
from test_krylov_oracle_cpu import STEP_CASES, step_case, step_errors, step_outputs

pytestmark = pytest.mark.gpu

assert np.finfo(np.longdouble).eps < 1e-18, "np.longdouble is not an extended format on this host"

EPS = np.finfo(np.float64).eps
NAN = complex(np.nan, np.nan)
LD = np.clongdouble


def _dev():
    return torch.device("cuda", 0)


def _lib_stream():
    from pyqed_amd import _lib
    _lib.ensure_device(_dev())
    return _lib, _lib.load(), _lib.stream_ptr(_dev())


def _to_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64).reshape(a.shape + (-1,))


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _cplx(rng, *sh):
    return rng.standard_normal(sh + (2,)).view(np.complex128)[..., 0]


# ---- qd_cgs_project ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("m", [1, 5])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 2047, 2048, 2049, 4097, 40001])
def test_cgs_project(n, m):
    """h_r = V_r^H w, one workgroup per row: every thread adds ceil(n / 256) products (8 loads in flight from
    n = 2048, a tail below) and a tree of 8 levels adds the threads.  Per entry |h_r - ref| <= 4 (ceil(n / 256) + 12)
    eps sum_i |V_ri| |w_i|: the summation depth, 4 for the complex products and the two real sums per component.
    With hsum the Hessenberg column (stride 7 here) accumulates old + h, one fp64 addition per component, and nothing
    between the strides moves.  The reduction order is fixed: two calls agree bit for bit."""
    _lib, lib, st = _lib_stream()
    rng = np.random.default_rng([1, n, m])
    ldv, ldh = n + 3, 7
    V = np.full((m, ldv), NAN)
    V[:, :n] = _cplx(rng, m, n)
    w = np.full(n + 3, NAN)
    w[:n] = _cplx(rng, n)
    hs0 = _cplx(rng, m * ldh)
    Vd, wd = _to_dev(V), _to_dev(w)
    ref = ok.project(V[:, :n], w[:n])
    bound = 4 * (math.ceil(n / 256) + 12) * EPS * (np.abs(V[:, :n]) @ np.abs(w[:n]))
    outs = []
    for hsum in (None, hs0, None):
        h = torch.full((m + 2,), NAN, dtype=torch.complex128, device=_dev())
        hsd = _to_dev(hsum) if hsum is not None else None
        _lib.check(lib.qd_cgs_project(Vd.data_ptr(), ldv, m, n, wd.data_ptr(), h.data_ptr(), _lib.ptr(hsd), ldh, st),
                   "qd_cgs_project")
        h = h.cpu().numpy()
        assert np.isnan(h[m:]).all()
        err = np.abs((h[:m] - ref).astype(complex))
        print(f"n={n} m={m}: max |h - ref| / bound = {float((err / bound).max()):.3f}")
        assert np.all(err <= bound)
        if hsum is not None:
            got = hsd.cpu().numpy()
            want = hs0.copy()
            want[::ldh] = hs0[::ldh] + h[:m]
            assert _same_bits(got, want)
        outs.append(h)
    assert _same_bits(outs[0], outs[1]) and _same_bits(outs[0], outs[2])
    assert _same_bits(Vd.cpu().numpy(), V) and _same_bits(wd.cpu().numpy(), w)


# ---- qd_cgs_normalize -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 257, 16383, 16384, 16385, 70001])
def test_cgs_normalize(n):
    """*hsub = ||w|| (relative 1e-14) and v = w / ||w|| (normwise 1e-14); the partial sums stride by 64 * 256 = 16384.
    v aliased to w is tested: cgs_norm_scale_kernel reads part[] (complete before it starts) and element i of w only
    in the thread that then writes element i of v, so the in-place call must give the same bits.  An all-zero w gives
    *hsub = 0 and a zero, finite v (the 1e-300 floor).  Two calls agree bit for bit."""
    _lib, lib, st = _lib_stream()
    rng = np.random.default_rng([2, n])
    w = np.full(n + 3, NAN)
    w[:n] = _cplx(rng, n)
    nrm, vref = ok.normalize(w[:n])

    def run(wd, vd):
        hsub = torch.full((3,), NAN, dtype=torch.complex128, device=_dev())
        _lib.check(lib.qd_cgs_normalize(wd.data_ptr(), n, vd.data_ptr(), hsub.data_ptr(), st), "qd_cgs_normalize")
        hsub = hsub.cpu().numpy()
        assert np.isnan(hsub[1:]).all()
        return hsub[0], vd.cpu().numpy()

    wd = _to_dev(w)
    h1, v1 = run(wd, torch.full((n + 3,), NAN, dtype=torch.complex128, device=_dev()))
    h2, v2 = run(wd, torch.full((n + 3,), NAN, dtype=torch.complex128, device=_dev()))
    h3, v3 = run(wd, wd)   # in place
    assert h1.imag == 0 and abs(h1.real - float(nrm)) <= 1e-14 * float(nrm)
    assert np.isnan(v1[n:]).all()
    err = float(relerr(v1[:n], vref))
    print(f"n={n}: |hsub / ||w|| - 1| = {abs(h1.real / float(nrm) - 1):.2e}, v {err:.2e}")
    assert err < 1e-14
    assert _same_bits(h1, h2) and _same_bits(v1, v2)
    assert _same_bits(h1, h3) and _same_bits(v1, v3)
    hz, vz = run(torch.zeros(n + 3, dtype=torch.complex128, device=_dev()),
                 torch.full((n + 3,), NAN, dtype=torch.complex128, device=_dev()))
    assert hz == 0 and not vz[:n].any() and np.isnan(vz[n:]).all()


# ---- qd_arnoldi_dcgs2_step --------------------------------------------------------------------------------------------

def _step_state(n, j, V, z, H):
    """Device arrays for step j from step_case's inputs: V [j + 3, n + 3] and H [j + 2, j + 5] with NaN in the padding
    columns, in V's rows j + 1 and j + 2 and in the entries of H the step writes without reading; st and cs sized as
    shifted_krylov_solve sizes them for m_max = j + 1 and filled with NaN."""
    ldv, ldh = n + 3, j + 5
    Vp = np.full((j + 3, ldv), NAN)
    Vp[:j + 1, :n] = V[:j + 1]
    Hp = np.full((j + 2, ldh), NAN)
    Hp[:, :j + 1] = H
    zp = np.full(n + 3, NAN)
    zp[:n] = z
    m_max = j + 1
    st = torch.full((16 * (m_max + 2),), NAN, dtype=torch.complex128, device=_dev())
    cs = torch.full((2 * (m_max + 3),), NAN, dtype=torch.complex128, device=_dev())
    return Vp, Hp, zp, st, cs


def _run_step(n, j, Vp, Hp, zp, st, cs):
    _lib, lib, stream = _lib_stream()
    Vd, Hd, zd = _to_dev(Vp), _to_dev(Hp), _to_dev(zp)
    _lib.check(lib.qd_arnoldi_dcgs2_step(Vd.data_ptr(), Vp.shape[1], j, n, zd.data_ptr(), Hd.data_ptr(), Hp.shape[1],
                                         st.data_ptr(), cs.data_ptr(), stream), "qd_arnoldi_dcgs2_step")
    torch.cuda.synchronize()
    assert _same_bits(zd.cpu().numpy(), zp)
    return Vd.cpu().numpy(), Hd.cpu().numpy(), cs.cpu().numpy()


def _untouched(n, j, Vp, Hp, Vg, Hg):
    """V outside rows j, j + 1 (columns < n) and H outside columns j - 1 and j (rows <= j) keep their bits."""
    wV = np.zeros(Vp.shape, bool)
    wV[j:j + 2, :n] = True
    wH = np.zeros(Hp.shape, bool)
    wH[:j + 1, max(j - 1, 0):j + 1] = True
    return (np.array_equal(_bits(Vp)[~wV], _bits(Vg)[~wV]) and np.array_equal(_bits(Hp)[~wH], _bits(Hg)[~wH]))


@pytest.mark.parametrize("n,j", STEP_CASES)
def test_dcgs2_single_step(n, j):
    """One step against the extended-precision oracle, normwise relative 1e-13 (the project's figure for
    qd_deom_apply against the assembled generator; the fp64 restatement stays 100 times inside it on these inputs,
    tests/test_krylov_oracle_cpu.py): v_j, u_{j+1}, column j, column j - 1, h_{j,j-1} (exactly real) and
    cs[j + 1] = 1 / rho.  What each (n, j) reaches: (1, 0) the j = 0 path and dynamic LDS of max(1, j); (12293, 8)
    n = 8 * 1536 + 5, every slice runs the unrolled body once and an uneven tail; (12293, 63 / 64) G 1 -> 2;
    (3077, 127 / 128) S 8 -> 7; (12293, 300) S = 3, G = 9; (4099, 513) S = 1, G = 16; (2051, 1100)
    1024 / (j + 1) = 0 clamped to 1 and five rounds of the coefficient kernel's r += 256 loop; (3100, 3073) dynamic
    LDS above 48 KiB, the attribute call."""
    V, z, H = step_case(n, j)
    Vx, Hx, info = ok.dcgs2_step(V, j, z, H)
    assert np.sum(np.abs(info["s"]) ** 2) <= info["alpha"] / 4
    Vp, Hp, zp, st, cs = _step_state(n, j, V, z, H)
    Vg, Hg, csg = _run_step(n, j, Vp, Hp, zp, st, cs)
    errs = step_errors(step_outputs(Vg[:, :n], Hg[:, :j + 1], j), step_outputs(Vx, Hx, j), n, j, z, info["rho"])
    print(f"(n, j) = ({n}, {j}): " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    for name, err in errs.items():
        assert err < 1e-13, name
    rho = float(info["rho"])
    if j:
        assert Hg[j, j - 1].imag == 0 and abs(Hg[j, j - 1].real - rho) < 1e-13 * rho
    assert csg[j + 1].imag == 0 and abs(csg[j + 1].real * rho - 1) < 1e-13
    assert _untouched(n, j, Vp, Hp, Vg, Hg)
    st.fill_(NAN)
    cs.fill_(NAN)
    Vg2, Hg2, csg2 = _run_step(n, j, Vp, Hp, zp, st, cs)
    assert _same_bits(Vg, Vg2) and _same_bits(Hg, Hg2) and _same_bits(csg, csg2)


def test_dcgs2_step_exact_breakdown():
    """u_j = 0 and z = 0 at (n, j) = (300, 5): rho = 0 gives finite output, zero v_j, u_{j+1} and column j,
    h_{j,j-1} = 0 and cs[j + 1] = 0; column j - 1 keeps its values (s = 0)."""
    n, j = 300, 5
    V, z, H = step_case(n, j)
    V[j] = 0.0
    z[:] = 0.0
    Vp, Hp, zp, st, cs = _step_state(n, j, V, z, H)
    Vg, Hg, csg = _run_step(n, j, Vp, Hp, zp, st, cs)
    assert not Vg[j, :n].any() and not Vg[j + 1, :n].any() and not Hg[:j + 1, j].any()
    assert Hg[j, j - 1] == 0 and csg[j + 1] == 0
    assert np.array_equal(Hg[:j, j - 1], H[:j, j - 1])
    assert np.all(np.isfinite(csg[:2 * j + 2]))
    assert _untouched(n, j, Vp, Hp, Vg, Hg)


def _ld_dot_last(X, Y):
    """sum_i X[r, i] Y[s, i] of complex arrays in extended precision, from real products contracted over the last
    axis of both (numpy's real longdouble einsum in that layout runs several times faster than its complex matmul)."""
    X, Y = np.asarray(X, dtype=LD), np.asarray(Y, dtype=LD)
    xr, xi, yr, yi = (np.ascontiguousarray(a) for a in (X.real, X.imag, Y.real, Y.imag))
    e = lambda a, b: np.einsum("ri,si->rs", a, b)
    return (e(xr, yr) - e(xi, yi)) + 1j * (e(xr, yi) + e(xi, yr))


def test_dcgs2_run_on_a_diagonal_operator():
    """Steps j = 0 .. 150 on the device operator diag(lambda), lambda_i = -0.5 + i w_i, w uniform on [-6, 6],
    n = 12293, z = lambda * V[j] each step.  Judged in extended precision at k = 150: max |V_k^H V_k - I| < 1e-12
    (delayed re-orthogonalisation leaves the newest vectors once-projected, hence the wider margin) and
    ||Lambda V_k^T - V_{k+1}^T Hbar_k||_F / ||Lambda||_F < 1e-13; H exactly zero below a real positive
    sub-diagonal.  The oracle's own fp64 run stays below 1e-15 on both (tests/test_krylov_oracle_cpu.py)."""
    _lib, lib, stream = _lib_stream()
    n, k = 12293, 150
    rng = np.random.default_rng(150)
    lam = -0.5 + 1j * rng.uniform(-6, 6, n)
    b = _cplx(rng, n)
    ldv, ldh, m_max = n + 3, k + 6, k + 1
    Vp = np.full((k + 3, ldv), NAN)
    Vp[0, :n] = b
    Vd = _to_dev(Vp)
    Hd = torch.zeros((k + 2, ldh), dtype=torch.complex128, device=_dev())
    Hd[:, k + 1:] = NAN
    lamd = _to_dev(lam)
    W = torch.empty(n, dtype=torch.complex128, device=_dev())
    st = torch.full((16 * (m_max + 2),), NAN, dtype=torch.complex128, device=_dev())
    cs = torch.full((2 * (m_max + 3),), NAN, dtype=torch.complex128, device=_dev())
    for j in range(k + 1):
        torch.mul(lamd, Vd[j, :n], out=W)
        _lib.check(lib.qd_arnoldi_dcgs2_step(Vd.data_ptr(), ldv, j, n, W.data_ptr(), Hd.data_ptr(), ldh,
                                             st.data_ptr(), cs.data_ptr(), stream), "qd_arnoldi_dcgs2_step")
    Vg, Hg = Vd.cpu().numpy(), Hd.cpu().numpy()
    assert np.isnan(Vg[:, n:]).all() and np.isnan(Vg[k + 2]).all() and np.isnan(Hg[:, k + 1:]).all()
    Hb = Hg[:k + 1, :k]
    assert np.all(np.tril(Hb, -2) == 0) and not Hg[k + 1, :k + 1].any()
    sub = np.diag(Hb, -1)
    assert np.all(sub.imag == 0) and np.all(sub.real > 0)
    V1 = Vg[:k + 1, :n]
    orth = 0.0
    for r0 in range(0, k, 50):   # the upper block triangle of the Hermitian Gram matrix
        G = _ld_dot_last(V1[r0:r0 + 50].conj(), V1[r0:k])
        orth = max(orth, float(np.abs(G - np.eye(G.shape[0], G.shape[1])).max()))
    VT = np.ascontiguousarray(V1.T)
    r2 = np.longdouble(0)
    for c0 in range(0, k, 50):   # columns c0 .. c0 + 49 of Hbar_k end at row c0 + 50
        R = lam.astype(LD)[None, :] * V1[c0:c0 + 50].astype(LD) \
            - _ld_dot_last(np.ascontiguousarray(Hb[:c0 + 51, c0:c0 + 50].T), VT[:, :c0 + 51])
        r2 += np.sum(R.real ** 2 + R.imag ** 2)
    arn = float(np.sqrt(r2) / np.linalg.norm(lam))
    print(f"orthogonality {orth:.2e}, Arnoldi relation {arn:.2e}")
    assert orth < 1e-12
    assert arn < 1e-13


# ---- shifted_krylov_solve end to end ----------------------------------------------------------------------------------

class _DiagOpDev:
    """y = alpha lam * x on the device, standing in for DeomOperator (test infrastructure only)."""

    def __init__(self, lam):
        self.lam = _to_dev(lam)
        self.n = len(lam)
        self.dev = _dev()
        self.norm = float(np.abs(lam).max())

    def apply(self, x, y, alpha=1.0):
        torch.mul(self.lam, x, out=y)
        if alpha != 1.0:
            y.mul_(alpha)
        return y


# Arnoldi steps of shifted_krylov_solve's CPU path (torch CGS2 on the host, fp64) for the operators below, seeds
# included, and its relerr against the closed form
CPU_STEPS = {6: (473, 1.4e-14), 12: (935, 2.7e-14)}


@pytest.mark.parametrize("width,delayed", [(6, True), (12, True), (6, False)])
def test_shifted_krylov_solve_closed_form(width, delayed):
    """x(s) = b / (-lambda - s) for the diagonal operator lambda_i = -0.5 + i w_i, w uniform on [-width, width],
    n = 12293, five shifts 0.1 + i [-3, 3], the exact answer evaluated in extended precision.  Width 6 walks S down to
    2 and G up to 14, width 12 reaches S = 1 and G = 16 and Hessenberg solves at k > 256; the plain CGS2 path
    (ARNOLDI_DCGS2 False) runs qd_cgs_project's unrolled body (n >= 2048) and qd_cgs_normalize.  relerr < 1e-11 (the
    solver's target is 1e-12 per residual; the host path lands at 3e-14) and the step count within 15 % of the host
    path's."""
    from pyqed_amd import deom_krylov as dk
    n = 12293
    rng = np.random.default_rng([41, width])
    lam = -0.5 + 1j * rng.uniform(-width, width, n)
    b = _cplx(rng, n)
    shifts = 0.1 + 1j * np.linspace(-3, 3, 5)
    exact = b.astype(LD)[None, :] / (-lam.astype(LD)[None, :] - shifts.astype(LD)[:, None])
    try:
        dk.ARNOLDI_DCGS2 = delayed
        X, k = dk.shifted_krylov_solve(_DiagOpDev(lam), _to_dev(b), shifts)
    finally:
        dk.ARNOLDI_DCGS2 = True
    err = float(relerr(X.cpu().numpy(), exact))
    print(f"width {width} delayed {delayed}: k = {k}, relerr {err:.2e}")
    assert err < 1e-11
    k_cpu = CPU_STEPS[width][0]
    assert abs(k - k_cpu) <= 0.15 * k_cpu


# ---- qd_shifted_hessenberg_solve --------------------------------------------------------------------------------------

HESS_SHIFTS = 0.2 + 1j * np.array([-2.5, 0.4, 2.3])
HESS_BETA = 1.7


def hess_case(k, kind):
    """H [k + 1, k + 4] upper Hessenberg (row k: h_{k+1,k}), entries above the diagonal complex normal of variance
    1 / k, diagonal -(1.5 + U[0, 1]) + 0.2i N(0, 1), sub-diagonal by kind: 'mixed' complex normal of modulus ~2 (as
    large as the shifted diagonal), 'noswap' modulus 1e-3, 'swap' modulus 10, random phases; NaN in the padding
    columns.  'swap' also sets h_00 = -HESS_SHIFTS[1] + 1e-9: the first pivot candidate of that shift is 1e-9 against
    10, so an elimination that did not swap would lose nine digits there (with a diagonal of order 1 throughout,
    skipping the swaps costs a factor 300 only and stays below every bound: the multipliers of 5 raise the next
    pivots until they are harmless)."""
    rng = np.random.default_rng([3, k, {"mixed": 0, "noswap": 1, "swap": 2}[kind]])
    H = np.full((k + 1, k + 4), NAN)
    U = _cplx(rng, k + 1, k)
    U *= 1 / np.sqrt(2 * k)
    H[:, :k] = np.triu(U, 1)
    i = np.arange(k)
    H[i, i] = -(1.5 + rng.uniform(0, 1, k)) + 0.2j * rng.standard_normal(k)
    sub = {"mixed": 1.5 * _cplx(rng, k), "noswap": np.full(k, 1e-3 + 0j), "swap": np.full(k, 10.0 + 0j)}[kind]
    H[i + 1, i] = sub * np.exp(2j * np.pi * rng.uniform(0, 1, k))
    if kind == "swap":
        H[0, 0] = -HESS_SHIFTS[1] + 1e-9
    return H


def hess_replay(H, k, shifts):
    """The elimination of hess_shift_kernel replayed in extended precision, all shifts at once: (swap [S, k - 1],
    the smallest max/min ratio of the two pivot candidates' moduli over all steps and shifts)."""
    S = len(shifts)
    sh = np.asarray(shifts, dtype=LD)
    row = lambda r, c0: np.tile(-np.asarray(H[r, c0:k], dtype=LD), (S, 1))
    cur = row(0, 0)
    cur[:, 0] -= sh
    swaps = np.zeros((S, max(k - 1, 0)), bool)
    closest = np.inf
    for j in range(k - 1):
        nxt = row(j + 1, j)
        nxt[:, 1] -= sh
        c = cur[:, j:]
        an, ac = np.abs(nxt[:, 0]), np.abs(c[:, 0])
        swap = an > ac
        swaps[:, j] = swap
        closest = min(closest, float((np.maximum(an, ac) / np.minimum(an, ac)).min()))
        if swap.all() or not swap.any():   # (no row-wise selection needed: most of the host time at k = 4096)
            piv, oth = (nxt, c) if swap[0] else (c, nxt)
        else:
            piv = np.where(swap[:, None], nxt, c)
            oth = np.where(swap[:, None], c, nxt)
        cur[:, j + 1:] = oth[:, 1:] - (oth[:, 0] / piv[:, 0])[:, None] * piv[:, 1:]
    return swaps, closest


@pytest.mark.parametrize("kind", ["mixed", "noswap", "swap"])
@pytest.mark.parametrize("k", [2, 255, 256, 257, 2048, 2049, 4096])
def test_shifted_hessenberg_solve_boundaries(k, kind):
    """(-H_k - s I) y = beta e_1 at the 256-thread stride (k = 255, 256, 257), the dynamic-LDS attribute switch
    (k = 2048 / 2049) and the largest k, on matrices where the pivoting swaps some rows, none ('noswap': a replay of
    the elimination in extended precision finds no swap and no pivot comparison closer than a factor 2, so the
    device's fp64 comparisons cannot differ) and every row ('swap', likewise).  S = 3 shifts, 1 at k = 4096 (the
    pivot-row scratch is S k^2 16 B = 268 MB there).

    hess_residual (the normwise backward error in extended precision) < 1e-13 for every shift: the fp64 host
    elimination of the same form (deom_krylov._shift_solutions_dev on the CPU) measures at most 8.7e-17 on these
    matrices (at k = 2; 1.5e-17 and less for 255 <= k <= 2049), a factor 1000 inside.  res equals |h_{k+1,k} y_{k-1}| / beta recomputed from the
    returned Y in extended precision (relative 1e-12); Y = NULL returns the same bits of res.  For k <= 257 Y also
    matches numpy.linalg.solve to 1e-10, and 'noswap' and 'swap' are well conditioned by construction (the diagonal
    dominates, or the sub-diagonal does and the top-right corner closes the cycle): cond < 1e4 is asserted there."""
    _lib, lib, stream = _lib_stream()
    shifts = HESS_SHIFTS[1:2] if k == 4096 else HESS_SHIFTS
    S = len(shifts)
    H = hess_case(k, kind)
    swaps, closest = hess_replay(H, k, shifts)
    if kind == "noswap":
        assert not swaps.any() and closest > 2
    elif kind == "swap":
        assert swaps.all() and closest > 2
    elif k >= 255:
        assert swaps.any() and not swaps.all()
    Hd, shd = _to_dev(H), _to_dev(shifts)
    outs = []
    for want_y in (True, False):
        Y = torch.full((S, k + 1), NAN, dtype=torch.complex128, device=_dev())
        res = torch.full((S + 1,), np.nan, dtype=torch.float64, device=_dev())
        _lib.check(lib.qd_shifted_hessenberg_solve(Hd.data_ptr(), k + 4, k, shd.data_ptr(), S, HESS_BETA,
                                                   Y.data_ptr() if want_y else None, res.data_ptr(), stream),
                   "qd_shifted_hessenberg_solve")
        outs.append((Y.cpu().numpy(), res.cpu().numpy()))
    assert _same_bits(Hd.cpu().numpy(), H)
    (Yg, res), (Yn, res2) = outs
    assert np.isnan(Yn).all() and np.isnan(res[S]) and _same_bits(res, res2)
    # Y is [S, k] contiguous: the call's k-strided rows lie in the first S k entries of the [S, k + 1] buffer
    flat = Yg.reshape(-1)
    assert np.isnan(flat[S * k:]).all()
    Yg = flat[:S * k].reshape(S, k)
    for i, sft in enumerate(shifts):
        back = float(ok.hess_residual(H, k, HESS_BETA, sft, Yg[i]))
        r_ref = float(np.abs(LD(H[k, k - 1]) * LD(Yg[i, k - 1])) / np.longdouble(HESS_BETA))
        print(f"k={k} {kind} shift {sft}: backward error {back:.2e}, res {res[i]:.3e}")
        assert back < 1e-13
        assert abs(res[i] - r_ref) <= 1e-12 * r_ref
        if k <= 257:
            A = -H[:k, :k] - sft * np.eye(k)
            if kind != "mixed":
                assert np.linalg.cond(A) < 1e4
            assert relerr(Yg[i], np.linalg.solve(A, HESS_BETA * np.eye(k)[:, 0])) < 1e-10


def test_refused_arguments():
    """j > 8192, k > 4096 and ldv < n are refused on the host (QD_CHECK_ARG), before any launch."""
    _lib, lib, stream = _lib_stream()
    t = torch.zeros(64, dtype=torch.complex128, device=_dev())
    p = t.data_ptr()
    with pytest.raises(ValueError):
        _lib.check(lib.qd_arnoldi_dcgs2_step(p, 4, 8193, 4, p, p, 8194, p, p, stream), "qd_arnoldi_dcgs2_step")
    with pytest.raises(ValueError):
        _lib.check(lib.qd_arnoldi_dcgs2_step(p, 3, 1, 4, p, p, 2, p, p, stream), "qd_arnoldi_dcgs2_step")
    with pytest.raises(ValueError):
        _lib.check(lib.qd_cgs_project(p, 3, 1, 4, p, p, None, 1, stream), "qd_cgs_project")
    with pytest.raises(ValueError):
        _lib.check(lib.qd_shifted_hessenberg_solve(p, 4097, 4097, p, 1, 1.0, p, p, stream),
                   "qd_shifted_hessenberg_solve")
    assert not t.cpu().numpy().any()
