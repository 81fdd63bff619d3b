"""The 2DES response kernels (pyqed_amd/csrc/response.hip) entry by entry against the extended-precision closed form of
oracle/response.py, at the block, table and grid edges of the kernels: grids that start away from zero, sizes around
the 16-row groups, the 128-blocks and the 1024-column table limit, K below one K-tile, member groups and members per
block on both sides of their limits, the 64- / 128-block switch, and the grid-extent guard of the operand build.

Metric.  Every case uses max_ik |got - ref| / scale[i,k], where scale is the closed form with every term replaced by
its modulus (what a correct evaluation's rounding error is proportional to).  The signals decay as e^{Re(lam) t}; a
Frobenius norm over the grid sees the first rows and columns only, so an error of order one in the last 16-row group,
the last coarse-table entries or the padding would pass it.

Bound (derived, in units of eps = 2^-52; not tuned to the kernels' output).  Per term of the sum:
  * a direct exponential e^{lam t} = e^{Re t} (cos, sin)(Im t): the products lam t round to |lam| t eps / 2 of phase
    and exponent; a uniform grid's point as the kernel forms it, t0 + j dt with dt = (t_last - t_first) / (n - 1),
    lies up to 1.5 ulps of t from the host array's (its own two roundings and dt's error times j), another
    1.5 |lam| t; exp and sincos an ulp each:  2 |lam| t + 2;
  * a complex product: sqrt(5)/2 eps, taken as 1.2;
  * a fine-table entry (e^{lam dt})^j, j <= 15: j (|lam| dt + 2) + 1.2 j;  a coarse entry of ens_z_uniform_kernel,
    beta e^{lam t0} (e^{16 lam dt})^l, l <= 63: the same per factor and 1.2 (l + 1) for the products.  Together with the
    product of the two:  E(t, j, l) = 2 |lam| t + 3.2 (j + l) + 5, with l = 0 where the coarse factor is a direct
    exponential (every X / P build) and j = l = 0 on array grids (counted as if tabled: an upper bound);
  * the contractions inside an operand entry (Mt y, X B, C Y; nin terms in all): 1.2 + nin / 2;
  * the GEMM: one product and K sequential MFMA additions, K / 2, and up to K / 64 slab additions, K / 128: 0.6 K;
  * the waiting-time factor of the scan: a direct exponential (t2 is an array) and a product, |lam| t2 + 3.2.
      c(i, k) = E(t3_i, i & 15, 0) + E(t1_k, k & 15, k >> 4) + nin + 0.6 K + 4   (+ |lam| t2_j + 3.2 for the scan)
  with |lam| <= hypot(0.2, 2) for the inputs below.  The resolvent grid has two Smith divisions (6 each, with the
  rounding of -Im(lam) - w) and two GEMMs over n:  c = 1.2 n + 20.  With accumulate the stored sum rounds once more:
  the scale gains |out0| and c one.
  The asserted bound is 4 c(i, k) eps per entry, the margin of 4 for the unmodelled error of the device exp / sincos.
  Measured worsts (kernel, and a float64 numpy evaluation of the same closed form against the oracle) are recorded in
  DESIGN.md, "2DES response kernels: per-entry edge tests".

Inputs: lam with Re in [-0.2, -0.01], Im in [-2, 2]; complex normal alpha, beta, Mt, B, C; fixed seeds; uniform grids
t0 + dt arange(n) with t0 != 0; array grids the uniform ones plus 1e-3 sin(arange).  Every case prints its worst
figure before it asserts; QD_EDGE_REPORT=1 adds the float64 figure (the reference's own rounding)."""
import os

import numpy as np
import pytest
import torch

from conftest import took
from oracle import response as orr

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
MARGIN = 4.0
LMAX = float(np.hypot(0.2, 2.0))
REPORT = os.environ.get("QD_EDGE_REPORT") == "1"


# ----------------------------------------------------------------------------- helpers
def _grid(n, kind, t0=3.7, dt=0.5):
    t = t0 + dt * np.arange(n)
    return t if kind == "u" else t + 1e-3 * np.sin(np.arange(n))


def _E(t, idx, coarse):
    idx = np.asarray(idx)
    return 2 * LMAX * np.abs(t) + 3.2 * ((idx & 15) + ((idx >> 4) if coarse else 0)) + 5.0


def _c(t3, t1, K, nin, rows=None, cols=None, extra=0.0):
    """c(i, k) of the module docstring over (rows, cols) of the grid."""
    i = np.arange(len(t3)) if rows is None else np.asarray(rows)
    k = np.arange(len(t1)) if cols is None else np.asarray(cols)
    return _E(np.asarray(t3)[i], i, False)[:, None] + _E(np.asarray(t1)[k], k, True)[None, :] + nin + 0.6 * K + 4 + extra


def _check(tag, got, ref, sc, c, ref64=None):
    got = np.asarray(got)
    assert got.shape == ref.shape == sc.shape == np.broadcast_shapes(np.shape(c), ref.shape), (tag, got.shape, ref.shape)
    err = np.abs(got - ref) / sc
    frac = float(np.max(err / (MARGIN * c * EPS)))
    msg = f"edge {tag}: worst {float(np.max(err)) / EPS:.1f} eps, {frac:.1e} of the bound"
    if REPORT and ref64 is not None:
        msg += f"; float64 closed form {orr.entry_error(ref64(), ref, sc) / EPS:.1f} eps"
    print(msg)
    assert frac < 1.0, msg          # a NaN fails too
    return frac


def _members(M, nL, seed, nz=None):
    """lam, alpha [M, nL]; Mt [M, nL, nz]; beta [M, nz] (+ lam_z [M, nz] when nz is given)."""
    rng = np.random.default_rng(seed)
    cn = lambda *s: rng.standard_normal(s) + 1j * rng.standard_normal(s)
    lm = lambda n: -rng.uniform(0.01, 0.2, (M, n)) + 1j * rng.uniform(-2, 2, (M, n))
    if nz is None:
        return lm(nL), cn(M, nL), cn(M, nL, nL), cn(M, nL)
    return lm(nL), cn(M, nL), cn(M, nL, nz), cn(M, nz), lm(nz)


def _ens(inp, t3, t1, prune, **kw):
    from pyqed_amd.response import response2d_ensemble
    took("")
    out = response2d_ensemble(*inp, t3, t1, prune=prune, **kw)
    return out, took("")[1]


def _ens_case(tag, inp, t3, t1, prunes=(False, True), rows=None, cols=None, want=None, nin=None, before=None):
    """Both wrapper forms against the oracle on (rows, cols); want: path names every run must have taken; before() runs
    ahead of each."""
    lam, alpha, Mt, beta = inp
    M, nL = alpha.shape
    ref, sc = orr.ensemble_slice(lam, alpha, Mt, beta, lam, t3, t1, rows, cols)
    ref64 = lambda: orr.ensemble_slice(lam, alpha, Mt, beta, lam, t3, t1, rows, cols, dtype=np.complex128)[0]
    if M * nL > orr.EXT_MAX_K:
        ref64 = None                    # the oracle is the float64 pairwise form itself there
    c = _c(t3, t1, M * nL, nL if nin is None else nin, rows, cols)
    dev = torch.device("cuda", 0)
    for prune in prunes:
        if before:
            before()
        out, paths = _ens(inp, t3, t1, prune)
        assert tuple(out.shape) == (len(t3), len(t1))
        for w in want or ():
            assert w in paths, (tag, prune, w, paths)
        if rows is not None:
            out = out[torch.as_tensor(rows, device=dev)][:, torch.as_tensor(cols, device=dev)]
        _check(f"{tag} prune={prune} {' '.join(paths)}", out.cpu().numpy(), ref, sc, c, ref64)


def _split_plan(n3, n1, K):
    """split_plan of response.hip for the padded problem: (block size, splits)."""
    up = lambda a, b: -(-a // b)
    Mp, Np, tiles = up(n3, 128) * 128, up(n1, 128) * 128, up(K, 16)
    splits = lambda bt: max(1, min(up(512 if bt == 64 else 256, (Mp // bt) * (Np // bt)), max(1, tiles // 4)))
    S128 = splits(128)
    bt = 64 if (Mp // 128) * (Np // 128) * S128 < 256 or tiles // S128 < 32 else 128
    return bt, splits(bt)


# ----------------------------------------------------------------------------- fixed-t2 ensemble
# every size of {1, 15, 16, 17, 127, 128, 129, 257} once as n3 and once as n1, the extremes paired with themselves too
PAIRS = [(1, 129), (15, 16), (16, 257), (17, 1), (127, 17), (128, 15), (129, 128), (257, 127), (1, 1), (257, 257)]


@pytest.mark.parametrize("kind", ["uu", "ua", "au", "aa"])
@pytest.mark.parametrize("n3,n1", PAIRS)
def test_ensemble_grid_edges(n3, n1, kind):
    """(n3, n1) around the 16-row groups and the 128-blocks, the four grid kinds (uniform / array per side), M in
    {1, 3}, nL = 9, grids that start at 3.7 and 1.3."""
    t3, t1 = _grid(n3, kind[0]), _grid(n1, kind[1], 1.3, 0.4)
    for M in (1, 3):
        _ens_case(f"grid {n3}x{n1} {kind} M={M}", _members(M, 9, 100 * n3 + n1 + M), t3, t1)


@pytest.mark.parametrize("n1,path", [(1024, "ens_z_uniform"), (1025, "ens_z_array")])
def test_ensemble_table_limit(n1, path):
    """n1 = 1024 fills the coarse table (nC = 64: the longest product chain, 63 factors of e^{16 lam dt}); at 1025
    the wrapper falls back to the array grid.  Same bound on both sides."""
    t3, t1 = _grid(17, "u"), _grid(n1, "u", 1.3, 0.4)
    _ens_case(f"table n1={n1}", _members(3, 9, n1), t3, t1, want=[path])


@pytest.mark.parametrize("kind", ["uu", "aa"])
@pytest.mark.parametrize("nL", [1, 15, 16, 17])
def test_ensemble_nl_edges(nL, kind):
    """nL around ZMAX = 16: 17 cannot use the register tables and takes ens_z_generic_kernel, also on uniform host grids."""
    t3, t1 = _grid(33, kind[0]), _grid(40, kind[1], 1.3, 0.4)
    want = ["ens_z_generic"] if nL == 17 else ["ens_z_uniform"] if kind == "uu" else ["ens_z_array"]
    _ens_case(f"nL={nL} {kind}", _members(3, nL, nL), t3, t1, want=want)


@pytest.mark.parametrize("kind", ["uu", "aa"])
@pytest.mark.parametrize("M,nL", [(1, 1), (3, 5), (2, 8), (17, 1), (7, 9), (5, 13)])
def test_ensemble_k_edges(M, nL, kind):
    """K = M nL in {1, 15, 16, 17, 63, 65}: below, at and just past one and four K-tiles, one split.  Rows K .. Kp - 1
    of Z are padding that ens_z_pad_kernel zeroes; they meet zero columns of X, so stale finite scratch would not
    show.  Each run therefore follows a call of the same scratch size (Kp members of one eigenvalue, same grids)
    whose operands are NaN, as an earlier caller's could be: the scratch is handed out again with NaN in those rows."""
    from pyqed_amd.response import response2d_ensemble
    t3, t1 = _grid(20, kind[0]), _grid(33, kind[1], 1.3, 0.4)
    assert _split_plan(20, 33, M * nL)[1] == 1
    Kp = -(-M * nL // 16) * 16
    nan = np.full((Kp, 1), np.nan + 0j)
    poison = lambda: response2d_ensemble(nan - 0.1, nan, nan[:, :, None], nan, t3, t1, prune=False)
    _ens_case(f"K={M * nL} {kind}", _members(M, nL, 7 * M + nL), t3, t1, before=poison)


def _sparse(M, nL, P, Q, seed):
    lam, alpha, Mt, beta = _members(M, nL, seed)
    za, zb = np.ones(nL, bool), np.ones(nL, bool)
    za[list(P)] = False
    zb[list(Q)] = False
    alpha[:, za] = 0
    beta[:, zb] = 0
    return lam, alpha, Mt, beta


@pytest.mark.parametrize("kind", ["uu", "aa"])
@pytest.mark.parametrize("na,nb", [(4, 2), (2, 4), (16, 1), (1, 16), (17, 3)])
def test_ensemble_pruned_supports(na, nb, kind):
    """alpha supported on na and beta on nb eigen indices: the wrapper keeps the supports, puts the smaller on K and
    transposes the output when that is beta's ((4, 2), (16, 1), (17, 3)).  70 x 45 leaves partial 16 x 16 tiles on
    both sides of the transposed reduction.  Then accumulate=True onto a non-zero grid: out = out0 + S."""
    from pyqed_amd.response import _prune_fixed_t2, response2d_ensemble
    nL = max(na, nb) + 2
    P = np.arange(1, na + 1)
    Q = np.arange(nL - nb, nL)
    inp = _sparse(5, nL, P, Q, 31 * na + nb)
    lam, alpha, Mt, beta = inp
    pr = _prune_fixed_t2(*(torch.from_numpy(x) for x in inp))
    assert pr[0] == (nb < na) and (pr[1].shape[1], pr[4].shape[1]) == (min(na, nb), max(na, nb))
    t3, t1 = _grid(70, kind[0]), _grid(45, kind[1], 1.3, 0.4)
    ref, sc = orr.ensemble_slice(lam, alpha, Mt, beta, lam, t3, t1)
    ref64 = lambda: orr.ensemble_slice(lam, alpha, Mt, beta, lam, t3, t1, dtype=np.complex128)[0]
    c = _c(t3, t1, 5 * min(na, nb), max(na, nb))
    out, paths = _ens(inp, t3, t1, True)
    _check(f"support ({na},{nb}) {kind} {' '.join(paths)}", out.cpu().numpy(), ref, sc, c, ref64)
    rng = np.random.default_rng(na)
    out0 = sc * np.exp(2j * np.pi * rng.uniform(size=sc.shape))
    acc = torch.from_numpy(out0.copy()).cuda()
    response2d_ensemble(*inp, t3, t1, out=acc, accumulate=True)
    _check(f"support ({na},{nb}) {kind} accumulate", acc.cpu().numpy() - out0, ref, sc + np.abs(out0), c + 1)


@pytest.mark.parametrize("trans", [0, 1])
@pytest.mark.parametrize("nx,nz", [(4, 2), (2, 4), (16, 1), (1, 16), (17, 3)])
def test_ensemble_rect_entry(nx, nz, trans):
    """qd_response2d_ensemble_rect itself, every (nx, nz) with the plain and the transposed reduction
    (ens_reduce_trans_kernel, partial tiles on both sides at 70 x 45), written and accumulated.  nx = 17 is past the
    table build, so its t1 is an array."""
    from pyqed_amd import _lib
    dev = torch.device("cuda", 0)
    M = 5
    lx, alpha, Mt, beta, lz = _members(M, nx, 17 * nx + nz + trans, nz=nz)
    t3, t1 = _grid(70, "u"), _grid(45, "u" if nx <= 16 else "a", 1.3, 0.4)
    ref, sc = orr.ensemble_slice(lx, alpha, Mt, beta, lz, t3, t1)
    c = _c(t3, t1, M * nx, nz)
    T = lambda x, dt=torch.complex128: torch.from_numpy(np.ascontiguousarray(x)).to(device=dev, dtype=dt)
    ops = [T(x) for x in (alpha, lx, Mt, beta, lz)]
    t1d = T(t1, torch.float64)
    p1 = (None, t1[0], (t1[-1] - t1[0]) / 44) if nx <= 16 else (t1d.data_ptr(), 0.0, 0.0)
    rng = np.random.default_rng(nx)
    out0 = sc * np.exp(2j * np.pi * rng.uniform(size=sc.shape))
    for acc in (0, 1):
        start = out0 if acc else np.full(sc.shape, np.nan + 0j)
        out = T(start.T if trans else start)
        rc = _lib.load().qd_response2d_ensemble_rect(ops[0].data_ptr(), ops[1].data_ptr(), nx, ops[2].data_ptr(),
                                                     ops[3].data_ptr(), ops[4].data_ptr(), nz, M, None, t3[0], 0.5, 70,
                                                     p1[0], p1[1], p1[2], 45, trans, out.data_ptr(), acc,
                                                     _lib.stream_ptr(dev))
        _lib.check(rc, "qd_response2d_ensemble_rect")
        got = out.cpu().numpy()
        got = got.T if trans else got
        if acc:
            _check(f"rect ({nx},{nz}) trans={trans} accumulate", got - out0, ref, sc + np.abs(out0), c + 1)
        else:
            _check(f"rect ({nx},{nz}) trans={trans}", got, ref, sc, c)


@pytest.mark.parametrize("M,G,last", [(1023, 1, 1), (1024, 1, 1), (3073, 3, 1), (33000, 32, 8)])
def test_ensemble_member_groups(M, G, last):
    """ens_z_uniform_kernel's member groups (z_group: min(32, LDS cap, M / 1024) members per block) at nL = 2: one
    member per block up to M = 2047, three with a last block of one at 3073, the cap of 32 with a last block of 8 at
    33,000.  Every member distinct; sampled rows and columns."""
    nL, n3, n1 = 2, 40, 100
    per = nL * nL + nL * (16 + 128 // 16) + 2 * nL
    g = max(1, min(max(1, min(32, 2048 // per)), M // 1024))
    assert (g, M - (-(-M // g) - 1) * g) == (G, last)
    rows, cols = [0, 15, 16, 39], [0, 15, 16, 17, 63, 64, 99]
    _ens_case(f"groups M={M}", _members(M, nL, M), _grid(n3, "u"), _grid(n1, "u", 1.3, 0.4), prunes=(False,),
              rows=rows, cols=cols, want=["ens_z_uniform"])


EDGE_RC = [0, 15, 16, 127, 128, 255]


@pytest.mark.parametrize("M,kind,path", [(2047, "uu", "ens_gemm64"), (2048, "uu", "ens_gemm128_xtab"),
                                         (2051, "uu", "ens_gemm128_xtab"), (2048, "au", "ens_gemm128"),
                                         (2051, "au", "ens_gemm128")])
def test_ensemble_block_size_switch(M, kind, path):
    """256 x 256, nL = 16: 2047 K-tiles over 64 splits leave 31 per workgroup (64-blocks), 2048 leave 32 (128-blocks:
    the A operand from tables on a uniform t3, materialised from an array t3); 2051 gives the splits uneven K-tile
    ranges.  Every member distinct, so a swapped or repeated K range shows."""
    assert _split_plan(256, 256, 16 * M) == ((64, 32) if M == 2047 else (128, 64))
    t3, t1 = _grid(256, kind[0]), _grid(256, kind[1], 1.3, 0.4)
    _ens_case(f"switch M={M} {kind}", _members(M, 16, M), t3, t1, prunes=(kind == "au",), rows=EDGE_RC, cols=EDGE_RC,
              want=[path, "ens_z_uniform"])


@pytest.mark.parametrize("kind", ["uu", "au"])
def test_ensemble_grid_extent_guard(kind):
    """M = 4096, nL = 16, n3 = 4096, n1 = 16: 128-blocks, so no X blocks are launched, yet their count (65,536) used to
    be held against the operand build's grid extent and the call was refused with 'uniform t1 needs nL <= 16 and n1 <=
    1024'.  Expected: the grid, on a uniform t3 (tables) and on an array t3."""
    M, nL, n3, n1 = 4096, 16, 4096, 16
    assert _split_plan(n3, n1, M * nL)[0] == 128
    rows = [0, 15, 16, 2047, 2048, 4080, 4095]
    _ens_case(f"guard {kind}", _members(M, nL, 4096), _grid(n3, kind[0], 3.7, 0.01), _grid(n1, "u", 1.3, 0.4),
              prunes=(kind == "au",), rows=rows, cols=list(range(n1)),
              want=["ens_gemm128_xtab" if kind == "uu" else "ens_gemm128", "ens_z_uniform"])


def test_ensemble_x_blocks_past_grid_extent():
    """The smallest shape whose launched X blocks overflow the operand build's grid: 64-blocks (K < 512), two
    256-column blocks (K > 256) and n3p / 16 = 32,768 row groups, n3 = 524,161.  X is then built in a launch of its
    own instead of the call being refused."""
    M, nL, n3, n1 = 17, 16, 524161, 3
    assert _split_plan(n3, n1, M * nL)[0] == 64
    rows = [0, 15, 16, 262143, 262144, 524159, 524160]
    _ens_case("own X launch", _members(M, nL, 5), _grid(n3, "u", 3.7, 1e-4), _grid(n1, "u", 1.3, 0.4), prunes=(False,),
              rows=rows, cols=[0, 1, 2], want=["ens_gemm64", "ens_z_uniform", "ens_x_uniform_own"])


# ----------------------------------------------------------------------------- waiting-time scan
T2 = {1: [25.0], 2: [0.0, 25.0], 5: [0.0, 1.3, 4.0, 7.5, 25.0]}


def _scan_inputs(M, nL, seed):
    rng = np.random.default_rng(seed)
    cn = lambda *s: rng.standard_normal(s) + 1j * rng.standard_normal(s)
    lam = -rng.uniform(0.01, 0.2, (M, nL)) + 1j * rng.uniform(-2, 2, (M, nL))
    return lam, cn(M, nL), cn(M, nL, nL), cn(M, nL, nL), cn(M, nL)


def _scan_case(tag, inp, t3, t2, t1, prune, sizes=None):
    from pyqed_amd.response import T2Scan, response2d_t2scan
    lam, alpha, B, C, beta = inp
    M, nL = alpha.shape
    ref, sc = orr.t2_scan(lam, alpha, B, lam, C, beta, lam, t3, t2, t1)
    ref64 = lambda: orr.t2_scan(lam, alpha, B, lam, C, beta, lam, t3, t2, t1, dtype=np.complex128)[0]
    npp, nr, nq = sizes or (nL, nL, nL)
    c = _c(t3, t1, M * nr, npp + nq)[None] + (LMAX * np.abs(np.asarray(t2)) + 3.2)[:, None, None]
    if sizes:
        assert T2Scan(lam, alpha, B, C, beta, t3, t1).index_sizes == sizes
    got = response2d_t2scan(lam, alpha, B, C, beta, t3, np.asarray(t2), t1, prune=prune).cpu().numpy()
    _check(tag, got, ref, sc, c, ref64)
    return ref, sc, c


@pytest.mark.parametrize("n2", [1, 2, 5])
@pytest.mark.parametrize("n1", [40, 129])
@pytest.mark.parametrize("n3", [63, 64, 65])
def test_t2scan_grid_edges(n3, n1, n2):
    """n3 around UNI_ROWS = 64 (ens_p_uniform_kernel's rows per block), n1 = 40 and 129 (n1p = 128 and 256, so the
    n2 * n1p / 128 column blocks map to waiting times one to one and two to one), non-uniform t2 with 0 and 25."""
    _scan_case(f"scan {n3}x{n2}x{n1}", _scan_inputs(5, 9, n3 + n1 + n2), _grid(n3, "u"), T2[n2], _grid(n1, "u", 1.3, 0.4),
               False)


@pytest.mark.parametrize("nL,M", [(16, 15), (16, 16), (16, 17), (9, 28), (9, 29), (3, 85), (3, 86)])
def test_t2scan_members_per_block(nL, M):
    """ens_p_uniform_kernel packs floor(256 / max(np, nr)) members into a block: 16, 28 and 85 members for nL = 16, 9
    and 3; one member fewer, exactly one block, and the first member of a second block."""
    assert 256 // nL in (M, M - 1, M + 1)
    _scan_case(f"scan members nL={nL} M={M}", _scan_inputs(M, nL, 100 * nL + M), _grid(65, "u"), T2[2],
               _grid(40, "u", 1.3, 0.4), False)


def _ladder(M, seed):
    """The 3-level ladder 'lccc' ensemble of tests/test_response_prune.py: p in {1,3,5,7}, r in {0,2,4,6}, q in {1,3}."""
    from pyqed_amd.response import ensemble_factors_bc, redfield_superop_batch
    from pyqed_amd.superoperator import operator_to_superoperator
    rng = np.random.default_rng(seed)
    E = np.array([0.0, 1.0, 1.5]) + np.array([0.0, 0.05, 0.08]) * rng.standard_normal((M, 3))
    R = redfield_superop_batch(E, np.diag([0.0, 1.0, 2.0]), np.full((M, 3, 3), 0.05))
    lam, U1 = np.linalg.eig(R)
    U2 = np.linalg.inv(U1)
    dip = np.zeros((3, 3)); dip[0, 1] = dip[1, 0] = dip[1, 2] = dip[2, 1] = 1.0
    ops = [operator_to_superoperator(dip, s).toarray() for s in "lccc"]
    rho0v = np.zeros(9, complex); rho0v[0] = 1
    return (lam,) + ensemble_factors_bc(lam, U1, U2, ops, rho0v)


def _synthetic_pruned(M, seed):
    """nL = 9 with alpha on 5 indices, B C coupled through 3 and beta on 2: np, nr, nq all different."""
    lam, alpha, B, C, beta = _scan_inputs(M, 9, seed)
    keep = lambda n, idx: np.isin(np.arange(n), idx)
    alpha[:, ~keep(9, [0, 2, 3, 6, 8])] = 0
    beta[:, ~keep(9, [4, 7])] = 0
    B[:, :, ~keep(9, [1, 5, 6])] = 0
    return lam, alpha, B, C, beta


@pytest.mark.parametrize("case", ["ladder", "synthetic"])
def test_t2scan_pruned_operands(case):
    """Pruned index sets against the oracle on the unpruned operands (the dropped terms are exact zeros): the ladder
    sets (4, 4, 2) and a synthetic (5, 3, 2); then T2Scan.apply in two buckets, accumulate=True onto non-zero output."""
    from pyqed_amd.response import T2Scan
    M = 37
    inp, sizes = (_ladder(M, 37), (4, 4, 2)) if case == "ladder" else (_synthetic_pruned(M, 41), (5, 3, 2))
    t3, t1, t2 = _grid(70, "u"), _grid(129, "u", 1.3, 0.4), np.array(T2[5])
    ref, sc, c = _scan_case(f"scan pruned {case}", inp, t3, t2, t1, True, sizes)
    rng = np.random.default_rng(9)
    out0 = sc * np.exp(2j * np.pi * rng.uniform(size=sc.shape))
    scan = T2Scan(*inp, t3, t1)
    lo = torch.from_numpy(out0[:2].copy()).cuda()
    hi = torch.from_numpy(out0[2:].copy()).cuda()
    scan.apply(t2[:2], out=lo, accumulate=True)
    scan.apply(t2[2:], out=hi, accumulate=True)
    got = np.concatenate([lo.cpu().numpy(), hi.cpu().numpy()])
    _check(f"scan pruned {case} buckets accumulate", got - out0, ref, sc + np.abs(out0), c + 1)


# ----------------------------------------------------------------------------- resolvent grid
def _resolvent(a, Mm, v, lam, wx, wy):
    from pyqed_amd import _lib
    dev = torch.device("cuda", 0)
    T = lambda x, dt=torch.complex128: torch.from_numpy(np.ascontiguousarray(x)).to(device=dev, dtype=dt)
    args = [T(a), T(Mm), T(v), T(lam)]
    wxt, wyt = T(wx, torch.float64), T(wy, torch.float64)
    out = torch.full((len(wx), len(wy)), float("nan"), dtype=torch.complex128, device=dev)
    rc = _lib.load().qd_resolvent_grid2d(*(x.data_ptr() for x in args), len(lam), wxt.data_ptr(), len(wx),
                                         wyt.data_ptr(), len(wy), out.data_ptr(), _lib.stream_ptr(dev))
    _lib.check(rc, "qd_resolvent_grid2d")
    return out.cpu().numpy()


@pytest.mark.parametrize("n,nx,ny", [(1, 33, 20), (127, 33, 20), (128, 33, 20), (129, 33, 20), (40, 1, 130),
                                     (40, 130, 1), (40, 129, 257)])
def test_resolvent_grid_edges(n, nx, ny):
    """qd_resolvent_grid2d at n around the 128-block (n is a row, a column and the K dimension), one-row, one-column
    and ragged grids; every fourth pole lies within 1e-3 of the frequency axis and on the grid's range, so entries
    differ by orders of magnitude."""
    rng = np.random.default_rng(1000 * n + nx + ny)
    lam = -rng.uniform(0.05, 2, n) + 1j * rng.uniform(-4, 4, n)
    lam[::4] = -rng.uniform(1e-4, 1e-3, len(lam[::4])) + 1j * rng.uniform(-3, 3, len(lam[::4]))
    a, v = (rng.standard_normal(n) + 1j * rng.standard_normal(n) for _ in range(2))
    Mm = rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))
    wx, wy = -4 + 8 * np.arange(nx) / max(nx - 1, 1) + 0.013, -3 + 9 * np.arange(ny) / max(ny - 1, 1) - 0.007
    if nx > 1:
        lam[0] = -2e-4 - 1j * (wx[nx // 2] + 1e-4)      # x_0 has its pole 2.2e-4 from a grid point
    if ny > 1 and (n > 1 or nx == 1):
        lam[-1] = -2e-4 - 1j * (wy[ny // 2] - 1e-4)     # z_{n-1} likewise
    ref, sc = orr.resolvent_grid(a, Mm, v, lam, wx, wy)
    assert np.max(sc) / np.min(sc) > 100
    ref64 = lambda: orr.resolvent_grid(a, Mm, v, lam, wx, wy, dtype=np.complex128)[0]
    _check(f"resolvent n={n} {nx}x{ny}", _resolvent(a, Mm, v, lam, wx, wy), ref, sc, 1.2 * n + 20.0, ref64)
