"""The launch plans of the 2DES response entry points (pyqed_amd/csrc/response_plan.hpp) on the host, compiled with the
host C++ compiler through tools/cpu_emu/response_plan_c.cpp.  Nothing of the rules is restated here: the tests
enumerate shapes, check that every planned launch is legal for the kernel it names and that the launches together cover
what the GEMM reads and the caller expects (what a kernel covers -- 256 columns per block, a member group per block row,
a grid-strided loop -- is the kernel's geometry, not a rule of the plan), that every refusal carries the entry point's
message, and that the typed dispatch reaches exactly the GEMM kernels that exist.  The anchors are what the GPU tests
(tests/test_response_edges_gpu.py, bench.py's grids) assert on hardware at their shapes."""
import ctypes
import itertools
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

EMU_DIR = os.path.join(ROOT, "tools", "cpu_emu")
GRID_X_MAX, GRID_YZ_MAX = 2 ** 31 - 1, 65535
LDS_DYNAMIC_MAX = 64 * 1024        # what a kernel may ask for without raising its limit; no response kernel raises it
(XTAB, Z_UNIFORM, X_UNIFORM, Z_PAD, XZ, Z_GENERIC, P_UNIFORM, P_PAD, E, REDUCE, REDUCE_TRANS, REDUCE_T2, PAD_SQUARE,
 RESOLVENT_OPERAND) = range(14)    # RespKernel
# Every ens_gemm_kernel instantiation: (noted name, BT, XTAB, DEPTH)
GEMM_KERNELS = {("ens_gemm64", 64, 0, 2), ("ens_gemm128_xtab", 128, 1, 1), ("ens_gemm128", 128, 0, 1)}
# Shapes whose plan holds a launch past a grid extent (to be fixed in the plan, pinned here until then): none at the
# sizes enumerated below.  The transposed reduction's grid y is ceil(n3 / 16) and ens_p_uniform_kernel's n3p / 64,
# neither guarded; they pass 65,535 from n3 = 1,048,561 and 4,194,177 on.
PINNED_GRID_FINDINGS = set()

MS = (1, 2, 255, 1023, 1024, 2047, 2048, 4096, 8192, 33000, 65535, 65536, 196609)
NLS = (1, 2, 9, 15, 16, 17, 40)
NS = (1, 15, 16, 17, 127, 128, 129, 257, 1024, 1025, 4096, 524161)
FN = "qd_response2d_ensemble_rect"


def ints(*names):
    return [(n, ctypes.c_int) for n in names]


def sizes(*names):
    return [(n, ctypes.c_size_t) for n in names]


class EnsDims(ctypes.Structure):
    _fields_ = ints("n3p", "n1p", "K", "tiles", "Kp")


class RespLaunch(ctypes.Structure):
    _fields_ = ints("kernel") + [("gx", ctypes.c_uint), ("gy", ctypes.c_uint)] + ints("M", "xrows", "xbx", "G") + \
               sizes("lds") + [("note", ctypes.c_char_p)]


class GemmPlan(ctypes.Structure):
    _fields_ = ints("bt", "xtab", "depth", "S") + [(n, ctypes.c_uint) for n in ("gx", "gy", "gz")] + \
               [("name", ctypes.c_char_p)]


class EnsPlan(ctypes.Structure):
    _fields_ = ints("refused") + [("d", EnsDims)] + ints("xtab", "nbuild") + \
               sizes("nX", "nZ", "nslabs", "offX", "offFine", "offZ", "offSlabs", "total") + \
               [("build", RespLaunch * 4), ("gemm", GemmPlan), ("reduce", RespLaunch), ("msg", ctypes.c_char * 192)]


class T2OpsPlan(ctypes.Structure):
    _fields_ = ints("refused") + [("d", EnsDims)] + ints("nbuild") + [("build", RespLaunch * 4),
                                                                       ("msg", ctypes.c_char * 192)]


class T2ApplyPlan(ctypes.Structure):
    _fields_ = ints("refused") + [("d", EnsDims)] + ints("S") + [(n, ctypes.c_uint) for n in ("gx", "gy", "gz")] + \
               [("ldz", ctypes.c_long)] + sizes("nE", "nslabs", "offE", "offSlabs", "total") + \
               [("e", RespLaunch), ("reduce", RespLaunch), ("msg", ctypes.c_char * 96)]


class ResolventPlan(ctypes.Structure):
    _fields_ = ints("np", "nxp", "nyp") + \
               sizes("nM", "nZ", "nW", "nX", "nslabs", "offM", "offZ", "offW", "offX", "offSlabs", "total") + \
               [("pad", RespLaunch), ("zop", RespLaunch), ("xop", RespLaunch), ("gemm1", GemmPlan), ("gemm2", GemmPlan),
                ("reduce1", RespLaunch), ("reduce2", RespLaunch)]


class SplitKPlan(ctypes.Structure):
    _fields_ = ints("refused") + [("gemm", GemmPlan), ("msg", ctypes.c_char * 48)]


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "c++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    so = str(tmp_path_factory.mktemp("plan") / "libresponse_plan.so")
    subprocess.run([cxx, "-std=c++17", "-O1", "-shared", "-fPIC", "-Wall", "-Werror",
                    os.path.join(EMU_DIR, "response_plan_c.cpp"), "-o", so], check=True)
    lib = ctypes.CDLL(so)
    for f in ("plan_resp_constants", "plan_ens_dims", "plan_ens", "plan_t2ops", "plan_t2apply",
              "plan_resolvent", "plan_splitk"):
        getattr(lib, f).restype = None
    lib.plan_z_lds.restype = ctypes.c_size_t
    lib.plan_ens_sizes_ok.argtypes = [ctypes.c_long, ctypes.c_long]
    c = (ctypes.c_int * 9)()
    lib.plan_resp_constants(c)
    (lib.BT, lib.KT, lib.ZMAX, lib.UNI_ROWS, lib.XU_ROWS, lib.UNI_MAXC, lib.MIN_TILES128, lib.YZ_MAX,
     lib.XZ_XROWS) = c
    assert (lib.BT, lib.KT, lib.YZ_MAX) == (128, 16, GRID_YZ_MAX)
    return lib


def up(a, b):
    return -(-a // b)


def check_grid(l, what):
    """One launch inside the grid extents and the dynamic LDS a kernel may ask for."""
    assert 1 <= l.gx <= GRID_X_MAX and l.lds <= LDS_DYNAMIC_MAX, what
    assert 1 <= l.gy <= GRID_YZ_MAX or what in PINNED_GRID_FINDINGS, what


def check_dims(lib, d, M, nL, n3, n1):
    assert d.n3p % lib.BT == 0 and 0 <= d.n3p - n3 < lib.BT and d.n1p % lib.BT == 0 and 0 <= d.n1p - n1 < lib.BT
    assert d.K == M * nL and d.Kp == d.tiles * lib.KT and 0 <= d.Kp - d.K < lib.KT


def check_gemm(lib, g, Mp, Np, tiles, hit, skinny=False):
    """The grid tiles Mp x Np exactly with the planned blocks, the split count is inside its rule's bound, and the
    typed dispatch reaches the kernel the plan names."""
    assert g.gx * g.bt == Np and g.gy * g.bt == Mp and g.gz == g.S and g.gy <= GRID_YZ_MAX
    assert 1 <= g.S <= max(1, tiles // (8 if skinny else 4)), (Mp, Np, tiles, g.S)
    assert lib.plan_gemm_dispatch(ctypes.byref(g)) == 100 * g.bt + 10 * g.xtab + g.depth
    key = (g.name.decode(), g.bt, g.xtab, g.depth)
    assert key in GEMM_KERNELS, key
    hit.add(key)


def check_z_uniform(lib, l, M, nL, nz, d, what):
    """ens_z_uniform_kernel: G members per block row, 256 columns per block, its tables in the planned LDS; returns the
    block rows left for X blocks."""
    assert nL <= lib.ZMAX and nz <= lib.ZMAX and d.n1p <= 16 * lib.UNI_MAXC, what
    assert l.M == M and l.G >= 1 and l.gx * 256 >= d.n1p, what
    # Mt, fine and coarse tables, lamz and beta of G members, 16 B each
    assert l.lds >= l.G * (nL * nz + nz * (16 + d.n1p // 16) + 2 * nz) * 16, what
    return l.gy - up(M, l.G)


def check_ens(lib, p, hit, paths, M, nL, nz, n3, n1, t3u, t1u, trans):
    what = (M, nL, nz, n3, n1, t3u, t1u, trans)
    d = p.d
    check_dims(lib, d, M, nL, n3, n1)
    # the workspace parts in order, without overlap, summing to the request
    assert (p.offX, p.offZ, p.offSlabs, p.total) == (0, p.nX, p.nX + p.nZ, p.nX + p.nZ + p.nslabs), what
    assert p.nX == d.n3p * d.Kp and p.nZ == d.Kp * d.n1p and p.nslabs >= p.gemm.S * d.n3p * d.n1p, what
    xblocks = up(d.Kp, 256) * (d.n3p // lib.XU_ROWS)
    z_rows, z_pad, x_writers, notes = 0, False, [], []
    for l in p.build[:p.nbuild]:
        check_grid(l, what)
        if l.note:
            notes.append(l.note.decode())
        if l.kernel == XTAB:          # a thread per column writes its 16 fine and n3p / 16 coarse entries
            assert p.xtab and l.gx * 256 >= d.Kp and p.offFine == (d.n3p // 16) * d.Kp, what
            assert p.offFine + 16 * d.Kp <= p.nX, what
            x_writers.append("tables")
        elif l.kernel == Z_UNIFORM:
            assert t1u and z_rows == 0, what
            riding = check_z_uniform(lib, l, M, nL, nz, d, what)
            z_rows = d.K
            if riding:                # X blocks in the block rows past the member groups
                assert riding == xblocks and l.xbx == up(d.Kp, 256), what
                x_writers.append("uniform")
        elif l.kernel == X_UNIFORM:   # block (x % xbx, x // xbx) of the (Kp / 256) x (n3p / 16) tiling
            assert l.gx == xblocks and l.xbx == up(d.Kp, 256) and l.gy == 1, what
            x_writers.append("uniform")
        elif l.kernel == Z_PAD:
            z_pad = True
        elif l.kernel == XZ:          # Z of member m in block row m < M, X grid-strided over the xrows after them
            assert l.gy == l.M + l.xrows and l.gx * 256 >= d.n1p, what
            if l.M:
                assert not t1u and l.M == M and nL <= lib.ZMAX and nz <= lib.ZMAX and z_rows == 0, what
                z_rows = d.K
            else:
                assert l.xrows == lib.XZ_XROWS, what
            if l.xrows:
                x_writers.append("array")
        elif l.kernel == Z_GENERIC:   # all Kp rows, grid-strided
            assert not t1u and z_rows == 0, what
            z_rows = d.Kp
        else:
            raise AssertionError(what + (l.kernel,))
    # Z rows [0, Kp): the build and the pad; X in full, once, from the kind of grid the call has
    assert z_rows == d.Kp or (z_rows == d.K and z_pad), what
    assert x_writers == (["array"] if not t3u else ["tables"] if p.xtab else ["uniform"]), what
    check_gemm(lib, p.gemm, d.n3p, d.n1p, d.tiles, hit)
    assert p.gemm.xtab == p.xtab, what
    check_grid(p.reduce, what)
    if trans:                         # 16 x 16 tiles
        assert p.reduce.kernel == REDUCE_TRANS and p.reduce.gx * 16 >= n1 and p.reduce.gy * 16 >= n3, what
    else:                             # grid-strided
        assert p.reduce.kernel == REDUCE and p.reduce.gy == 1, what
    paths.add(tuple(notes) + (p.gemm.name.decode(),))
    return notes + [p.gemm.name.decode()]


def ens(lib, M, nL, nz, n3, n1, t3u, t1u, trans=0, fn=FN):
    p = EnsPlan()
    lib.plan_ens(fn.encode(), M, nL, nz, n3, n1, t3u, t1u, trans, ctypes.byref(p))
    return p


def test_ensemble_plans_are_legal_and_cover(plan):
    """Every (M, nL, nz, n3, n1) of the lists, square (nz = nL) and rectangular, the four grid kinds, both trans."""
    lib = plan
    hit, paths, refused, accepted = set(), set(), 0, 0
    for M, nL in itertools.product(MS, NLS):
        if not lib.plan_ens_sizes_ok(M, nL):
            continue
        for nz, n3, n1, t3u, t1u, trans in itertools.product(NLS, NS, NS, (0, 1), (0, 1), (0, 1)):
            p = ens(lib, M, nL, nz, n3, n1, t3u, t1u, trans)
            if p.refused:
                d = p.d
                groups = up(M, lib.plan_z_group(nL, nz, d.n1p, M))
                assert t1u and (nL > lib.ZMAX or nz > lib.ZMAX or d.n1p > 16 * lib.UNI_MAXC or groups > GRID_YZ_MAX)
                assert p.msg.decode() == (f"{FN}: uniform t1 needs nL <= 16, n1 <= 1024 and at most 65535 member "
                                          f"groups (M = {M} makes {groups})")
                refused += 1
            else:
                check_ens(lib, p, hit, paths, M, nL, nz, n3, n1, t3u, t1u, trans)
                accepted += 1
    assert accepted > 500000 and refused > 50000, (accepted, refused)
    assert hit == GEMM_KERNELS                     # ens_gemm64_xtab is never planned
    # every order of notes these shapes take: the Z build's, then the GEMM's.  (A uniform X launch of its own needs
    # 256 < K < 512 at n3 = 524,161, which no M nL of the lists gives: test_ensemble_anchors plans it.)
    assert paths == {(z, g) for z in ("ens_z_uniform", "ens_z_array", "ens_z_generic")
                     for g in ("ens_gemm64", "ens_gemm128", "ens_gemm128_xtab")}


def test_ensemble_anchors(plan):
    """What the GPU tests assert on hardware at their shapes."""
    lib = plan
    hit, paths = set(), set()
    go = lambda M, nL, n3, n1, kind: (lambda p: (p, check_ens(lib, p, hit, paths, M, nL, nL, n3, n1, *kind, 0)))(
        ens(lib, M, nL, nL, n3, n1, *kind))
    for M, nL in ((1, 1), (3, 5), (2, 8), (17, 1), (7, 9), (5, 13)):      # test_ensemble_k_edges: K <= 65, one split
        for kind in ((1, 1), (0, 0)):
            assert go(M, nL, 20, 33, kind)[0].gemm.S == 1
    sw = lambda M, kind: (lambda p, names: (p.gemm.bt, p.gemm.S, names[-1]))(*go(M, 16, 256, 256, kind))
    assert sw(2047, (1, 1)) == (64, 32, "ens_gemm64")                     # test_ensemble_block_size_switch
    assert sw(2048, (1, 1)) == (128, 64, "ens_gemm128_xtab")
    assert sw(2048, (0, 1)) == (128, 64, "ens_gemm128")
    assert sw(8192, (1, 1)) == (128, 64, "ens_gemm128_xtab")              # the bench grid, K = 131,072
    assert sw(1024, (1, 1)) == (64, 32, "ens_gemm64")                     # its 1/8 shard, K = 16,384
    assert lib.plan_z_group(2, 2, 256, 65536) == 28
    for kind, name in (((1, 1), "ens_gemm128_xtab"), ((0, 1), "ens_gemm128")):   # test_ensemble_grid_extent_guard
        assert go(4096, 16, 4096, 16, kind)[1] == ["ens_z_uniform", name]
    # test_ensemble_x_blocks_past_grid_extent
    assert go(17, 16, 524161, 3, (1, 1))[1] == ["ens_z_uniform", "ens_x_uniform_own", "ens_gemm64"]
    p = ens(lib, 196609, 16, 16, 16, 128, 1, 1, fn="qd_response2d_ensemble_uniform")
    assert p.refused and p.msg.decode() == ("qd_response2d_ensemble_uniform: uniform t1 needs nL <= 16, n1 <= 1024 and "
                                            "at most 65535 member groups (M = 196609 makes 65537)")


def test_member_groups(plan):
    """z_group and z_lds over the enumeration: at least one member, at most 32, the tables inside the dynamic LDS
    whenever the uniform build can be planned (nL, nz <= ZMAX, n1p <= 1024)."""
    lib = plan
    for nL, nz, n1p, M in itertools.product(NLS, NLS, range(128, 1025, 128), MS):
        G = lib.plan_z_group(nL, nz, n1p, M)
        assert 1 <= G <= 32 and G <= max(1, M)
        if nL <= lib.ZMAX and nz <= lib.ZMAX:
            assert lib.plan_z_lds(G, nL, nz, n1p) <= 32 * 1024


def test_scan_plans(plan):
    """qd_response2d_t2_operands_rect and qd_response2d_t2_apply: the plan's dimensions are those of
    qd_response2d_t2_dims (the same ens_dims), P and Q written in full, the GEMM's columns map to waiting times."""
    lib = plan
    fo, fa = "qd_response2d_t2_operands_rect", "qd_response2d_t2_apply"
    for M, np_, nr, nq, n3, n1 in itertools.product((1, 15, 17, 86, 4096, 196609), (1, 9, 16), (1, 9, 16), (2, 16),
                                                    (1, 63, 64, 65, 129, 4096), (1, 40, 129, 1024)):
        what = (M, np_, nr, nq, n3, n1)
        p, dref = T2OpsPlan(), EnsDims()
        lib.plan_t2ops(fo.encode(), M, np_, nr, nq, n3, n1, ctypes.byref(p))
        lib.plan_ens_dims(M, nr, n3, n1, ctypes.byref(dref))
        groups = up(M, lib.plan_z_group(nr, nq, dref.n1p, M))
        if p.refused:
            assert groups > GRID_YZ_MAX and p.msg.decode() == f"{fo}: M={M} too large", what
            continue
        d = p.d
        check_dims(lib, d, M, nr, n3, n1)
        assert [getattr(d, f) for f, _ in EnsDims._fields_] == [getattr(dref, f) for f, _ in EnsDims._fields_]
        kinds = [l.kernel for l in p.build[:p.nbuild]]
        assert kinds == [P_UNIFORM] + [P_PAD] * (d.Kp > d.K) + [Z_UNIFORM] + [Z_PAD] * (d.Kp > d.K), what
        for l in p.build[:p.nbuild]:
            check_grid(l, what)
            if l.kernel == P_UNIFORM:     # 256 // max(np, nr) members per block, UNI_ROWS rows per block row
                assert l.gx * (256 // max(np_, nr)) >= M and l.gy * lib.UNI_ROWS == d.n3p, what
            elif l.kernel == Z_UNIFORM:   # Z rows only: no block row past the member groups
                assert check_z_uniform(lib, l, M, nr, nq, d, what) == 0 and l.xbx == 1, what
    for args, msg in (((3, 17, 4, 4, 8, 8), f"{fo}: np=17 nr=4 nq=4 (<= 16), n1=8 (<= 1024)"),
                      ((3, 4, 4, 4, 8, 1025), f"{fo}: np=4 nr=4 nq=4 (<= 16), n1=1025 (<= 1024)"),
                      ((1 << 27, 4, 8, 4, 8, 8), f"{fo}: M={1 << 27} too large")):
        p = T2OpsPlan()
        lib.plan_t2ops(fo.encode(), *args, ctypes.byref(p))
        assert p.refused and p.msg.decode() == msg
    hit = set()
    for M, nL, n3, n1, n2 in itertools.product((1, 5, 4096), (1, 9, 16), (1, 65, 129, 4096), (1, 40, 129, 1024),
                                               (1, 2, 5, 511, 512, 65535)):
        what = (M, nL, n3, n1, n2)
        p = T2ApplyPlan()
        lib.plan_t2apply(fa.encode(), M, nL, n3, n1, n2, ctypes.byref(p))
        n1p = up(n1, lib.BT) * lib.BT
        if p.refused:
            assert n2 * n1p // lib.BT > GRID_YZ_MAX and p.msg.decode() == f"{fa}: n2*n1 too large", what
            continue
        d = p.d
        check_dims(lib, d, M, nL, n3, n1)
        assert n2 * n1p // lib.BT <= GRID_YZ_MAX, what
        assert p.ldz == n2 * d.n1p and p.gx * lib.BT == p.ldz and p.gy * lib.BT == d.n3p and p.gz == p.S, what
        assert p.gx <= GRID_X_MAX and p.gy <= GRID_YZ_MAX and 1 <= p.S <= max(1, d.tiles // 4), what
        assert (p.offE, p.offSlabs, p.total) == (0, p.nE, p.nE + p.nslabs), what
        assert p.nE == n2 * d.Kp and p.nslabs >= p.S * d.n3p * p.ldz, what
        for l in (p.e, p.reduce):
            check_grid(l, what)
        assert (p.e.kernel, p.reduce.kernel) == (E, REDUCE_T2)
        hit.add(n2)
    assert {1, 65535} <= hit               # n2 = 65,535 with n1p = 128 is accepted; with n1p = 256 it is not
    p = T2ApplyPlan()
    lib.plan_t2apply(fa.encode(), 5, 9, 65, 129, 65535, ctypes.byref(p))
    assert p.refused and p.msg.decode() == "qd_response2d_t2_apply: n2*n1 too large"


def test_resolvent_and_splitk_plans(plan):
    lib = plan
    hit = set()
    for n, nx, ny in itertools.product((1, 40, 127, 128, 129, 4096, 65536), (1, 33, 129, 130, 65536),
                                       (1, 20, 257, 65536)):
        what = (n, nx, ny)
        p = ResolventPlan()
        lib.plan_resolvent(n, nx, ny, ctypes.byref(p))
        for v, vp in ((n, p.np), (nx, p.nxp), (ny, p.nyp)):
            assert vp % lib.BT == 0 and 0 <= vp - v < lib.BT, what
        offs = (p.offM, p.offZ, p.offW, p.offX, p.offSlabs, p.total)
        assert offs == tuple(itertools.accumulate((0, p.nM, p.nZ, p.nW, p.nX, p.nslabs))), what
        assert (p.nM, p.nZ, p.nW, p.nX) == (p.np * p.np, p.np * p.nyp, p.np * p.nyp, p.nxp * p.np), what
        check_gemm(lib, p.gemm1, p.np, p.nyp, p.np // lib.KT, hit)      # W = M Z
        check_gemm(lib, p.gemm2, p.nxp, p.nyp, p.np // lib.KT, hit)     # out = X W
        assert p.nslabs >= max(p.gemm1.S * p.np * p.nyp, p.gemm2.S * p.nxp * p.nyp), what
        for l in (p.pad, p.zop, p.xop, p.reduce1, p.reduce2):
            check_grid(l, what)
    assert hit == {("ens_gemm128", 128, 0, 1)}
    hit = set()
    for Mp, Kp, Np, max_S in itertools.product((128, 256, 1024, 4096), (16, 64, 1024, 32768, 1 << 20),
                                               (64, 128, 192, 256, 1024), (1, 8, 64)):
        p = SplitKPlan()
        lib.plan_splitk(Mp, Kp, Np, max_S, ctypes.byref(p))
        assert not p.refused
        check_gemm(lib, p.gemm, Mp, Np, Kp // lib.KT, hit, skinny=Np % 128 != 0)
        assert p.gemm.S <= max_S and (Np % 128 == 0 or p.gemm.bt == 64)
    assert hit == {("ens_gemm64", 64, 0, 2), ("ens_gemm128", 128, 0, 1)}
    for Mp, Kp, Np in ((64, 16, 128), (128, 8, 128), (128, 16, 96)):
        p = SplitKPlan()
        lib.plan_splitk(Mp, Kp, Np, 8, ctypes.byref(p))
        assert p.refused and p.msg.decode() == "cgemm_splitk_slabs: bad padding"


def test_unguarded_grid_y_extents(plan):
    """Findings not acted on ("Next"): two launches whose grid y grows with n3 and is not held against
    65,535.  The figures are what the plans give today at the smallest n3 past the extent and at the one before it;
    whether the runtime refuses such a launch has not been measured on hardware, and no GPU test goes there."""
    lib = plan
    for n3, gy in ((1048560, 65535), (1048561, 65536)):      # the transposed reduction: ceil(n3 / 16)
        p = ens(lib, 1, 16, 16, n3, 16, 1, 1, trans=1)
        assert not p.refused and (p.reduce.kernel, p.reduce.gy) == (REDUCE_TRANS, gy)
    for n3, gy in ((4194176, 65534), (4194177, 65536)):      # ens_p_uniform_kernel: n3p / 64, two per 128 rows
        p = T2OpsPlan()
        lib.plan_t2ops(b"qd_response2d_t2_operands_rect", 1, 16, 16, 16, n3, 16, ctypes.byref(p))
        assert not p.refused and (p.build[0].kernel, p.build[0].gy) == (P_UNIFORM, gy)
