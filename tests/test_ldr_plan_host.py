"""The launch plan of qd_ldr_run (pyqed_amd/csrc/ldr_plan.hpp) on the host, compiled with the host C++ compiler through
tools/cpu_emu/ldr_plan_c.cpp.  Nothing of the rules is restated here: the tests enumerate shapes and check that every
planned launch is legal, that the row tiles, K-tiles and column sub-tiles cover every index exactly once, that no point
straddles two sub-tiles of a projecting pass, that the LDS is within its limit and as large as its use, that the
scratch parts do not overlap, that the buffers chain from pass to pass, and that every refusal carries its message.
What a workgroup covers (LDR_RT rows, LDR_NSUB sub-tiles of cu columns, K in tiles of LDR_KT) is the kernel's geometry,
read from the plan's constants.  The C entry's own checks run without a GPU: they come before any device work."""
import ctypes
import itertools
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

EMU_DIR = os.path.join(ROOT, "tools", "cpu_emu")
GRID_X_MAX, GRID_YZ_MAX = 2 ** 31 - 1, 65535
FN = "qd_ldr_run"
AUTO, FUSED, SPLIT = 0, 1, 2
BUF_PSI, BUF_W0, BUF_W1 = 0, 1, 2


class LdrLaunch(ctypes.Structure):
    _fields_ = [(n, ctypes.c_uint) for n in ("gx", "gy", "gz")] + [("tpb", ctypes.c_int), ("lds", ctypes.c_size_t)]


class LdrAxis(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int) for n in ("n", "ktiles", "cu", "expand", "project", "src", "dst")] + \
               [(n, ctypes.c_uint) for n in ("s", "st", "outer", "C")] + [("launch", LdrLaunch)]


class LdrPlan(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int) for n in ("refused", "path", "ndim", "M", "ns", "B")] + \
               [("n", ctypes.c_int * 3), ("npts", ctypes.c_long), ("nsnap", ctypes.c_int), ("nrun", ctypes.c_int),
                ("axis", LdrAxis * 3), ("expand_dst", ctypes.c_int), ("project_src", ctypes.c_int)] + \
               [(n, LdrLaunch) for n in ("open", "expand", "project")] + \
               [(n, ctypes.c_size_t) for n in ("ws_psi0", "ws_psi1", "ws_w0", "ws_w1", "ws_total")] + \
               [("msg", ctypes.c_char * 200)]


CONSTANTS = ("MAX_DIM", "MAX_M", "MAX_N", "WAVES", "TPB", "SUB", "RT", "NSUB", "CT", "KT", "BS_STRIDE", "DS_STRIDE",
             "FUSE_MIN_COLS", "POINT_GRID_MAX", "INDEX_MAX", "LDS_MAX")


def build_plan_lib(tmp):
    """The plan library and its constants as attributes."""
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "c++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    so = os.path.join(str(tmp), "libldr_plan.so")
    subprocess.run([cxx, "-std=c++17", "-O1", "-shared", "-fPIC", "-Wall", "-Werror",
                    os.path.join(EMU_DIR, "ldr_plan_c.cpp"), "-o", so], check=True)
    lib = ctypes.CDLL(so)
    lib.plan_ldr.restype = None
    lib.plan_ldr.argtypes = [ctypes.c_char_p, ctypes.c_long, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                             ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(LdrPlan)]
    lib.plan_ldr_constants.restype = None
    c = (ctypes.c_long * len(CONSTANTS))()
    lib.plan_ldr_constants(c)
    for name, v in zip(CONSTANTS, c):
        setattr(lib, name, int(v))
    return lib


def plan_of(lib, B, dims, M, ns, nsteps=5, nout=2, path=AUTO, fn=FN):
    p = LdrPlan()
    d = None if dims is None else (ctypes.c_int * max(1, len(dims)))(*dims)
    lib.plan_ldr(fn.encode(), B, 0 if dims is None else len(dims), d, M, ns, nsteps, nout, path, ctypes.byref(p))
    return p


def edge_lengths(lib):
    """1 .. 130 and the values around every multiple of the K-tile, the row tile, the MFMA tile and the staged columns
    up to four tiles, and around the longest axis."""
    out = set(range(1, 131))
    for c in (lib.KT, lib.RT, lib.SUB, lib.CT):
        for m in range(1, 5):
            out |= {m * c - 1, m * c, m * c + 1}
    out |= {1023, 1024, 1025, lib.MAX_N - 1, lib.MAX_N}
    return sorted(n for n in out if 1 <= n <= lib.MAX_N)


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    lib = build_plan_lib(tmp_path_factory.mktemp("plan"))
    assert (lib.MAX_DIM, lib.MAX_M) == (3, 32) and lib.MAX_N >= 1024
    assert lib.TPB == 64 * lib.WAVES and lib.RT == lib.SUB * lib.WAVES and lib.CT == lib.SUB * lib.NSUB
    assert lib.SUB == 16 and lib.KT % 4 == 0 and (lib.KT * lib.CT) % lib.TPB == 0 and lib.TPB % lib.CT == 0
    assert lib.BS_STRIDE >= lib.CT and lib.DS_STRIDE >= lib.SUB and lib.LDS_MAX <= 64 * 1024
    return lib


def check_launch(l, what, lds_max):
    assert 1 <= l.gx <= GRID_X_MAX and 1 <= l.gy <= GRID_YZ_MAX and 1 <= l.gz <= GRID_YZ_MAX, what
    assert l.tpb % 64 == 0 and 64 <= l.tpb <= 1024 and l.lds <= lds_max and l.lds % 16 == 0, what


def check_plan(lib, p, B, dims, M, ns, nsteps, nout, path_req, what):
    ndim = len(dims)
    npts = 1
    for n in dims:
        npts *= n
    fusable = lib.plan_ldr_fusable(M) > 0
    assert (p.ndim, p.M, p.ns, p.B, p.npts) == (ndim, M, ns, B, npts) and list(p.n[:ndim]) == list(dims), what
    assert p.path == ((FUSED if fusable else SPLIT) if path_req == AUTO else path_req), what
    fused = p.path == FUSED
    assert (p.nsnap, p.nrun) == (nsteps // nout, nsteps // nout * nout), what
    s = npts
    prev_dst = BUF_PSI if fused else p.expand_dst
    for d in range(ndim):
        a, n = p.axis[d], dims[d]
        s //= n
        assert (a.n, a.s, a.st, a.outer, a.C) == (n, s, s * M, npts // (n * s), B * npts * M // n), (what, d)
        # rows, K and columns: every index in exactly one tile
        check_launch(a.launch, (what, d), lib.LDS_MAX)
        assert a.launch.tpb == lib.TPB and (a.launch.gy - 1) * lib.RT < n <= a.launch.gy * lib.RT, (what, d)
        assert (a.ktiles - 1) * lib.KT < n <= a.ktiles * lib.KT, (what, d)
        assert 1 <= a.cu <= lib.SUB, (what, d)
        per_wg = lib.NSUB * a.cu
        assert (a.launch.gx - 1) * per_wg < a.C <= a.launch.gx * per_wg, (what, d)
        assert (a.expand, a.project) == (int(fused and d == 0), int(fused and d == ndim - 1)), (what, d)
        need = lib.KT * lib.BS_STRIDE * 16
        if a.project:
            # the M values of a point inside one sub-tile; the pass is the last axis
            assert a.cu == lib.plan_ldr_fusable(M) >= lib.FUSE_MIN_COLS and a.cu % M == 0 and a.C % M == 0, (what, d)
            assert a.s == 1 and a.st == M, (what, d)
            need += lib.WAVES * lib.SUB * lib.DS_STRIDE * 16
        else:
            assert a.cu == lib.SUB, (what, d)
        assert a.launch.lds >= need, (what, d)
        # the buffers chain, and no pass but psi -> psi' (its own two states) reads what it writes
        assert a.src == prev_dst and (a.src != a.dst or a.src == BUF_PSI), (what, d)
        assert a.src in (BUF_PSI, BUF_W0, BUF_W1) and a.dst in (BUF_PSI, BUF_W0, BUF_W1), (what, d)
        assert (a.src == BUF_PSI) == bool(a.expand) and (a.dst == BUF_PSI) == bool(a.project), (what, d)
        prev_dst = a.dst
    assert prev_dst == (BUF_PSI if fused else p.project_src), what
    for l, elems in ((p.open, B * npts * ns), (p.expand, B * npts * M), (p.project, B * npts * ns)):
        check_launch(l, what, 0)
        assert l.gx <= lib.POINT_GRID_MAX and (l.gx == lib.POINT_GRID_MAX or l.gx * l.tpb >= elems), what
    # scratch: two states, two work arrays, in order and without overlap
    offs = (p.ws_psi0, p.ws_psi1, p.ws_w0, p.ws_w1, p.ws_total)
    need = (B * npts * ns * 16,) * 2 + (B * npts * M * 16,) * 2
    assert offs[0] == 0 and all(o % 256 == 0 for o in offs), what
    assert all(b - a >= n for a, b, n in zip(offs, offs[1:], need)), (what, offs, need)


def shapes_with(n):
    """The probed length alone, and on the first, middle and last axis beside short ones."""
    return [(n,), (n, 3), (3, n), (n, 3, 4), (3, n, 4), (3, 4, n)]


def test_plans_are_legal_and_cover(plan):
    lib = plan
    pairs = [(1, 1), (2, 2), (3, 2), (5, 3), (9, 2), (16, 3), (17, 2), (32, 32)]
    count, paths = 0, set()
    for n, (M, ns), B in itertools.product(edge_lengths(lib), pairs, (1, 3, 64)):
        for dims in shapes_with(n):
            p = plan_of(lib, B, dims, M, ns)
            assert not p.refused, (dims, M, ns, B, p.msg)
            check_plan(lib, p, B, dims, M, ns, 5, 2, AUTO, (dims, M, ns, B))
            paths.add(p.path)
            count += 1
    assert count > 20000 and paths == {FUSED, SPLIT}


def test_every_m_and_ns_on_both_paths(plan):
    lib = plan
    count = 0
    fused_m = set()
    for M in range(1, lib.MAX_M + 1):
        for ns, B, dims in itertools.product(range(1, M + 1), (1, 3, 64), ((1,), (17,), (65, 3), (3, 4, 64))):
            for path in (AUTO, FUSED, SPLIT):
                p = plan_of(lib, B, dims, M, ns, nsteps=7, nout=3, path=path)
                what = (dims, M, ns, B, path)
                if path == FUSED and not lib.plan_ldr_fusable(M):
                    assert p.refused and p.msg.decode() == \
                        f"{FN}: the fused path needs ({lib.SUB} / M) * M >= {lib.FUSE_MIN_COLS} columns of a tile " \
                        f"(M = {M})", what
                    continue
                assert not p.refused, (what, p.msg)
                check_plan(lib, p, B, dims, M, ns, 7, 3, path, what)
                if p.path == FUSED:
                    fused_m.add(M)
                count += 1
    assert count > 10000
    # the rule the plan states: fused while at most a quarter of a sub-tile idles
    assert fused_m == {M for M in range(1, 17) if (16 // M) * M >= lib.FUSE_MIN_COLS}
    assert {1, 2, 3, 5, 16} <= fused_m and not {9, 17, 32} & fused_m


def test_every_refusal_carries_its_message(plan):
    lib = plan
    base = dict(B=1, dims=(5, 4), M=3, ns=2, nsteps=5, nout=2, path=AUTO)
    for kw, msg in ((dict(dims=()), "ndim=0 outside [1, 3]"), (dict(dims=(2, 2, 2, 2)), "ndim=4 outside [1, 3]"),
                    (dict(ns=0), "ns=0, M=3 outside 1 <= ns <= M <= 32"),
                    (dict(ns=4), "ns=4, M=3 outside 1 <= ns <= M <= 32"),
                    (dict(M=33, ns=2), "ns=2, M=33 outside 1 <= ns <= M <= 32"),
                    (dict(M=0, ns=0), "ns=0, M=0 outside 1 <= ns <= M <= 32"),
                    (dict(B=0), "B=0 must be at least 1"), (dict(B=-2), "B=-2 must be at least 1"),
                    (dict(dims=(5, 0)), "dims[1]=0 outside [1, 4096]"),
                    (dict(dims=(4097,)), "dims[0]=4097 outside [1, 4096]"),
                    (dict(dims=(-1, 3)), "dims[0]=-1 outside [1, 4096]"),
                    (dict(dims=(4096, 4096, 64), M=2), "B * npts * M must stay below 2^31"),
                    (dict(B=2 ** 31, dims=(1,), M=1, ns=1), "B * npts * M must stay below 2^31"),
                    (dict(B=2 ** 29, dims=(2,), M=2), "B * npts * M must stay below 2^31"),
                    (dict(nsteps=-1), "nsteps=-1 must not be negative and nout=2 at least 1"),
                    (dict(nout=0), "nsteps=5 must not be negative and nout=0 at least 1"),
                    (dict(path=-1), "path=-1 outside [0, 2]"), (dict(path=3), "path=3 outside [0, 2]"),
                    (dict(M=17, path=FUSED), "the fused path needs (16 / M) * M >= 12 columns of a tile (M = 17)"),
                    (dict(M=9, path=FUSED), "the fused path needs (16 / M) * M >= 12 columns of a tile (M = 9)")):
        args = dict(base)
        args.update(kw)
        p = plan_of(lib, **args)
        assert p.refused and p.msg.decode() == f"{FN}: {msg}", (kw, p.msg)
    p = LdrPlan()
    lib.plan_ldr(FN.encode(), 1, 2, None, 2, 2, 1, 1, 0, ctypes.byref(p))
    assert p.refused and p.msg.decode() == f"{FN}: null dims"
    # admitted at the edges: the largest index product, the longest axis, no steps
    assert lib.MAX_N == 4096 and lib.INDEX_MAX == 2 ** 31 - 1
    assert not plan_of(lib, 1, (4096, 4096, 127), 1, 1).refused
    assert plan_of(lib, 1, (4096, 4096, 128), 1, 1).refused
    assert not plan_of(lib, 2 ** 31 - 1, (1,), 1, 1).refused
    q = plan_of(lib, 1, (5, 4), 3, 2, nsteps=0, nout=1)
    assert not q.refused and (q.nsnap, q.nrun) == (0, 0)
    q = plan_of(lib, 1, (5, 4), 3, 2, nsteps=7, nout=3)
    assert (q.nsnap, q.nrun) == (2, 6)


def test_c_entry_checks_come_before_any_device_work():
    """qd_ldr_run refuses what the plan refuses and every null pointer it needs, with no GPU in the machine."""
    from pyqed_amd import _lib
    lib = _lib.load()
    dims = (ctypes.c_int * 2)(5, 4)
    buf = ctypes.create_string_buffer(16 * 5 * 4 * 3 * 2)   # stands for every array: never read, the call is refused
    a = ctypes.addressof(buf)

    def call(psi=a, B=1, ndim=2, d=dims, M=3, ns=2, U=a, eV=a, eVh=a, K0=a, K1=a, K2=None, nsteps=2, nout=1, snap=a,
             path=0):
        rc = lib.qd_ldr_run(psi, B, ndim, d, M, ns, U, eV, eVh, K0, K1, K2, nsteps, nout, snap, path, None)
        return rc, _lib.last_error()

    for kw, msg in ((dict(psi=None), "qd_ldr_run: null psi, U, expV or expVh"),
                    (dict(U=None), "qd_ldr_run: null psi, U, expV or expVh"),
                    (dict(eV=None), "qd_ldr_run: null psi, U, expV or expVh"),
                    (dict(eVh=None), "qd_ldr_run: null psi, U, expV or expVh"),
                    (dict(K1=None), "qd_ldr_run: null K1 with ndim=2"),
                    (dict(K0=None), "qd_ldr_run: null K0 with ndim=2"),
                    (dict(snap=None), "qd_ldr_run: null snap with 2 snapshots due"),
                    (dict(d=None), "qd_ldr_run: null dims"),
                    (dict(ndim=4), "qd_ldr_run: ndim=4 outside [1, 3]"),
                    (dict(M=33), "qd_ldr_run: ns=2, M=33 outside 1 <= ns <= M <= 32"),
                    (dict(ns=4), "qd_ldr_run: ns=4, M=3 outside 1 <= ns <= M <= 32"),
                    (dict(B=0), "qd_ldr_run: B=0 must be at least 1"),
                    (dict(nout=0), "qd_ldr_run: nsteps=2 must not be negative and nout=0 at least 1"),
                    (dict(path=5), "qd_ldr_run: path=5 outside [0, 2]"),
                    (dict(M=17, path=1),
                     "qd_ldr_run: the fused path needs (16 / M) * M >= 12 columns of a tile (M = 17)")):
        rc, err = call(**kw)
        assert rc == _lib.QD_EINVAL and err == msg, (kw, rc, err)
    # no snapshot due: nothing to compute, and no snapshot buffer needed
    assert call(nsteps=1, nout=2, snap=None)[0] == _lib.QD_OK
    assert call(nsteps=0, snap=None)[0] == _lib.QD_OK



def test_gpu_probe_lengths_straddle_every_tile_edge(plan):
    """The axis lengths the GPU kernel tests run (ldr_models.PROBE_LENGTHS, fixed there so that those tests need no
    host compile) against the plan's constants: one value on each side of every K-tile, row-tile and MFMA-tile edge up
    to four K-tiles, more than two row tiles, and lengths of many K-tiles."""
    from ldr_models import PROBE_LENGTHS
    lib = plan
    for edge in (lib.SUB, lib.KT, 2 * lib.KT, lib.RT, 3 * lib.KT, 4 * lib.KT, 2 * lib.RT):
        assert edge - 1 in PROBE_LENGTHS and edge + 1 in PROBE_LENGTHS, edge
    assert {1, 3, 15, 16, 17, 63, 64, 65} <= set(PROBE_LENGTHS)
    assert {-(-n // lib.RT) for n in PROBE_LENGTHS} >= {1, 2, 3, 5, 17}
    assert max(PROBE_LENGTHS) > 1024 and max(PROBE_LENGTHS) // lib.KT >= 32 and max(PROBE_LENGTHS) <= lib.MAX_N
