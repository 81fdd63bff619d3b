"""The launch plan of qd_ldr_jacobi_run (pyqed_amd/csrc/ldr_plan.hpp ldr_jacobi_plan) on the host, compiled with the
host C++ compiler through tools/cpu_emu/ldr_plan_c.cpp.  Nothing of the rules is restated here: the tests enumerate
shapes and check the pass order (forward on the last axis, the plain axes in order, back on the last axis) and roles,
that every planned launch is legal, that the row tiles, K-tiles and column sub-tiles of every pass cover every index
exactly once, that no point straddles two sub-tiles of the projecting pass, that the LDS is within its limit and as
large as its use, that no pass reads the buffer it writes, that the buffers chain, that the scratch parts do not
overlap, and that every refusal carries its message."""
import ctypes
import itertools
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

EMU_DIR = os.path.join(ROOT, "tools", "cpu_emu")
GRID_X_MAX, GRID_YZ_MAX = 2 ** 31 - 1, 65535
FN = "qd_ldr_jacobi_run"
AUTO, FUSED, SPLIT = 0, 1, 2
BUF_PSI, BUF_W0, BUF_W1 = 0, 1, 2
MAX_PASS = 4


class LdrLaunch(ctypes.Structure):
    _fields_ = [(n, ctypes.c_uint) for n in ("gx", "gy", "gz")] + [("tpb", ctypes.c_int), ("lds", ctypes.c_size_t)]


class JacobiPass(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int) for n in ("axis", "real", "expand", "phase", "project", "n", "ktiles", "cu", "src",
                                            "dst")] + \
               [(n, ctypes.c_uint) for n in ("s", "st", "outer", "C")] + [("launch", LdrLaunch)]


class JacobiPlan(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int) for n in ("refused", "path", "ndim", "M", "ns", "B")] + \
               [("n", ctypes.c_int * 3), ("npts", ctypes.c_long), ("nsnap", ctypes.c_int), ("nrun", ctypes.c_int),
                ("npass", ctypes.c_int), ("passes", JacobiPass * MAX_PASS), ("expand_dst", ctypes.c_int),
                ("project_src", ctypes.c_int)] + \
               [(n, LdrLaunch) for n in ("open", "expand", "project")] + \
               [(n, ctypes.c_size_t) for n in ("ws_psi0", "ws_psi1", "ws_w0", "ws_w1", "ws_total")] + \
               [("msg", ctypes.c_char * 200)]


CONSTANTS = ("MAX_DIM", "MAX_M", "MAX_N", "WAVES", "TPB", "SUB", "RT", "NSUB", "CT", "KT", "BS_STRIDE", "DS_STRIDE",
             "FUSE_MIN_COLS", "POINT_GRID_MAX", "INDEX_MAX", "LDS_MAX")


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "c++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    so = os.path.join(str(tmp_path_factory.mktemp("jplan")), "libldr_plan.so")
    subprocess.run([cxx, "-std=c++17", "-O1", "-shared", "-fPIC", "-Wall", "-Werror",
                    os.path.join(EMU_DIR, "ldr_plan_c.cpp"), "-o", so], check=True)
    lib = ctypes.CDLL(so)
    lib.plan_ldr_jacobi.restype = None
    lib.plan_ldr_jacobi.argtypes = [ctypes.c_char_p, ctypes.c_long, ctypes.c_int, ctypes.c_void_p, ctypes.c_int,
                                    ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(JacobiPlan)]
    lib.plan_ldr_constants.restype = None
    c = (ctypes.c_long * len(CONSTANTS))()
    lib.plan_ldr_constants(c)
    for name, v in zip(CONSTANTS, c):
        setattr(lib, name, int(v))
    assert lib.plan_ldr_jacobi_max_pass() == MAX_PASS == lib.MAX_DIM + 1
    assert lib.SUB == 16 and lib.KT % 4 == 0 and lib.LDS_MAX <= 64 * 1024
    return lib


def plan_of(lib, B, dims, M, ns, nsteps=5, nout=2, path=AUTO, fn=FN):
    p = JacobiPlan()
    d = None if dims is None else (ctypes.c_int * max(1, len(dims)))(*dims)
    lib.plan_ldr_jacobi(fn.encode(), B, 0 if dims is None else len(dims), d, M, ns, nsteps, nout, path,
                        ctypes.byref(p))
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
    # the pass list: forward on the last axis, the plain axes in order, back on the last axis
    assert p.npass == ndim + 1, what
    assert [p.passes[i].axis for i in range(p.npass)] == [ndim - 1] + list(range(ndim - 1)) + [ndim - 1], what
    prev_dst = BUF_PSI if fused else p.expand_dst
    for i in range(p.npass):
        a = p.passes[i]
        fwd, back = i == 0, i == p.npass - 1
        n = dims[a.axis]
        s = 1
        for m in dims[a.axis + 1:]:
            s *= m
        assert (a.real, a.phase) == (int(fwd or back), int(fwd)), (what, i)
        assert (a.expand, a.project) == (int(fused and fwd), int(fused and back)), (what, i)
        assert (a.n, a.s, a.st, a.outer, a.C) == (n, s, s * M, npts // (n * s), B * npts * M // n), (what, i)
        if a.real:
            # the real kernel is written for the last axis: columns (o, mu), the phase row inside a point block
            assert a.s == 1 and a.st == M and a.outer * n == npts, (what, i)
        check_launch(a.launch, (what, i), lib.LDS_MAX)
        assert a.launch.tpb == lib.TPB and (a.launch.gy - 1) * lib.RT < n <= a.launch.gy * lib.RT, (what, i)
        assert (a.ktiles - 1) * lib.KT < n <= a.ktiles * lib.KT, (what, i)
        assert 1 <= a.cu <= lib.SUB, (what, i)
        per_wg = lib.NSUB * a.cu
        assert (a.launch.gx - 1) * per_wg < a.C <= a.launch.gx * per_wg, (what, i)
        need = lib.KT * lib.BS_STRIDE * 16
        if a.project:
            assert a.cu == lib.plan_ldr_fusable(M) >= lib.FUSE_MIN_COLS and a.cu % M == 0 and a.C % M == 0, (what, i)
            need += lib.WAVES * lib.SUB * lib.DS_STRIDE * 16
        else:
            assert a.cu == lib.SUB, (what, i)
        assert need <= a.launch.lds <= lib.LDS_MAX, (what, i)
        # the buffers chain, and no pass reads what it writes (psi -> psi' are the step's own two states)
        assert a.src == prev_dst and a.src != a.dst, (what, i)
        assert a.src in (BUF_PSI, BUF_W0, BUF_W1) and a.dst in (BUF_PSI, BUF_W0, BUF_W1), (what, i)
        assert (a.src == BUF_PSI) == bool(a.expand) and (a.dst == BUF_PSI) == bool(a.project), (what, i)
        prev_dst = a.dst
    assert prev_dst == (BUF_PSI if fused else p.project_src), what
    if not fused:
        assert p.expand_dst in (BUF_W0, BUF_W1) and p.project_src in (BUF_W0, BUF_W1), what
    for l, elems in ((p.open, B * npts * ns), (p.expand, B * npts * M), (p.project, B * npts * ns)):
        check_launch(l, what, 0)
        assert l.gx <= lib.POINT_GRID_MAX and (l.gx == lib.POINT_GRID_MAX or l.gx * l.tpb >= elems), what
    # scratch: two states, two work arrays, in order and without overlap
    offs = (p.ws_psi0, p.ws_psi1, p.ws_w0, p.ws_w1, p.ws_total)
    need = (B * npts * ns * 16,) * 2 + (B * npts * M * 16,) * 2
    assert offs[0] == 0 and all(o % 256 == 0 for o in offs), what
    assert all(b - a >= n for a, b, n in zip(offs, offs[1:], need)), (what, offs, need)


def shapes_with(n):
    """The probed length as the transformed (last) axis and as each plain axis, in one to three dimensions."""
    return [(n,), (n, 3), (3, n), (n, 3, 4), (3, n, 4), (3, 4, n)]


def test_plans_are_legal_and_cover(plan):
    lib = plan
    pairs = [(1, 1), (2, 2), (3, 2), (5, 3), (9, 4), (16, 3), (17, 2), (32, 32)]
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
    count, fused_m = 0, set()
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
    # the fused / split rule is qd_ldr_run's
    assert fused_m == {M for M in range(1, 17) if (16 // M) * M >= lib.FUSE_MIN_COLS}
    assert {1, 2, 3, 5, 16} <= fused_m and not {9, 17, 32} & fused_m


def test_one_dimension_is_the_two_real_passes(plan):
    for path, chain in ((FUSED, [(BUF_PSI, BUF_W0), (BUF_W0, BUF_PSI)]), (SPLIT, [(BUF_W0, BUF_W1), (BUF_W1, BUF_W0)])):
        p = plan_of(plan, 3, (33,), 3, 2, path=path)
        assert not p.refused and p.npass == 2
        assert [(p.passes[i].real, p.passes[i].phase, p.passes[i].axis) for i in range(2)] == [(1, 1, 0), (1, 0, 0)]
        assert [(p.passes[i].src, p.passes[i].dst) for i in range(2)] == chain


def test_every_refusal_carries_its_message(plan):
    lib = plan
    base = dict(B=1, dims=(5, 4), M=3, ns=2, nsteps=5, nout=2, path=AUTO)
    for kw, msg in ((dict(dims=()), "ndim=0 outside [1, 3]"), (dict(dims=(2, 2, 2, 2)), "ndim=4 outside [1, 3]"),
                    (dict(ns=0), "ns=0, M=3 outside 1 <= ns <= M <= 32"),
                    (dict(ns=4), "ns=4, M=3 outside 1 <= ns <= M <= 32"),
                    (dict(M=33, ns=2), "ns=2, M=33 outside 1 <= ns <= M <= 32"),
                    (dict(B=0), "B=0 must be at least 1"), (dict(B=-2), "B=-2 must be at least 1"),
                    (dict(dims=(5, 0)), "dims[1]=0 outside [1, 4096]"),
                    (dict(dims=(4097,)), "dims[0]=4097 outside [1, 4096]"),
                    (dict(dims=(4096, 4096, 64), M=2), "B * npts * M must stay below 2^31"),
                    (dict(B=2 ** 31, dims=(1,), M=1, ns=1), "B * npts * M must stay below 2^31"),
                    (dict(nsteps=-1), "nsteps=-1 must not be negative and nout=2 at least 1"),
                    (dict(nout=0), "nsteps=5 must not be negative and nout=0 at least 1"),
                    (dict(path=-1), "path=-1 outside [0, 2]"), (dict(path=3), "path=3 outside [0, 2]"),
                    (dict(M=17, path=FUSED), "the fused path needs (16 / M) * M >= 12 columns of a tile (M = 17)"),
                    (dict(M=9, ns=4, path=FUSED), "the fused path needs (16 / M) * M >= 12 columns of a tile (M = 9)")):
        args = dict(base)
        args.update(kw)
        p = plan_of(lib, **args)
        assert p.refused and p.msg.decode() == f"{FN}: {msg}", (kw, p.msg)
    p = JacobiPlan()
    lib.plan_ldr_jacobi(FN.encode(), 1, 2, None, 2, 2, 1, 1, 0, ctypes.byref(p))
    assert p.refused and p.msg.decode() == f"{FN}: null dims"
    # admitted at the edges: the largest index product, the longest axis, no steps
    assert not plan_of(lib, 1, (4096, 4096, 127), 1, 1).refused
    assert plan_of(lib, 1, (4096, 4096, 128), 1, 1).refused
    q = plan_of(lib, 1, (5, 4), 3, 2, nsteps=0, nout=1)
    assert not q.refused and (q.nsnap, q.nrun) == (0, 0)
    q = plan_of(lib, 1, (5, 4), 3, 2, nsteps=7, nout=3)
    assert (q.nsnap, q.nrun) == (2, 6)


def test_gpu_probe_lengths_straddle_every_tile_edge(plan):
    """The axis lengths the GPU kernel tests run (ldr_models.PROBE_LENGTHS) against this plan's constants: one value on
    each side of every K-tile, row-tile and MFMA-tile edge up to four K-tiles and two row tiles, and the plan of each
    takes the tile counts those edges stand for, on the transformed axis as on a plain one."""
    from ldr_models import PROBE_LENGTHS
    lib = plan
    for edge in (lib.SUB, lib.KT, 2 * lib.KT, lib.RT, 3 * lib.KT, 4 * lib.KT, 2 * lib.RT):
        assert edge - 1 in PROBE_LENGTHS and edge + 1 in PROBE_LENGTHS, edge
    seen = set()
    for n in (m for m in PROBE_LENGTHS if m <= 129):
        p = plan_of(lib, 1, (3, n), 2, 2)
        q = plan_of(lib, 1, (n, 3), 2, 2)
        assert p.passes[0].ktiles == p.passes[2].ktiles == q.passes[1].ktiles == -(-n // lib.KT)
        assert p.passes[0].launch.gy == q.passes[1].launch.gy == -(-n // lib.RT)
        seen.add((p.passes[0].ktiles, p.passes[0].launch.gy))
    assert {k for k, _ in seen} >= {1, 2, 3, 4, 5} and {r for _, r in seen} >= {1, 2, 3}
