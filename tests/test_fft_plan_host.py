"""The decisions of the any-size FFT engine (pyqed_amd/csrc/fft_plan.hpp) on the host: the axis plan, the four-step
split, the plan of an fft_lines call, the tile of a fused pass, the 2D layout and the step sequence, compiled with the
host C++ compiler through tools/cpu_emu/fft_plan_c.cpp.  Nothing of the rules is restated here: the tests enumerate,
check that what is planned is legal for the kernels that run it (spo_gen_kernels.hpp: lines of M slots in two LDS
buffers, 32-bit flat indices, a grid that covers the array), and compare what is reached with the tables written
below, so that a change to a tiling rule shows as a diff.  tests/test_fft_engine_host.py and test_spo_gen_host.py run
the same plans through the emulated kernels."""
import ctypes
import itertools
import os
import shutil
import subprocess

import pytest

import fft_cases as fc
from conftest import ROOT

EMU_DIR = os.path.join(ROOT, "tools", "cpu_emu")
MAX_ST, LDS_MAX, MAX_M, ELEM = 32, 160 * 1024, 5120, 16
MIXED, BLUESTEIN, DIRECT = range(3)
F_INV, F_PT1, F_SNAP, F_PT2, F_FWD, F_KY, F_KMUL = (1 << k for k in range(7))
U_NONE, U_HALF, U_FULL = range(3)
LMAX = 12288


class FDiv(ctypes.Structure):
    _fields_ = [(n, ctypes.c_uint) for n in "dms"]


class AxisPlan(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int) for n in ("L", "M", "kind", "nst")] + \
               [("R", ctypes.c_int * MAX_ST), ("Ns", ctypes.c_int * MAX_ST), ("dnb", FDiv * MAX_ST),
                ("dns", FDiv * MAX_ST), ("dM", FDiv)] + \
               [(n, ctypes.c_size_t) for n in ("slots", "tw", "chirp", "b", "bhat")] + [("refused", ctypes.c_bool)]


class LinesPlan(ctypes.Structure):
    _fields_ = [("O", ctypes.c_long), ("I", ctypes.c_long)] + \
               [(n, ctypes.c_int) for n in ("L", "kind", "L1", "L2", "l2")] + \
               [("ax", AxisPlan * 2), ("slots", ctypes.c_size_t), ("tw_l", ctypes.c_size_t), ("scratch", ctypes.c_bool)]


class PassPlan(ctypes.Structure):
    _fields_ = [("fused", ctypes.c_bool)] + [(n, ctypes.c_int) for n in ("C", "G", "twl")] + \
               [("lds", ctypes.c_size_t), ("gx", ctypes.c_long), ("gy", ctypes.c_long)] + \
               [(n, FDiv) for n in ("dLC", "dC", "dLns", "dns")]


class NdLayout(ctypes.Structure):
    _fields_ = [("xpose", ctypes.c_bool), ("row", PassPlan), ("kin", PassPlan)]


class StepPass(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int) for n in ("axis", "flags", "u1", "u2", "rec")]


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "c++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    so = str(tmp_path_factory.mktemp("plan") / "libfft_plan.so")
    subprocess.run([cxx, "-std=c++17", "-O1", "-shared", "-fPIC", "-Wall", "-Werror",
                    os.path.join(EMU_DIR, "fft_plan_c.cpp"), "-o", so], check=True)
    lib = ctypes.CDLL(so)
    for f in (lib.plan_fft_axis, lib.plan_fft_lines, lib.plan_fft_pass, lib.plan_nd_layout, lib.plan_fdiv):
        f.restype = None
    lib.plan_fft_lines.argtypes = [ctypes.c_long, ctypes.c_int, ctypes.c_long, ctypes.c_void_p]
    lib.plan_fft_pass.argtypes = [ctypes.c_void_p, ctypes.c_long, ctypes.c_long, ctypes.c_int, ctypes.c_int,
                                  ctypes.c_void_p]
    lib.plan_fdiv.argtypes = [ctypes.c_uint, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    return lib


@pytest.fixture(scope="module")
def axes(plan):
    """The axis plan of every length 1..12288, computed once."""
    out = {}
    for L in range(1, LMAX + 1):
        out[L] = AxisPlan()
        plan.plan_fft_axis(L, ctypes.byref(out[L]))
    return out


def is_prime(n):
    return n >= 2 and all(n % p for p in range(2, int(n ** 0.5) + 1))


def smooth5(n):
    for p in (2, 3, 5):
        while n % p == 0:
            n //= p
    return n == 1


def axis_divisors(a):
    return {a.M} | {a.M // a.R[s] for s in range(a.nst)} | {a.Ns[s] for s in range(a.nst)}


def test_axis_plans(axes):
    kinds = [0, 0, 0]
    for L, a in axes.items():
        assert a.L == L and not a.refused and a.nst <= MAX_ST, L
        kinds[a.kind] += 1
        if a.kind == DIRECT:
            assert a.M == L and a.nst == 0, L
        else:   # the stages are an M-point Stockham transform that two LDS buffers hold
            assert a.M <= MAX_M, L
            run = 1
            for s in range(a.nst):
                assert a.Ns[s] == run, (L, s)
                assert a.R[s] in (2, 3, 4, 5, 8) or (is_prime(a.R[s]) and a.R[s] <= 61), (L, s, a.R[s])
                assert (a.dnb[s].d, a.dns[s].d) == (a.M // a.R[s], a.Ns[s]), (L, s)
                run *= a.R[s]
            assert run == a.M and a.dM.d == a.M, L
        # the tables tile the slots: tw [M], and for Bluestein chirp [L], b [M], bhat [M]
        tables = [(a.tw, a.M)]
        if a.kind == BLUESTEIN:
            assert a.M >= 2 * L - 1 and smooth5(a.M), L
            tables += [(a.chirp, L), (a.b, a.M), (a.bhat, a.M)]
        else:
            assert a.M == L, L
        end = 0
        for off, n in sorted(tables):
            assert off == end, (L, tables)
            end += n
        assert a.slots == end, L
    print("axis plans 1..%d: %d mixed, %d Bluestein, %d direct" % ((LMAX,) + tuple(kinds)))
    assert sum(kinds) == LMAX and all(kinds)


def lines_class(p):
    return "fourstep" if p.L1 else ("mixed", "bluestein", "direct")[p.kind]


def test_plan_classes_of_the_conformance_lengths(plan):
    """Each length of fft_cases.CLASSES runs the plan it is filed under (8192, the last power of two, is a four-step
    length, as the comment there says)."""
    p = LinesPlan()
    for cls, lengths in fc.CLASSES.items():
        for n in lengths:
            plan.plan_fft_lines(2, n, 3, ctypes.byref(p))
            want = cls if cls in ("bluestein", "direct", "fourstep") else "fourstep" if n == 8192 else "mixed"
            assert lines_class(p) == want, (cls, n, lines_class(p))


def test_lines_plans(plan, axes):
    p = LinesPlan()
    for L in range(1, LMAX + 1):
        plan.plan_fft_lines(3, L, 5, ctypes.byref(p))
        assert (p.O, p.L, p.I, p.kind) == (3, L, 5, axes[L].kind), L
        if p.L1:   # both factors LDS plans, the more balanced one first, the L-point twiddles behind their tables
            a1, a2 = p.ax
            assert p.kind == DIRECT and p.L1 * p.L2 == L and 2 <= p.L1 <= p.L2 == p.l2, L
            assert (a1.L, a2.L) == (p.L1, p.L2) and DIRECT not in (a1.kind, a2.kind), L
            assert p.tw_l == a1.slots + a2.slots and p.slots == p.tw_l + L and not p.scratch, L
        else:
            assert p.l2 == 0 and p.L2 == 0 and p.ax[0].L == L and p.slots == axes[L].slots, L
            assert p.scratch == (p.kind == DIRECT), L


@pytest.mark.parametrize("n,l2", [(5120, 0), (2557, 0), (2579, 0), (5158, 0), (7919, 0), (8192, 128), (5121, 569),
                                  (6499, 97), (5114, 2557), (10201, 101), (12288, 128), (5125, 125), (6000, 80)])
def test_fourstep_split_of_fft_lines(plan, n, l2):
    """The pairs of test_fft_engine_host.py::test_emulated_engine_fourstep_split, straight from the plan."""
    p = LinesPlan()
    plan.plan_fft_lines(1, n, 1, ctypes.byref(p))
    assert p.l2 == l2 and (p.kind == DIRECT or not l2)
    if p.kind == DIRECT:
        assert plan.plan_fourstep_split(n, 1) == p.L1 == (n // l2 if l2 else 0)


def test_fourstep_split_of_the_1d_run(plan):
    """Both factors mixed-radix: 6000 = 75 x 80 splits, 5121 = 9 x 569 (569 a Bluestein length) does not."""
    assert plan.plan_fourstep_split(6000, 0) == 75
    assert plan.plan_fourstep_split(5121, 0) == 0 and plan.plan_fourstep_split(5121, 1) == 9


PASS_LENGTHS = fc.SHAPE_LENGTHS + [509, 2557, 5120]
ROW_NS = (1, 2, 3, 9, 32)
ROW_O = sorted({o for o, _ in fc.SHAPES})


def pass_cases():
    """(L, O, I, ns, rows): the column-tile passes of fft_lines over fft_cases.SHAPES, and whole-row passes."""
    for L in PASS_LENGTHS:
        for o, i in fc.SHAPES:
            yield L, o, i, i, 0
        for o in ROW_O:
            for ns in ROW_NS:
                yield L, o, ns, ns, 1


def pass_divisors(L, t, ns):
    return {L * t.C, t.C, L * ns, ns}


def pass_values(t):
    return (t.fused, t.C, t.G, t.twl, t.lds, t.gx, t.gy) + tuple((d.d, d.m, d.s) for d in (t.dLC, t.dC, t.dLns, t.dns))


def test_fdiv_is_exact(plan, axes):
    """fdiv(x, make_fdiv(d)) == x // d for every divisor the plans form over these enumerations."""
    ds = {1, 2, 3, 2 ** 31 - 1, 2 ** 31}
    for a in axes.values():
        ds |= axis_divisors(a)
    t = PassPlan()
    for L, o, i, ns, rows in pass_cases():
        plan.plan_fft_pass(ctypes.byref(axes[L]), o, i, ns, rows, ctypes.byref(t))
        if t.fused:
            ds |= pass_divisors(L, t, ns) | {o}   # o: nlo of a pass that stores into the other layout
    top = 2 ** 32 - 1
    for d in sorted(ds):
        xs = sorted({0, top} | {k * d + e for k in (1, 2, top // d) for e in (-1, 0, 1) if 0 <= k * d + e <= top})
        arr = (ctypes.c_uint * len(xs))(*xs)
        out = (ctypes.c_uint * len(xs))()
        plan.plan_fdiv(d, arr, len(xs), out)
        assert list(out) == [x // d for x in xs], d
    print("fdiv: %d divisors, largest below 2^31 - 1: %d" % (len(ds), sorted(ds)[-3]))


# What the pass plans reach, per axis length: its kind; (C, G) of the column-tile pass at each of fft_cases.SHAPES;
# and per outer count of ROW_O the whole-row pass at each ns of ROW_NS, (C, G) or None where the row does not fit the
# LDS and the pass runs unfused.
_ONE = [(1, 1)] * 9
_NO = None
PASS_TABLE = {
    12: (MIXED, [(1, 1), (1, 1), (1, 1), (1, 1), (1, 1), (1, 2), (2, 2), (3, 4), (8, 1)], {
        1: [(1, 1), (2, 1), (3, 1), (9, 1), (32, 1)],
        2: [(1, 1), (2, 1), (3, 1), (9, 1), (32, 1)],
        3: [(1, 1), (2, 1), (3, 1), (9, 1), (32, 1)],
        5: [(1, 1), (2, 1), (3, 1), (9, 1), (32, 1)],
        90: [(1, 1), (2, 1), (3, 1), (9, 1), (32, 1)],
        601: [(1, 2), (2, 2), (3, 2), (9, 2), (32, 1)],
        1025: [(1, 4), (2, 4), (3, 4), (9, 4), (32, 1)],
    }),
    61: (MIXED, [(1, 1), (1, 1), (1, 1), (1, 1), (1, 1), (1, 2), (2, 2), (3, 2), (8, 1)], {
        1: [(1, 1), (2, 1), (3, 1), (9, 1), (32, 1)],
        2: [(1, 1), (2, 1), (3, 1), (9, 1), (32, 1)],
        3: [(1, 1), (2, 1), (3, 1), (9, 1), (32, 1)],
        5: [(1, 1), (2, 1), (3, 1), (9, 1), (32, 1)],
        90: [(1, 1), (2, 1), (3, 1), (9, 1), (32, 1)],
        601: [(1, 2), (2, 2), (3, 2), (9, 1), (32, 1)],
        1025: [(1, 4), (2, 4), (3, 2), (9, 1), (32, 1)],
    }),
    67: (BLUESTEIN, [(1, 1), (1, 1), (1, 1), (1, 1), (1, 1), (1, 2), (2, 2), (3, 2), (8, 1)], {
        1: [(1, 1), (2, 1), (3, 1), (9, 1), (32, 1)],
        2: [(1, 1), (2, 1), (3, 1), (9, 1), (32, 1)],
        3: [(1, 1), (2, 1), (3, 1), (9, 1), (32, 1)],
        5: [(1, 1), (2, 1), (3, 1), (9, 1), (32, 1)],
        90: [(1, 1), (2, 1), (3, 1), (9, 1), (32, 1)],
        601: [(1, 2), (2, 2), (3, 2), (9, 1), (32, 1)],
        1025: [(1, 4), (2, 2), (3, 2), (9, 1), (32, 1)],
    }),
    200: (MIXED, [(1, 1), (1, 1), (1, 1), (1, 1), (1, 1), (1, 2), (2, 1), (3, 1), (8, 1)], {
        1: [(1, 1), (2, 1), (3, 1), (9, 1), _NO],
        2: [(1, 1), (2, 1), (3, 1), (9, 1), _NO],
        3: [(1, 1), (2, 1), (3, 1), (9, 1), _NO],
        5: [(1, 1), (2, 1), (3, 1), (9, 1), _NO],
        90: [(1, 1), (2, 1), (3, 1), (9, 1), _NO],
        601: [(1, 2), (2, 1), (3, 1), (9, 1), _NO],
        1025: [(1, 2), (2, 1), (3, 1), (9, 1), _NO],
    }),
    1024: (MIXED, [(1, 1), (1, 1), (1, 1), (1, 1), (1, 1), (1, 1), (2, 1), (1, 1), (2, 1)],
           {o: [(1, 1), (2, 1), (3, 1), _NO, _NO] for o in ROW_O}),
    509: (BLUESTEIN, [(1, 1), (1, 1), (1, 1), (1, 1), (1, 1), (1, 1), (2, 1), (1, 1), (2, 1)],
          {o: [(1, 1), (2, 1), (3, 1), _NO, _NO] for o in ROW_O}),
    2557: (BLUESTEIN, _ONE, {o: [(1, 1), _NO, _NO, _NO, _NO] for o in ROW_O}),
    5120: (MIXED, _ONE, {o: [(1, 1), _NO, _NO, _NO, _NO] for o in ROW_O}),
}


def test_pass_plans(plan, axes):
    reached, t, max_gy = {}, PassPlan(), 0
    for L, o, i, ns, rows in pass_cases():
        a = axes[L]
        what = (L, o, i, ns, rows)
        plan.plan_fft_pass(ctypes.byref(a), o, i, ns, rows, ctypes.byref(t))
        entry = reached.setdefault(L, (a.kind, [], {}))
        if rows:
            entry[2].setdefault(o, []).append((t.C, t.G) if t.fused else None)
        else:
            assert t.fused, what   # a column tile narrows to one line, which every LDS plan holds
            entry[1].append((t.C, t.G))
        if not t.fused:
            assert rows and 2 * i * a.M * ELEM > LDS_MAX, what
            continue
        C, G, M = t.C, t.G, a.M
        assert 1 <= C <= i and G >= 1 and (not rows or C == i), what
        lines = 2 * G * C * M * ELEM
        assert t.twl == (lines + M * ELEM <= LDS_MAX) and t.lds == lines + t.twl * M * ELEM <= LDS_MAX, what
        assert G * C * M < 2 ** 31 and G * L * C < 2 ** 31, what
        assert t.gx * G >= o > (t.gx - 1) * G and t.gy * C >= i > (t.gy - 1) * C, what
        assert G == 1 or C == i, what
        assert (t.dLC.d, t.dC.d, t.dLns.d, t.dns.d) == (L * C, C, L * ns, ns), what
        max_gy = max(max_gy, t.gy)
    print("pass plans: largest grid y", max_gy)
    assert reached == PASS_TABLE, {L: v for L, v in reached.items() if PASS_TABLE.get(L) != v}


@pytest.mark.parametrize("O,L,I,gy", [(1, 12, 10 ** 6, 125_000), (4, 100, 524_288, 65_536)])
def test_column_tile_grid_y_extent(plan, axes, O, L, I, gy):
    """A finding, recorded and not judged: shapes qd_fft_axis admits (O L I < 2^31) whose column tile has a grid y
    beyond 65535.  Whether the runtime takes such a launch has not been measured."""
    t = PassPlan()
    plan.plan_fft_pass(ctypes.byref(axes[L]), O, I, I, 0, ctypes.byref(t))
    print("column tile of (O, L, I) = (%d, %d, %d): C %d, grid y %d" % (O, L, I, t.C, t.gy))
    assert O * L * I < 2 ** 31 and t.fused and t.gy == gy and t.gy * t.C >= I > (t.gy - 1) * t.C


def test_nd_layout(plan):
    """Alternating layouts exactly for 2D grids of one step or more whose whole rows fit on both axes; their two
    passes are the whole-row plans of those shapes."""
    lay, t, a = NdLayout(), PassPlan(), AxisPlan()
    for (n0, n1), ns, nsteps in itertools.product(((20, 20), (96, 80), (67, 45), (12, 10), (6, 600), (600, 6),
                                                   (2579, 12), (12, 2579), (1000, 1000), (3, 5120)),
                                                  (1, 2, 9, 32), (0, 1, 4)):
        dims = (ctypes.c_int * 2)(n0, n1)
        plan.plan_nd_layout(dims, 2, ns, nsteps, ctypes.byref(lay))
        fits = []
        for L, o, got in ((n1, n0, lay.row), (n0, n1, lay.kin)):
            plan.plan_fft_axis(L, ctypes.byref(a))
            plan.plan_fft_pass(ctypes.byref(a), o, ns, ns, 1, ctypes.byref(t))
            fits.append(t.fused)
            if lay.xpose:
                assert pass_values(got) == pass_values(t), (n0, n1, ns, nsteps)
        assert lay.xpose == (nsteps >= 1 and all(fits)), (n0, n1, ns, nsteps)
    dims = (ctypes.c_int * 3)(24, 20, 18)
    plan.plan_nd_layout(dims, 3, 2, 4, ctypes.byref(lay))
    assert not lay.xpose


def step_passes(plan, D, nsteps, nout, snaps, merged, ky):
    out = (StepPass * 256)()
    n = plan.plan_step_sequence(D, nsteps, nout, snaps, merged, ky, out, 256)
    assert n <= 256
    return [out[k] for k in range(n)]


@pytest.mark.parametrize("D,nsteps,nout,merged,ky", itertools.product((2, 3), (0, 1, 2, 5), (1, 2), (0, 1), (0, 1)))
def test_step_sequence(plan, D, nsteps, nout, merged, ky):
    last = D - 1
    for snaps in (0, 1):
        kspace = [False] * D      # per axis: the state is in k-space along it
        ops, steps, recs = "", 0, []
        for p in step_passes(plan, D, nsteps, nout, snaps, merged, ky):
            f, d = p.flags, p.axis
            assert (f & (F_PT1 | F_PT2 | F_SNAP | F_KY)) == 0 or d == last, (d, f)
            assert not f & F_KMUL or (d == 0 and f == F_KMUL), (d, f)
            if f & F_INV:         # the kernel's order inside a pass: IFFT, U1, snapshot, U2, FFT, k_y, K
                assert kspace[d], (d, f)
                kspace[d] = False
            if f & (F_PT1 | F_PT2 | F_SNAP):   # point operators and snapshots see the state in real space
                assert not any(kspace), (d, f)
            if f & F_PT1:
                assert p.u1 in (U_HALF, U_FULL)
                ops += "H" if p.u1 == U_HALF else "F"
            if f & F_SNAP:        # after the step's first point operator, at every nout-th step
                assert f & F_PT1 and steps % nout == 0 and p.rec == steps // nout - 1, (steps, p.rec)
                recs.append(p.rec)
            else:
                assert p.rec == -1
            if f & F_PT2:
                assert p.u2 == U_HALF
                ops += "H"
            if f & F_FWD:
                assert not kspace[d], (d, f)
                kspace[d] = True
            assert bool(f & F_KY) == bool(ky and d == last and f & F_FWD), (d, f)
            if f & F_KMUL:        # FFT, K, IFFT along axis 0 with every other axis in k-space
                assert all(kspace[1:]) and not kspace[0], (d, f)
                ops += "K"
                steps += 1
        assert not any(kspace)
        assert recs == (list(range(nsteps // nout)) if snaps else [])
        if merged:   # wpd.py:736-755: V/2, nsteps x [K, V], K, V/2
            assert ops == "H" + "KF" * nsteps + "KH"
        else:        # wpd.py:723-730: both halves of every step
            assert ops.count("H") == 2 * nsteps and "F" not in ops and ops.count("K") == nsteps
            assert ops == ("H" + "KHH" * (nsteps - 1) + "KH" if nsteps else "")
