"""The dispatch of the DEOM launches (pyqed_amd/csrc/deom_plan.hpp) on the host: the stage plan and the band plan,
compiled with the host C++ compiler through tools/cpu_emu/deom_plan_c.cpp, over every kind of shape the entry points
accept.  Nothing of the rules is restated here: the tests enumerate, check that each planned launch is legal for the
kernel it names (what a kernel needs -- a lane per matrix element, a wave per ADO or tile, its rows in LDS -- is the
kernel's geometry, not a rule of the plan), that the typed dispatch reaches that kernel, and compare the set of
(name, template values) reached with the sets written below, which are the DEOM stage and band kernels that exist.
The anchors are the names the GPU tests assert on hardware at their shapes."""
import ctypes
import itertools
import math
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

EMU_DIR = os.path.join(ROOT, "tools", "cpu_emu")
LDS_MAX = 160 * 1024
GRID_MAX = 2 ** 31 - 1
ELEMENT, GROUP, GROUP_W5, PIPE, MFMA16, TILE, TMFMA = range(7)   # StageKind
STAGE_NEEDS_GROUP, STAGE_LANE_RANGE = 1, 2                       # StageRefusal
BAND_NS, BAND_K, BAND_LANES, BAND_LDS = 1, 2, 3, 4               # BandRefusal


class StagePlan(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int) for n in ("kind", "G", "KMAX", "NS2", "UNI", "HM", "NM", "tpb", "max_tpb",
                                            "resident")] + \
               [("grid", ctypes.c_long), ("lds", ctypes.c_size_t)] + \
               [(n, ctypes.c_int) for n in ("xsplit", "ntst", "bchunk", "refusal")] + \
               [("name", ctypes.c_char_p), ("msg", ctypes.c_char * 112)]


class BandPlan(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int) for n in ("G", "KMAX", "NS2", "FAST", "TPB", "tpb")] + \
               [("lds", ctypes.c_size_t), ("refusal", ctypes.c_int), ("name", ctypes.c_char_p),
                ("msg", ctypes.c_char * 112)]


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "c++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    so = str(tmp_path_factory.mktemp("plan") / "libdeom_plan.so")
    subprocess.run([cxx, "-std=c++17", "-O1", "-shared", "-fPIC", "-Wall", "-Werror",
                    os.path.join(EMU_DIR, "deom_plan_c.cpp"), "-o", so], check=True)
    lib = ctypes.CDLL(so)
    lib.plan_deom_stage.restype = lib.plan_deom_band.restype = None
    return lib


# Every stage kernel: (noted name, G, KMAX, NS2, UNI, HM, NM).  26 instantiations of the five templated families and
# the three kernels without template values.
STAGE_KERNELS = (
    {(n, 0, 0, 0, 0, 0, 0) for n in ("deom_element", "deom_tile", "deom_tmfma")} |
    {("deom_mfma16", 0, 0, 0, 0, 0, nm) for nm in (1, 2)} |
    {("deom_pipe_k%d" % k, 4, k, 0, 0, 0, 0) for k in (4, 5, 6)} |
    {("deom_grp4_w5", 4, 5, 1, 0, 1, 0)} |
    {("deom_grp", g, 8, 0, 0, 0, 0) for g in (1, 16, 32, 64)} |
    {("deom_grp4", 4, k, 1, 0, hm, 0) for k in (4, 5, 6, 8) for hm in (0, 1)} |
    {("deom_grp4_uniform", 4, k, 1, 1, hm, 0) for k in (4, 5, 6, 8) for hm in (0, 1)})
# Every band kernel: (noted name, G, KMAX, NS2, TPB, FAST): 15 instantiations.
BAND_KERNELS = {(n, g, k, ns2, t, f) for t in (256, 512, 1024) for n, g, k, ns2, f in (
    ("deom_banded_fast", 4, 5, 1, 1), ("deom_banded_fast", 4, 6, 1, 1), ("deom_banded", 4, 5, 1, 0),
    ("deom_banded", 4, 8, 1, 0), ("deom_banded_g16", 16, 8, 0, 0))}


def test_kernel_lists_have_the_size_of_the_library():
    """41 templated deom_*_kernel<...> instantiations in the device code, and three stage kernels without values."""
    assert len(STAGE_KERNELS) == 29 and len(BAND_KERNELS) == 15
    assert sum(1 for k in STAGE_KERNELS if any(k[1:])) + len(BAND_KERNELS) == 41


def stage_values(p):
    return (p.kind, p.G, p.KMAX, p.NS2, p.UNI, p.HM, p.NM)


def check_stage(lib, p, hit, B, nmax, K, ns, nmod, bminor, horner):
    """One accepted stage plan: a legal launch of a kernel that exists and covers the stage."""
    what = (B, nmax, K, ns, nmod, bminor, horner, p.name)
    kind, grid, tpb = p.kind, p.grid, p.tpb
    assert tpb % 64 == 0 and 64 <= tpb <= p.max_tpb <= 1024, what
    assert p.lds <= LDS_MAX and 1 <= grid <= GRID_MAX, what
    assert p.bchunk in (0, 16) and p.xsplit in (0, 8) and p.ntst in (0, 1), what
    rows = B * nmax
    if kind in (GROUP, GROUP_W5):
        assert p.G >= ns * ns and p.KMAX >= K, what           # a lane per matrix element, registers for K neighbours
        if p.xsplit:   # the grid is dealt to 8 block classes of B / xsplit hierarchies each
            assert B % p.xsplit == 0 and grid % 8 == 0 and (grid // 8) * tpb >= (rows // p.xsplit) * p.G, what
        else:
            assert grid * tpb >= rows * p.G, what
        if p.bchunk:
            assert bminor and p.xsplit and (B // p.xsplit) % p.bchunk == 0, what
        if p.UNI:
            assert p.G == 4 and bminor and p.xsplit > 0, what
        assert not p.HM or horner, what                        # compile-time Horner stages only for undriven runs
        assert kind == GROUP or p.HM == 1, what
    elif kind == PIPE:   # persistent: 8 classes x what is resident, the waves stride over their class
        assert p.resident == 1 and grid == 8 and tpb == 256 and p.xsplit == 8 and p.bchunk == 0, what
        assert p.G == 4 == ns * ns and p.KMAX >= K and horner and bminor, what
    elif kind == ELEMENT:
        assert grid * tpb >= rows * ns * ns, what
    elif kind == MFMA16:   # a wave per ADO, the matrix padded to 16 x 16
        assert grid * (tpb // 64) >= rows and ns <= 16 and p.NM >= nmod, what
    else:                  # 16 x 16 tiles: a workgroup each, or a wave each in 2 x 2 blocks
        nt = -(-ns // 16)
        assert kind in (TILE, TMFMA) and tpb == 256, what
        assert grid >= rows * (nt * nt if kind == TILE else (-(-nt // 2)) ** 2), what
    assert kind in (GROUP, GROUP_W5, PIPE) or not (bminor or p.xsplit or p.bchunk or p.resident), what
    assert lib.plan_deom_stage_hits(ctypes.byref(p), hit) == 1, what + ("dispatch miss",)
    assert tuple(hit) == stage_values(p), what


def test_stage_plans(plan):
    from pyqed_amd.deom import ado_major_ok
    reached, refused, p, hit = set(), set(), StagePlan(), (ctypes.c_int * 7)()
    ref, fn = ctypes.byref(p), plan.plan_deom_stage
    sizes = list(itertools.product((1, 7, 8, 16, 64, 72, 128, 256, 1024), (1, 24, 462, 1287, 6188, 2_000_000)))
    for ns, K, nmod, bminor, horner in itertools.product(range(1, 21), range(1, 23), range(1, 10), (0, 1), (0, 1)):
        for B, nmax in sizes:
            fn(B, nmax, K, ns, nmod, bminor, horner, ref)
            if p.refusal:   # by a stated rule, never a dispatch miss
                assert p.refusal in (STAGE_NEEDS_GROUP, STAGE_LANE_RANGE) and p.msg.startswith(b"qd_deom_rk4"), p.msg
                assert (p.refusal == STAGE_NEEDS_GROUP) == (bminor and not ado_major_ok(ns, K)), (ns, K, p.msg)
                refused.add(p.refusal)
                continue
            assert not bminor or ado_major_ok(ns, K), (ns, K)
            check_stage(plan, p, hit, B, nmax, K, ns, nmod, bminor, horner)
            reached.add((p.name.decode(),) + stage_values(p)[1:])
    assert reached == STAGE_KERNELS, (sorted(reached - STAGE_KERNELS), sorted(STAGE_KERNELS - reached))
    assert refused == {STAGE_NEEDS_GROUP, STAGE_LANE_RANGE}


def nado(L, K):
    return math.comb(L + K, K)


# What the GPU tests assert on hardware (tests/test_deom_gpu.py): (B, nmax, K, ns, nmod, ADO-major, undriven) -> name
ANCHORS = [
    ((64, 1287, 5, 2, 1, 1, 1), "deom_pipe_k5"), ((72, 1287, 5, 2, 1, 1, 1), "deom_pipe_k5"),
    ((64, 1365, 4, 2, 1, 1, 1), "deom_pipe_k4"), ((64, 1716, 6, 2, 1, 1, 1), "deom_pipe_k6"),
    ((64, 462, 5, 2, 1, 1, 1), "deom_grp4_w5"), ((64, 462, 5, 2, 1, 0, 1), "deom_grp4_w5"),
    ((64, 6188, 5, 2, 1, 1, 1), "deom_pipe_k5"), ((64, 6188, 5, 2, 1, 0, 1), "deom_grp4_w5"),
    ((128, nado(6, 5), 5, 2, 1, 1, 1), "deom_grp4_uniform"),          # test_deom_xcd_block_classes (2, 128, 4), L = 6
    ((1, nado(2, 4), 4, 12, 2, 0, 0), "deom_mfma16"),                 # test_deom_mfma16_matches_oracle (12, 2, 1, 2)
    ((1, nado(3, 2), 2, 16, 1, 0, 0), "deom_mfma16"), ((1, nado(3, 2), 2, 16, 2, 0, 0), "deom_mfma16"),
]


@pytest.mark.parametrize("shape,name", ANCHORS)
def test_stage_plan_anchors(plan, shape, name):
    assert (nado(8, 5), nado(11, 4), nado(7, 6), nado(6, 5), nado(12, 5)) == (1287, 1365, 1716, 462, 6188)
    p = StagePlan()
    plan.plan_deom_stage(*shape, ctypes.byref(p))
    assert not p.refusal and p.name.decode() == name, (shape, p.name, p.msg)


def band_key(p):
    return (p.name.decode(), p.G, p.KMAX, p.NS2, p.TPB, p.FAST)


def test_band_plans(plan):
    from pyqed_amd.deom import banded_ok
    reached, refused, p, hit = set(), set(), BandPlan(), (ctypes.c_int * 5)()
    ref = ctypes.byref(p)

    def accepts(*shape):
        plan.plan_deom_band(*shape, ref)
        return not p.refusal

    # max_own: the issue's sizes, and 128 for the 512-thread class of ns = 2 (4 lanes per ADO)
    for ns, K, nmod, max_own in itertools.product(range(1, 6), range(1, 10), range(1, 4), (1, 24, 64, 128, 256, 257)):
        locs = [max_own, max_own + 7]
        if accepts(ns, K, nmod, max_own, max_own):   # the largest max_loc the plan takes, and one past it
            lo, hi = max_own, 1 << 20
            assert not accepts(ns, K, nmod, max_own, hi)
            while hi - lo > 1:
                mid = (lo + hi) // 2
                lo, hi = (mid, hi) if accepts(ns, K, nmod, max_own, mid) else (lo, mid)
            locs += [lo, lo + 1]
        for i, max_loc in enumerate(locs):
            what = (ns, K, nmod, max_own, max_loc)
            ok = accepts(*what)
            assert (p.refusal in (BAND_NS, BAND_K)) == (not banded_ok(ns, K)), what
            assert i != 2 or ok, what                        # the largest max_loc within the LDS ...
            assert i != 3 or p.refusal == BAND_LDS, what     # ... and the first beyond it
            if not ok:   # by a stated rule, never a dispatch miss
                assert p.refusal in (BAND_NS, BAND_K, BAND_LANES, BAND_LDS), what
                assert p.msg.startswith(b"qd_deom_rk4_banded: "), (what, p.msg)
                refused.add(p.refusal)
                continue
            assert p.tpb % 64 == 0 and 64 <= p.tpb <= p.TPB and p.TPB in (256, 512, 1024), what
            assert p.G >= ns * ns and p.tpb >= max_own * p.G and p.KMAX >= K, what   # a lane group per owned ADO
            # H(t), Q(t), the band's rows and the zero row of absent neighbours
            assert (1 + nmod + max_loc + 1) * ns * ns * 16 <= p.lds <= LDS_MAX, what
            assert not p.FAST or (p.NS2 and p.KMAX == K and nmod == 1), what
            assert bool(p.NS2) == (ns == 2), what
            assert plan.plan_deom_band_hits(ref, hit) == 1, what + ("dispatch miss",)
            assert tuple(hit) == (p.G, p.KMAX, p.NS2, p.TPB, p.FAST), what
            reached.add(band_key(p))
    assert reached == BAND_KERNELS, (sorted(reached - BAND_KERNELS), sorted(BAND_KERNELS - reached))
    assert refused == {BAND_NS, BAND_K, BAND_LANES, BAND_LDS}


def test_python_shape_rules_agree_with_the_plans(plan):
    """DEOMSolver decides the layout and the banded launch before any device call; its two rules against the plans."""
    from pyqed_amd.deom import ado_major_ok, banded_ok
    sp, bp = StagePlan(), BandPlan()
    for ns, K in itertools.product(range(1, 21), range(1, 23)):
        plan.plan_deom_stage(16, 24, K, ns, 1, 1, 1, ctypes.byref(sp))
        assert (not sp.refusal) == ado_major_ok(ns, K), (ns, K, sp.msg)
        plan.plan_deom_band(ns, K, 1, 8, 20, ctypes.byref(bp))
        assert (not bp.refusal) == banded_ok(ns, K), (ns, K, bp.msg)


def test_unplanned_values_miss_the_dispatch(plan):
    """Values no plan returns reach no kernel: the dispatch reports the miss instead of launching nothing."""
    sp, bp, hit = StagePlan(), BandPlan(), (ctypes.c_int * 7)()
    plan.plan_deom_stage(64, 462, 5, 2, 1, 1, 1, ctypes.byref(sp))
    assert plan.plan_deom_stage_hits(ctypes.byref(sp), hit) == 1
    for field, value in (("KMAX", 7), ("G", 8), ("kind", 99), ("UNI", 1), ("HM", 0)):   # w5 exists for one set only
        q = StagePlan.from_buffer_copy(sp)
        setattr(q, field, value)
        assert plan.plan_deom_stage_hits(ctypes.byref(q), hit) == 0, (field, value)
    plan.plan_deom_band(2, 5, 1, 24, 60, ctypes.byref(bp))
    assert plan.plan_deom_band_hits(ctypes.byref(bp), hit) == 1
    for field, value in (("KMAX", 8), ("TPB", 128), ("G", 8), ("NS2", 0)):   # FAST exists for K = 5 and 6 only
        q = BandPlan.from_buffer_copy(bp)
        setattr(q, field, value)
        assert plan.plan_deom_band_hits(ctypes.byref(q), hit) == 0, (field, value)
