"""The plan of qd_lvc_pair_observe and qd_lvc_pair_rk4 (LvcPairPlan, pyqed_amd/csrc/lvc_plan.hpp) on the host, compiled
with the host C++ compiler through tools/cpu_emu/lvc_pair_plan_c.cpp.  Enumerated over shapes, P in {1, 3}, block lists
and the three path requests: every launch is legal; the path is the pair limit's; the embedded LvcPlan equals
lvc_plan()'s for the 2 P states; the partial rows hold what the kernels write and every value of a record comes from
exactly one (pass, value) of them; the resident LDS regions are in order, as large as their use and within LVC_LDS_MAX;
the scratch parts do not overlap; every refusal carries its message; P at 32767 and 32768; the limit's neighbours."""
import ctypes
import itertools
import os
import shutil
import subprocess

import pytest

from conftest import ROOT
from test_lvc_plan_host import (AUTO, LDS_CU, RESIDENT, STAGED, LvcLaunch, LvcPlan, check_launch, check_plan,
                                build_plan_lib, plan_of)

EMU_DIR = os.path.join(ROOT, "tools", "cpu_emu")
FN = "qd_lvc_pair_rk4"
NSTEPS, SE = 5, 2


class LvcPairBlocks(ctypes.Structure):
    _fields_ = [("nblk", ctypes.c_int), ("r", ctypes.c_int * 7)]


class LvcPairPlan(ctypes.Structure):
    _fields_ = [("refused", ctypes.c_int), ("base", LvcPlan), ("P", ctypes.c_int), ("blocks", LvcPairBlocks)] + \
               [(n, ctypes.c_int) for n in ("rows", "passes", "nv", "nrec")] + \
               [(n, LvcLaunch) for n in ("part", "fin", "resident")] + \
               [(n, ctypes.c_size_t) for n in ("lds_ket1", "lds_bra0", "lds_bra1", "lds_tab", "lds_wave", "lds_tile",
                                               "ws_part", "ws_part_bytes", "ws_total")] + \
               [("msg", ctypes.c_char * 200)]


def build_pair_plan_lib(tmp):
    """The pair plan library and its constants as attributes (also used by the GPU tests)."""
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "c++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    so = os.path.join(str(tmp), "liblvc_pair_plan.so")
    subprocess.run([cxx, "-std=c++17", "-O1", "-shared", "-fPIC", "-Wall", "-Werror",
                    os.path.join(EMU_DIR, "lvc_pair_plan_c.cpp"), "-o", so], check=True)
    lib = ctypes.CDLL(so)
    lib.plan_lvc_pair.restype = None
    lib.plan_lvc_pair.argtypes = [ctypes.c_char_p, ctypes.c_long, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                  ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                  ctypes.POINTER(LvcPairPlan)]
    lib.plan_lvc_pair_limit.restype = ctypes.c_long
    lib.plan_lvc_pair_limit.argtypes = [ctypes.c_int]
    lib.limit = lib.plan_lvc_pair_limit      # the resident limit of a model with M modes; RES_MAX_D is the largest
    c = (ctypes.c_long * 10)()
    lib.plan_lvc_pair_constants(c)
    (lib.PAIR_MAX, lib.RES_MAX_D, lib.LDS_MAX, lib.TILE, lib.RES_TPB, lib.NV_MAX, lib.REG_NEL, lib.OBS_MAX_GRID,
     lib.SIZEOF_PLAN, lib.SIZEOF_PAIR_PLAN) = c
    assert lib.SIZEOF_PLAN == ctypes.sizeof(LvcPlan) and lib.SIZEOF_PAIR_PLAN == ctypes.sizeof(LvcPairPlan)
    return lib


def _ints(v):
    return None if v is None else (ctypes.c_int * max(1, len(v)))(*v)


def pair_plan_of(lib, P, nel, dims, blocks=(0,), path=AUTO, nsteps=NSTEPS, se=SE, fn=FN, nblk=None):
    p = LvcPairPlan()
    nblk = (0 if blocks is None else len(blocks)) if nblk is None else nblk
    lib.plan_lvc_pair(fn.encode(), P, nel, 0 if dims is None else len(dims), _ints(dims), nblk, _ints(blocks), path,
                      nsteps, se, ctypes.byref(p))
    return p


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    lib = build_pair_plan_lib(tmp_path_factory.mktemp("pair_plan"))
    assert lib.PAIR_MAX == 32767 and lib.LDS_MAX <= LDS_CU and lib.NV_MAX == 2 * lib.REG_NEL ** 2
    return lib


@pytest.fixture(scope="module")
def base_lib(tmp_path_factory):
    return build_plan_lib(tmp_path_factory.mktemp("plan"))


def _shapes(lib):
    L, T = lib.RES_MAX_D, lib.TILE
    for M in range(3, 7):           # the neighbours of every mode count's own limit
        n = lib.limit(M) // 3       # 0 where the plan never goes resident: the smallest model is staged then
        yield from [(3, (1,) * (M - 1) + (max(n, 1),)), (3, (1,) * (M - 1) + (n + 1,))]
    yield from [(1, (1,)), (1, (2,)), (2, (2, 2)), (3, (3, 5, 7)), (4, (3, 5)), (5, (4, 3)), (8, (4, 3)), (3, (5, 67)),
                (3, (65, 3)), (2, (1, 9, 1)), (3, (2,) * 6), (3, (T - 1,)), (3, (T,)), (3, (T + 1,)), (1, (L,)),
                (1, (L + 1,)), (3, (L // 3,)), (3, (L // 3 + 1,)), (8, (L // 8,)), (8, (L // 8 + 1,)),
                (8, (1, 1, 1, 1, 1, L // 8)), (4, (1, 1, 1, 1, 1, L // 4)), (7, (2, 2, 2, 2, 2, 4)), (6, (13, 13)),
                (3, (16, 16, 16)), (3, (20,) * 5), (1, (T * lib.OBS_MAX_GRID + 1,))]


def _block_sets(M):
    yield (0,)
    yield (M,)
    yield tuple(range(1 + M))
    yield tuple(reversed(range(1 + M)))
    if M > 1:
        yield (1, 0)
        yield (M, M)


def check_pair_plan(lib, base_lib, p, P, nel, dims, blocks, path_req, what):
    M, nblk = len(dims), len(blocks)
    D = p.base.dev.D
    fits = D <= lib.limit(M)
    assert p.base.path == ((RESIDENT if fits else STAGED) if path_req == AUTO else path_req), what
    # the embedded plan is lvc_plan()'s for the 2 P states on that path: byte for byte, and legal by that test's rules
    q = plan_of(base_lib, 2 * P, nel, dims, p.base.path, NSTEPS, SE, 1, fn=FN)
    assert not q.refused and bytes(p.base) == bytes(q), what
    check_plan(base_lib, p.base, 2 * P, nel, dims, p.base.path, what)
    assert p.P == P and p.blocks.nblk == nblk and list(p.blocks.r[:nblk]) == list(blocks), what
    # one pass takes every row up to REG_NEL states, one row past it; a partial row holds the pass's sums
    assert (p.rows, p.passes) == ((nel, 1) if nel <= lib.REG_NEL else (1, nel)), what
    assert p.nv == 2 * nel * p.rows <= lib.NV_MAX and p.nv <= lib.TILE and p.nrec == nblk * nel * nel, what
    # every double of a record comes from exactly one (pass, value)
    slots = sorted(2 * ((q_ * p.rows + v // (2 * nel)) * nel + (v // 2) % nel) + (v & 1)
                   for q_ in range(p.passes) for v in range(p.nv))
    assert slots == list(range(2 * nel * nel)), what
    check_launch(p.part, what)
    check_launch(p.fin, what)
    tiles = p.base.stage.gx
    assert (p.part.gx, p.part.gy, p.part.gz, p.part.tpb) == (p.base.G, nblk * p.passes, P, lib.TILE), what
    assert p.part.gx == min(tiles, lib.OBS_MAX_GRID) and (p.fin.gx, p.fin.tpb) == (P, lib.TILE), what
    # scratch: the stage vectors of the 2 P states, then the partial rows, in order and without overlap
    assert p.base.ws_x1 - p.base.ws_x0 >= 2 * P * D * 16 and p.ws_part - p.base.ws_x1 >= 2 * P * D * 16, what
    assert p.ws_part % 16 == 0 and p.ws_part_bytes >= P * nblk * p.passes * p.base.G * p.nv * 8, what
    assert p.ws_total == p.ws_part + p.ws_part_bytes, what
    if fits:
        check_launch(p.resident, what, lib.LDS_MAX)
        assert (p.resident.gx, p.resident.tpb) == (P, lib.RES_TPB), what
        offs = (0, p.lds_ket1, p.lds_bra0, p.lds_bra1, p.lds_tab, p.lds_wave, p.lds_tile, p.resident.lds)
        need = (D * 16,) * 4 + ((1 + M) * nel * nel * 16, (lib.RES_TPB // 64) * p.nv * 8, tiles * p.nv * 8)
        assert all(o % 16 == 0 for o in offs), what
        assert all(b - a >= n for a, b, n in zip(offs, offs[1:], need)), (what, offs, need)
        # the kernel's points per thread cover the state
        kp = -(-(-(-lib.RES_MAX_D // nel)) // lib.RES_TPB)
        assert kp * lib.RES_TPB >= p.base.dev.nvib and tiles == p.base.G, what
    else:
        assert path_req != RESIDENT, what


def test_plans_are_legal(plan, base_lib):
    lib = plan
    accepted, worst_lds = 0, 0
    for nel, dims in _shapes(lib):
        M = len(dims)
        D = nel
        for N in dims:
            D *= N
        for blocks, P, path_req in itertools.product(_block_sets(M), (1, 3), (AUTO, STAGED, RESIDENT)):
            what = (nel, dims, blocks, P, path_req)
            p = pair_plan_of(lib, P, nel, dims, blocks, path_req)
            if path_req == RESIDENT and D > lib.limit(M):
                assert p.refused and p.msg.decode() == \
                    f"{FN}: the pair resident path needs D <= {lib.limit(M)} with {M} modes (D = {D})", what
                continue
            assert not p.refused, (what, p.msg)
            check_pair_plan(lib, base_lib, p, P, nel, dims, blocks, path_req, what)
            worst_lds = max(worst_lds, p.resident.lds)
            accepted += 1
            # qd_lvc_pair_observe's call: no path, no steps
            o = pair_plan_of(lib, P, nel, dims, blocks, AUTO, 0, 0, fn="qd_lvc_pair_observe")
            assert not o.refused and bytes(o.part) == bytes(p.part) and bytes(o.fin) == bytes(p.fin), what
            assert o.ws_part_bytes == p.ws_part_bytes, what
    print(f"pair plans accepted {accepted}, largest resident LDS {worst_lds} of {lib.LDS_MAX}")
    assert accepted > 300 and 64 * 1024 < worst_lds <= lib.LDS_MAX


def test_every_refusal_carries_its_message(plan):
    lib = plan
    for kw, msg in ((dict(P=0), "P=0 outside [1, 32767]"), (dict(P=-1), "P=-1 outside [1, 32767]"),
                    (dict(P=32768), "P=32768 outside [1, 32767]"),
                    (dict(blocks=None, nblk=1), "null blocks"),
                    (dict(blocks=()), "nblk=0 outside [1, 3]"), (dict(blocks=(0, 1, 2, 0)), "nblk=4 outside [1, 3]"),
                    (dict(blocks=(0, 3)), "blocks[1]=3 outside [0, 2]"), (dict(blocks=(-1,)), "blocks[0]=-1 outside [0, 2]"),
                    (dict(se=0), "observables need save_every > 0"),
                    # everything qd_lvc_rk4 refuses, under this entry point's name
                    (dict(nel=0), "nel=0 outside [1, 8]"), (dict(nel=9), "nel=9 outside [1, 8]"),
                    (dict(dims=()), "M=0 outside [1, 6]"), (dict(dims=(2,) * 7), "M=7 outside [1, 6]"),
                    (dict(dims=(2, 0)), "dims[1]=0 must be at least 1"),
                    (dict(nel=2, dims=(1024, 1024, 1024)), "D = nel * prod(dims) must stay below 2^31"),
                    (dict(path=-1), "path=-1 outside [0, 2]"), (dict(path=3), "path=3 outside [0, 2]"),
                    (dict(nsteps=-1), "nsteps=-1 and save_every=2 must not be negative"),
                    (dict(se=-2), "nsteps=5 and save_every=-2 must not be negative"),
                    (dict(dims=(19, 18), path=RESIDENT), f"the pair resident path needs D <= {lib.limit(2)} with 2 modes (D = 1026)"),
                    (dict(dims=(1, 1, 1, 1, 1, lib.limit(6) // 3 + 1), path=RESIDENT),
                     f"the pair resident path needs D <= {lib.limit(6)} with 6 modes (D = {lib.limit(6) // 3 * 3 + 3})")):
        args = dict(P=1, nel=3, dims=(4, 4), blocks=(0, 2), path=AUTO, nsteps=5, se=2)
        args.update(kw)
        p = pair_plan_of(lib, **args)
        assert p.refused and p.msg.decode() == f"{FN}: {msg}", (kw, p.msg)
    p = LvcPairPlan()
    lib.plan_lvc_pair(FN.encode(), 1, 3, 2, None, 1, _ints((0,)), 0, 0, 0, ctypes.byref(p))
    assert p.refused and p.msg.decode() == f"{FN}: null dims"
    # admitted at the edges: no steps needs no save_every, the largest P, a block named twice
    assert not pair_plan_of(lib, 1, 3, (4, 4), (0,), nsteps=0, se=0).refused
    assert not pair_plan_of(lib, 32767, 3, (4, 4), (0,)).refused
    assert not pair_plan_of(lib, 1, 3, (4, 4), (2, 2, 2)).refused


def test_the_largest_batch(plan):
    """P = 32767: the 2 P states are one legal batch of the stage kernel; P = 32768 is refused."""
    lib = plan
    p = pair_plan_of(lib, 32767, 2, (3, 3), (0, 1, 2))
    assert not p.refused and p.base.stage.gy == 65534 and p.part.gz == 32767 and p.resident.gx == 32767
    check_launch(p.base.stage, "stage")
    check_launch(p.part, "part")
    q = pair_plan_of(lib, 32768, 2, (3, 3), (0, 1, 2))
    assert q.refused and q.msg.decode() == f"{FN}: P=32768 outside [1, 32767]"


def test_resident_limit_and_cap(plan, base_lib):
    """At the pair limit of its mode count the resident LDS stays within LVC_LDS_MAX for every (nel, M); one element past
    it the plan goes staged and a forced resident call is refused.  No limit exceeds half the single-state kernel's,
    the size the kernel is built for, and the limits do not grow with the mode count (the measured crossovers)."""
    lib = plan
    lims = [lib.limit(M) for M in range(1, 7)]
    assert lib.RES_MAX_D == max(lims) <= base_lib.RES_MAX_D // 2 and lib.LDS_MAX == base_lib.LDS_MAX
    assert lims == sorted(lims, reverse=True) and min(lims) >= 0
    for nel in range(1, 9):
        for M in range(1, 7):
            nv = lib.limit(M) // nel
            blocks = tuple(range(1 + M))
            if nv == 0:     # never resident with this many modes: the smallest model is staged, a forced call refused
                assert pair_plan_of(lib, 1, nel, (1,) * M, blocks).base.path == STAGED
                assert pair_plan_of(lib, 1, nel, (1,) * M, blocks, path=RESIDENT).refused
                continue
            p = pair_plan_of(lib, 1, nel, (1,) * (M - 1) + (nv,), blocks)
            assert not p.refused and p.base.path == RESIDENT and p.resident.lds <= lib.LDS_MAX <= LDS_CU
            q = pair_plan_of(lib, 1, nel, (1,) * (M - 1) + (nv + 1,), blocks)
            assert not q.refused and q.base.path == STAGED
            r = pair_plan_of(lib, 1, nel, (1,) * (M - 1) + (nv + 1,), blocks, path=RESIDENT)
            assert r.refused and r.msg.decode() == \
                f"{FN}: the pair resident path needs D <= {lib.limit(M)} with {M} modes (D = {nel * (nv + 1)})"
