"""The plan of qd_lvc_driven_rk4 (LvcDrivePlan, pyqed_amd/csrc/lvc_plan.hpp) on the host, compiled with the host C++
compiler through tools/cpu_emu/lvc_drive_plan_c.cpp.  Enumerated over shapes, nd in 0 .. 8, every drive_mode value, both
sampling modes and hold in {1, 2, 3, nsteps + 1}: every launch is legal and the driven resident kernel's LDS stays
within the plan's own cap (itself within a CU's 160 KiB), regions in order and as large as their use; the scratch parts
do not overlap; the row of every (step, stage) is within nf exactly when the plan admits nf; every refusal carries its
message; the embedded LvcPlan equals lvc_plan()'s for the same shape."""
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
FN = "qd_lvc_driven_rk4"
HOLD, STAGE = 0, 1
NSTEPS, SE = 5, 2


class LvcDrive(ctypes.Structure):
    _fields_ = [("nd", ctypes.c_int), ("mode", ctypes.c_int * 8)]


class LvcDrivePlan(ctypes.Structure):
    _fields_ = [("refused", ctypes.c_int), ("base", LvcPlan), ("drive", LvcDrive), ("sample", ctypes.c_int),
                ("hold", ctypes.c_int), ("rows_needed", ctypes.c_int), ("resident", LvcLaunch)] + \
               [(n, ctypes.c_size_t) for n in ("lds_vec1", "lds_tab", "lds_eff", "lds_drv", "lds_wave", "lds_tile",
                                               "lds_nbar", "ws_acc", "ws_total")] + \
               [("msg", ctypes.c_char * 200)]


def build_drive_plan_lib(tmp):
    """The driven plan library and its constants as attributes (also used by the GPU tests)."""
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "c++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    so = os.path.join(str(tmp), "liblvc_drive_plan.so")
    subprocess.run([cxx, "-std=c++17", "-O1", "-shared", "-fPIC", "-Wall", "-Werror",
                    os.path.join(EMU_DIR, "lvc_drive_plan_c.cpp"), "-o", so], check=True)
    lib = ctypes.CDLL(so)
    lib.plan_lvc_drive.restype = None
    lib.plan_lvc_drive.argtypes = [ctypes.c_char_p, ctypes.c_long, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                   ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_long,
                                   ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                   ctypes.POINTER(LvcDrivePlan)]
    lib.plan_lvc_drive_limit.restype = ctypes.c_long
    lib.plan_lvc_drive_limit.argtypes = [ctypes.c_int]
    lib.plan_lvc_drive_row.restype = ctypes.c_long
    lib.plan_lvc_drive_row.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_long, ctypes.c_int]
    c = (ctypes.c_long * 7)()
    lib.plan_lvc_drive_constants(c)
    lib.MAX_DRIVES, lib.RES_MAX_D, lib.LDS_MAX, lib.TILE, lib.RES_TPB, lib.OBS_NV, lib.SIZEOF_PLAN = c
    assert lib.SIZEOF_PLAN == ctypes.sizeof(LvcPlan)
    lib.limit = lib.plan_lvc_drive_limit      # the resident limit of a model with M modes; RES_MAX_D is the largest
    return lib


def _ints(v):
    return None if v is None else (ctypes.c_int * max(1, len(v)))(*v)


def drive_plan_of(lib, B, nel, dims, modes=(), sample=HOLD, hold=1, nf=None, path=AUTO, nsteps=NSTEPS, se=SE, obs=1,
                  fn=FN, nd=None):
    p = LvcDrivePlan()
    nd = (0 if modes is None else len(modes)) if nd is None else nd
    if nf is None:
        nf = 2 * nsteps + 1
    lib.plan_lvc_drive(fn.encode(), B, nel, 0 if dims is None else len(dims), _ints(dims), nd,
                       _ints(modes) if modes is not None else None, sample, hold, nf, path, nsteps, se, obs,
                       ctypes.byref(p))
    return p


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    lib = build_drive_plan_lib(tmp_path_factory.mktemp("drive_plan"))
    assert lib.MAX_DRIVES == 8 and lib.LDS_MAX <= LDS_CU
    return lib


@pytest.fixture(scope="module")
def base_lib(tmp_path_factory):
    return build_plan_lib(tmp_path_factory.mktemp("plan"))


def _rows(lib, sample, hold, nsteps):
    return [lib.plan_lvc_drive_row(sample, hold, s, stage) for s in range(nsteps) for stage in range(4)]


def _shapes(lib):
    L, T, L6 = lib.RES_MAX_D, lib.TILE, lib.limit(6)
    yield from [(3, (2, 2, 2, 2, 2, L6 // 96)), (3, (1, 1, 1, 1, 1, L6 // 3)), (3, (1, 1, 1, 1, 1, L6 // 3 + 1)),
                (1, (1, 1, 1, 1, 1, L)), (1, (1, 1, 1, 1, L)),
                (1, (1,)), (1, (2,)), (3, (70,)), (3, (3, 5, 7)), (8, (4, 3)), (3, (2,) * 6), (3, (5, 67)), (3, (65, 3)),
                (2, (1, 9, 1)), (3, (37, 37)), (3, (T - 1,)), (3, (T,)), (3, (T + 1,)), (1, (L,)), (1, (L + 1,)),
                (8, (L // 8,)), (8, (1, 1, 1, 1, 1, L // 8)), (8, (L // 8 + 1,)), (3, (L // 3,)), (3, (L // 3 + 1,)),
                (3, (20,) * 5), (7, (2, 2, 2, 2, 2, 9))]


def _mode_sets(M):
    """nd = 0 .. 8 with every drive_mode value -1 .. M - 1 taken somewhere, and all drives on one table."""
    vals = list(range(-1, M))
    for nd in range(0, 9):
        yield tuple(vals[(d + nd) % len(vals)] for d in range(nd))
    for v in vals:
        yield (v,) * 8


def check_drive_plan(lib, base_lib, p, B, nel, dims, modes, sample, hold, path_req, what):
    M, nd = len(dims), len(modes)
    D = p.base.dev.D
    # the path is the driven limit's choice
    fits = D <= lib.limit(M)
    assert p.base.path == ((RESIDENT if fits else STAGED) if path_req == AUTO else path_req), what
    # the embedded plan is lvc_plan()'s for that path: byte for byte, and legal by the undriven test's own rules
    q = plan_of(base_lib, B, nel, dims, p.base.path, NSTEPS, SE, 1, fn=FN)
    assert not q.refused and bytes(p.base) == bytes(q), what
    check_plan(base_lib, p.base, B, nel, dims, p.base.path, what)
    assert p.drive.nd == nd and list(p.drive.mode[:nd]) == list(modes), what
    assert p.sample == sample and (sample == STAGE or p.hold == hold) and p.hold >= 1, what
    # scratch: the undriven parts, then the accumulator in stage mode, in order and without overlap
    assert p.ws_acc == p.base.ws_total and p.ws_acc % 16 == 0, what
    assert p.ws_total - p.ws_acc == (B * D * 16 if sample == STAGE else 0), what
    if fits:
        check_launch(p.resident, what, lib.LDS_MAX)
        assert (p.resident.gx, p.resident.tpb) == (B, lib.RES_TPB), what
        tab = (1 + M) * nel * nel * 16
        tiles = p.base.stage.gx
        offs = (0, p.lds_vec1, p.lds_tab, p.lds_eff, p.lds_drv, p.lds_wave, p.lds_tile, p.lds_nbar, p.resident.lds)
        need = (D * 16, D * 16, tab, tab, nd * nel * nel * 16, (lib.RES_TPB // 64) * lib.OBS_NV * 8,
                tiles * lib.OBS_NV * 8, M * nel * 8)
        assert all(o % 16 == 0 for o in offs), what
        assert all(b - a >= n for a, b, n in zip(offs, offs[1:], need)), (what, offs, need)
        assert p.base.kp * lib.RES_TPB >= p.base.dev.nvib, what
    else:
        assert path_req != RESIDENT, what


def test_plans_are_legal(plan, base_lib):
    lib = plan
    accepted = 0
    worst_lds = 0
    for nel, dims in _shapes(lib):
        M = len(dims)
        D = nel
        for N in dims:
            D *= N
        for modes, sample, hold, B, path_req in itertools.product(
                _mode_sets(M), (HOLD, STAGE), (1, 2, 3, NSTEPS + 1), (1, 3), (AUTO, STAGED, RESIDENT)):
            what = (nel, dims, modes, sample, hold, B, path_req)
            p = drive_plan_of(lib, B, nel, dims, modes, sample, hold, path=path_req)
            if path_req == RESIDENT and D > lib.limit(M):
                assert p.refused and p.msg.decode() == \
                    f"{FN}: the resident path needs D <= {lib.limit(M)} with {M} modes (D = {D})", what
                continue
            assert not p.refused, (what, p.msg)
            check_drive_plan(lib, base_lib, p, B, nel, dims, modes, sample, hold, path_req, what)
            worst_lds = max(worst_lds, p.resident.lds)
            accepted += 1
    print(f"driven plans accepted {accepted}, largest resident LDS {worst_lds} of {lib.LDS_MAX}")
    assert accepted > 5000 and 64 * 1024 < worst_lds <= lib.LDS_MAX


def test_rows_are_within_nf_exactly_when_admitted(plan):
    lib = plan
    for sample, nsteps in itertools.product((HOLD, STAGE), (0, 1, 2, 5, 6, 7)):
        for hold in (1, 2, 3, nsteps + 1):
            rows = _rows(lib, sample, hold, nsteps)
            if sample == STAGE:
                assert rows == [r for s in range(nsteps) for r in (2 * s, 2 * s + 1, 2 * s + 1, 2 * s + 2)]
            else:
                assert rows == [s // hold for s in range(nsteps) for _ in range(4)]
            need = max(rows) + 1 if rows else 0
            assert need == (0 if nsteps == 0 else 2 * nsteps + 1 if sample == STAGE else -(-nsteps // hold))
            for nf in range(0, need + 3):
                p = drive_plan_of(lib, 1, 3, (4, 5), (-1, 1), sample, hold, nf=nf, nsteps=nsteps, se=1)
                within = all(r < nf for r in rows)
                assert (not p.refused) == within, (sample, nsteps, hold, nf, p.msg)
                if p.refused:
                    rule = "2 nsteps + 1" if sample == STAGE else "ceil(nsteps / hold)"
                    assert p.msg.decode() == f"{FN}: fvals holds {nf} rows, {need} are needed ({rule})"
                else:
                    assert p.rows_needed == need
            # with no drive nothing of fvals is read: any nf, and no drive_mode
            p = drive_plan_of(lib, 1, 3, (4, 5), None, sample, hold, nf=0, nsteps=nsteps, se=1)
            assert not p.refused and p.rows_needed == 0 and p.drive.nd == 0


def test_every_refusal_carries_its_message(plan):
    lib = plan
    for kw, msg in ((dict(nd=-1), "nd=-1 outside [0, 8]"), (dict(nd=9, modes=(0,) * 9), "nd=9 outside [0, 8]"),
                    (dict(modes=None, nd=2), "null drive_mode"),
                    (dict(modes=(-1, 2)), "drive_mode[1]=2 outside [-1, 2)"),
                    (dict(modes=(-2,)), "drive_mode[0]=-2 outside [-1, 2)"),
                    (dict(sample=2), "sample=2 outside {0, 1}"), (dict(sample=-1), "sample=-1 outside {0, 1}"),
                    (dict(hold=0), "hold=0 must be at least 1"), (dict(hold=-3), "hold=-3 must be at least 1"),
                    (dict(nf=2, hold=2), "fvals holds 2 rows, 3 are needed (ceil(nsteps / hold))"),
                    (dict(nf=10, sample=STAGE), "fvals holds 10 rows, 11 are needed (2 nsteps + 1)"),
                    # everything qd_lvc_rk4 refuses, under this entry point's name
                    (dict(nel=0), "nel=0 outside [1, 8]"), (dict(nel=9), "nel=9 outside [1, 8]"),
                    (dict(dims=()), "M=0 outside [1, 6]"), (dict(dims=(2,) * 7), "M=7 outside [1, 6]"),
                    (dict(dims=(2, 0)), "dims[1]=0 must be at least 1"),
                    (dict(nel=2, dims=(1024, 1024, 1024)), "D = nel * prod(dims) must stay below 2^31"),
                    (dict(B=0), "B=0 outside [1, 65535]"), (dict(B=65536), "B=65536 outside [1, 65535]"),
                    (dict(path=-1), "path=-1 outside [0, 2]"), (dict(path=3), "path=3 outside [0, 2]"),
                    (dict(nsteps=-1), "nsteps=-1 and save_every=2 must not be negative"),
                    (dict(se=-2), "nsteps=5 and save_every=-2 must not be negative"),
                    (dict(se=0, obs=1), "observables need save_every > 0"),
                    (dict(dims=(37, 37), path=RESIDENT), "the resident path needs D <= 2048 with 2 modes (D = 4107)"),
                    (dict(dims=(1, 1, 1, 1, 1, 513), path=RESIDENT),
                     "the resident path needs D <= 1536 with 6 modes (D = 1539)")):
        args = dict(B=1, nel=3, dims=(4, 4), modes=(-1, 1), sample=HOLD, hold=1, nf=11, path=AUTO, nsteps=5, se=2,
                    obs=1)
        args.update(kw)
        p = drive_plan_of(lib, **args)
        assert p.refused and p.msg.decode() == f"{FN}: {msg}", (kw, p.msg)
    p = LvcDrivePlan()
    lib.plan_lvc_drive(FN.encode(), 1, 3, 2, None, 0, None, 0, 1, 0, 0, 0, 0, 0, ctypes.byref(p))
    assert p.refused and p.msg.decode() == f"{FN}: null dims"
    # admitted at the edges: hold is ignored in stage mode, nd = 8, a hold past the call, no steps
    assert not drive_plan_of(lib, 1, 3, (4, 4), (-1,), STAGE, hold=0).refused
    assert not drive_plan_of(lib, 1, 3, (4, 4), (1,) * 8, HOLD, hold=6, nf=1).refused
    assert not drive_plan_of(lib, 1, 3, (4, 4), (0,), STAGE, nf=0, nsteps=0, se=0).refused


def test_resident_limit_and_cap(plan):
    """At the driven limit of its mode count the resident LDS stays within the driven cap for every (nel, M) with all
    eight drives; one element past it the plan goes staged.  The limit is the measured crossover: 2048, the size the
    kernel is built for, in one to five modes, 1536 in six."""
    lib = plan
    assert [lib.limit(M) for M in range(1, 7)] == [2048] * 5 + [1536] and lib.RES_MAX_D == max(map(lib.limit, range(1, 7)))
    for nel in range(1, 9):
        for M in range(1, 7):
            nv = lib.limit(M) // nel
            dims = (1,) * (M - 1) + (nv,)
            p = drive_plan_of(lib, 1, nel, dims, (-1,) * 8, STAGE, nf=11)
            assert not p.refused and p.base.path == RESIDENT and p.resident.lds <= lib.LDS_MAX <= LDS_CU
            q = drive_plan_of(lib, 1, nel, (1,) * (M - 1) + (nv + 1,), (-1,) * 8, STAGE, nf=11)
            assert not q.refused and q.base.path == STAGED
            r = drive_plan_of(lib, 1, nel, (1,) * (M - 1) + (nv + 1,), (-1,) * 8, STAGE, nf=11, path=RESIDENT)
            assert r.refused and r.msg.decode() == \
                f"{FN}: the resident path needs D <= {lib.limit(M)} with {M} modes (D = {nel * (nv + 1)})"
