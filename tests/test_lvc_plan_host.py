"""The launch plan of the LVC entry points (pyqed_amd/csrc/lvc_plan.hpp) on the host, compiled with the host C++
compiler through tools/cpu_emu/lvc_plan_c.cpp.  Nothing of the rules is restated here: the tests enumerate shapes and
check that every planned launch is legal, that the tiles cover every vibrational index exactly once, that the resident
rule is consistent with the LDS bytes planned, that the scratch parts do not overlap, and that every refusal carries
its entry point's message.  What a kernel covers (LVC_TILE points per workgroup, the tiles g, g + G, ... per partial
workgroup, kp points per resident thread) is the kernel's geometry, read from the plan's constants."""
import ctypes
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT

EMU_DIR = os.path.join(ROOT, "tools", "cpu_emu")
GRID_X_MAX, GRID_YZ_MAX = 2 ** 31 - 1, 65535
LDS_DEFAULT_MAX = 64 * 1024     # what a kernel may ask for without raising its limit (only the resident kernel raises it)
LDS_CU = 160 * 1024
FN = "qd_lvc_rk4"
AUTO, STAGED, RESIDENT = 0, 1, 2


class LvcDev(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int) for n in ("nel", "M", "nvib", "D")] + \
               [("dims", ctypes.c_int * 6), ("stride", ctypes.c_int * 6), ("omega", ctypes.c_double * 6)]


class LvcLaunch(ctypes.Structure):
    _fields_ = [(n, ctypes.c_uint) for n in ("gx", "gy", "gz")] + [("tpb", ctypes.c_int), ("lds", ctypes.c_size_t)]


class LvcPlan(ctypes.Structure):
    _fields_ = [("refused", ctypes.c_int), ("path", ctypes.c_int), ("dev", LvcDev)] + \
               [(n, ctypes.c_int) for n in ("nobs", "rows", "G", "kp")] + \
               [(n, LvcLaunch) for n in ("stage", "resident", "obs_part", "obs_final", "snap")] + \
               [(n, ctypes.c_size_t) for n in ("lds_vec1", "lds_tab", "lds_wave", "lds_tile", "lds_nbar", "ws_x0",
                                               "ws_x1", "ws_part", "ws_part_bytes", "ws_total")] + \
               [("msg", ctypes.c_char * 160)]


def build_plan_lib(tmp):
    """The plan library and its constants as attributes (also used by the GPU tests)."""
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "c++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    so = os.path.join(str(tmp), "liblvc_plan.so")
    subprocess.run([cxx, "-std=c++17", "-O1", "-shared", "-fPIC", "-Wall", "-Werror",
                    os.path.join(EMU_DIR, "lvc_plan_c.cpp"), "-o", so], check=True)
    lib = ctypes.CDLL(so)
    lib.plan_lvc.restype = None
    lib.plan_lvc.argtypes = [ctypes.c_char_p, ctypes.c_long, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int,
                             ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(LvcPlan)]
    lib.plan_lvc_constants.restype = None
    c = (ctypes.c_long * 10)()
    lib.plan_lvc_constants(c)
    (lib.MAX_NEL, lib.MAX_MODES, lib.TILE, lib.RES_TPB, lib.RES_MAX_D, lib.OBS_MAX_GRID, lib.OBS_NV, lib.YZ_MAX,
     lib.LDS_MAX, lib.FLAT_GRID_MAX) = c
    return lib


def plan_of(lib, B, nel, dims, path=AUTO, nsteps=5, se=2, obs=1, fn=FN):
    p = LvcPlan()
    d = None if dims is None else (ctypes.c_int * max(1, len(dims)))(*dims)
    lib.plan_lvc(fn.encode(), B, nel, 0 if dims is None else len(dims), d, path, nsteps, se, obs, ctypes.byref(p))
    return p


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    lib = build_plan_lib(tmp_path_factory.mktemp("plan"))
    assert (lib.MAX_NEL, lib.MAX_MODES, lib.YZ_MAX) == (8, 6, GRID_YZ_MAX)
    assert lib.TILE % 64 == 0 and lib.RES_TPB % lib.TILE == 0 and lib.LDS_MAX <= LDS_CU
    return lib


def dims_lists(lib):
    """Every tuple of the extents for M <= 2; for M >= 3 each extent on each axis beside small ones, and a seeded sample
    of the full product."""
    ext = sorted({1, 2, 3, lib.TILE - 1, lib.TILE, lib.TILE + 1, 64, 65, 257})
    rng = np.random.default_rng(11)
    for M in range(1, lib.MAX_MODES + 1):
        if M <= 2:
            yield from itertools.product(ext, repeat=M)
            continue
        seen = set()
        for ax, e, small in itertools.product(range(M), ext, (1, 2, 3)):
            seen.add(tuple(e if k == ax else small for k in range(M)))
        for _ in range(250):
            seen.add(tuple(int(v) for v in rng.choice(ext, M)))
        yield from sorted(seen)


def check_launch(l, what, lds_max=LDS_DEFAULT_MAX):
    assert 1 <= l.gx <= GRID_X_MAX and 1 <= l.gy <= GRID_YZ_MAX and 1 <= l.gz <= GRID_YZ_MAX, what
    assert l.tpb % 64 == 0 and 64 <= l.tpb <= 1024 and l.lds <= lds_max and l.lds % 16 == 0, what


def check_plan(lib, p, B, nel, dims, path_req, what):
    M, d = len(dims), p.dev
    D = nel * int(np.prod(dims, dtype=object))
    assert (d.nel, d.M, d.D, d.nvib * nel) == (nel, M, D, D), what
    # strides: row-major, last mode fastest; padding axes inert
    assert list(d.dims[:M]) == list(dims) and all(d.dims[j] == d.stride[j] == 1 for j in range(M, 6)), what
    assert [d.stride[j] for j in range(M)] == [int(np.prod(dims[j + 1:], dtype=object)) for j in range(M)], what
    assert p.nobs == nel * nel * (1 + M) + M and p.rows == (1 + M) * nel and 2 * nel + 1 <= lib.OBS_NV, what
    # the stage grid: tiles of LVC_TILE points cover [0, nvib) once, members along y
    tiles = p.stage.gx
    check_launch(p.stage, what)
    assert (tiles - 1) * lib.TILE < d.nvib <= tiles * lib.TILE and p.stage.tpb == lib.TILE and p.stage.gy == B, what
    assert p.stage.lds >= (1 + M) * nel * nel * 16, what
    # partial workgroups: g takes the tiles g, g + G, ...: all of them once
    check_launch(p.obs_part, what)
    assert 1 <= p.G <= min(tiles, lib.OBS_MAX_GRID) and p.obs_part.tpb == lib.TILE, what
    assert (p.obs_part.gx, p.obs_part.gy, p.obs_part.gz) == (p.G, p.rows, B), what
    check_launch(p.obs_final, what)
    assert p.obs_final.gx == B and p.obs_final.tpb == lib.TILE, what
    check_launch(p.snap, what)
    assert p.snap.gx <= lib.FLAT_GRID_MAX, what
    # scratch: two stage vectors of B states, then the partial rows, in order and without overlap
    assert (p.ws_x0, p.ws_x1, p.ws_part, p.ws_total) == (0, B * D * 16, 2 * B * D * 16,
                                                         2 * B * D * 16 + p.ws_part_bytes), what
    assert p.ws_part_bytes >= B * p.rows * p.G * lib.OBS_NV * 8 and p.ws_part_bytes % 16 == 0, what
    fits = D <= lib.RES_MAX_D
    assert p.path == ((RESIDENT if fits else STAGED) if path_req == AUTO else path_req), what
    if fits:
        # the resident rule against the LDS planned: regions in order, 16-byte aligned, each as large as its use
        check_launch(p.resident, what, lib.LDS_MAX)
        assert (p.resident.gx, p.resident.tpb) == (B, lib.RES_TPB), what
        offs = (0, p.lds_vec1, p.lds_tab, p.lds_wave, p.lds_tile, p.lds_nbar, p.resident.lds)
        need = (D * 16, D * 16, (1 + M) * nel * nel * 16, (lib.RES_TPB // 64) * lib.OBS_NV * 8,
                tiles * lib.OBS_NV * 8, M * nel * 8)
        assert all(o % 16 == 0 for o in offs), what
        assert all(b - a >= n for a, b, n in zip(offs, offs[1:], need)), (what, offs, need)
        # one tile per partial workgroup, every point owned by one resident thread
        assert p.G == tiles and p.kp * lib.RES_TPB >= d.nvib, what
    else:
        assert path_req != RESIDENT, what


def test_plans_are_legal_and_cover(plan):
    lib = plan
    accepted = refused = 0
    hit_paths = set()
    for nel, dims in itertools.product(range(1, lib.MAX_NEL + 1), dims_lists(lib)):
        D = nel * int(np.prod(dims, dtype=object))
        for B, path_req in itertools.product((1, 3, 65535, 65536), (AUTO, STAGED, RESIDENT)):
            p = plan_of(lib, B, nel, dims, path_req)
            what = (nel, dims, B, path_req)
            if D >= 2 ** 31:
                assert p.refused and p.msg.decode() == f"{FN}: D = nel * prod(dims) must stay below 2^31", what
            elif B > GRID_YZ_MAX:
                assert p.refused and p.msg.decode() == f"{FN}: B={B} outside [1, 65535]", what
            elif path_req == RESIDENT and D > lib.RES_MAX_D:
                assert p.refused and p.msg.decode() == \
                    f"{FN}: the resident path needs D <= {lib.RES_MAX_D} (D = {D})", what
            else:
                assert not p.refused, (what, p.msg)
                check_plan(lib, p, B, nel, dims, path_req, what)
                hit_paths.add((path_req, p.path))
                accepted += 1
                continue
            refused += 1
    assert accepted > 20000 and refused > 10000, (accepted, refused)
    assert hit_paths == {(AUTO, STAGED), (AUTO, RESIDENT), (STAGED, STAGED), (RESIDENT, RESIDENT)}


def test_resident_limit_and_its_neighbours(plan):
    """At the limit the resident LDS fits a CU for every (nel, M); one element past it the plan goes staged."""
    lib = plan
    for nel in range(1, lib.MAX_NEL + 1):
        nv = lib.RES_MAX_D // nel
        for M in range(1, lib.MAX_MODES + 1):
            dims = (1,) * (M - 1) + (nv,)
            p = plan_of(lib, 1, nel, dims)
            assert not p.refused and p.path == RESIDENT and p.resident.lds <= lib.LDS_MAX <= LDS_CU
            check_plan(lib, p, 1, nel, dims, AUTO, (nel, dims))
            q = plan_of(lib, 1, nel, (1,) * (M - 1) + (nv + 1,))
            assert not q.refused and q.path == STAGED
            r = plan_of(lib, 1, nel, (1,) * (M - 1) + (nv + 1,), RESIDENT)
            assert r.refused and r.msg.decode() == \
                f"{FN}: the resident path needs D <= {lib.RES_MAX_D} (D = {nel * (nv + 1)})"
    p = plan_of(lib, 1, 3, (37, 37))          # D = 4107: past the limit, and past the 4096 at which the LDS would still fit
    assert lib.RES_MAX_D == 2048 and p.path == STAGED and p.dev.D == 4107


def test_every_refusal_carries_its_entry_points_message(plan):
    lib = plan
    for fn in ("qd_lvc_apply", "qd_lvc_rk4", "qd_lvc_observe"):
        for kw, msg in ((dict(nel=0), "nel=0 outside [1, 8]"), (dict(nel=9), "nel=9 outside [1, 8]"),
                        (dict(dims=()), "M=0 outside [1, 6]"), (dict(dims=(2,) * 7), "M=7 outside [1, 6]"),
                        (dict(dims=(2, 0, 2)), "dims[1]=0 must be at least 1"),
                        (dict(dims=(2, -3)), "dims[1]=-3 must be at least 1"),
                        (dict(nel=2, dims=(1024, 1024, 1024)), "D = nel * prod(dims) must stay below 2^31"),
                        (dict(nel=1, dims=(2 ** 30, 2)), "D = nel * prod(dims) must stay below 2^31"),
                        (dict(B=0), "B=0 outside [1, 65535]"), (dict(B=65536), "B=65536 outside [1, 65535]"),
                        (dict(path=-1), "path=-1 outside [0, 2]"), (dict(path=3), "path=3 outside [0, 2]"),
                        (dict(nsteps=-1), "nsteps=-1 and save_every=2 must not be negative"),
                        (dict(se=-2), "nsteps=5 and save_every=-2 must not be negative"),
                        (dict(se=0, obs=1), "observables need save_every > 0"),
                        (dict(dims=(37, 37), path=RESIDENT), "the resident path needs D <= 2048 (D = 4107)")):
            args = dict(B=1, nel=3, dims=(4, 4), path=AUTO, nsteps=5, se=2, obs=1)
            args.update(kw)
            p = plan_of(lib, fn=fn, **args)
            assert p.refused and p.msg.decode() == f"{fn}: {msg}", (fn, kw, p.msg)
    p = LvcPlan()
    lib.plan_lvc(b"qd_lvc_apply", 1, 3, 2, None, 0, 0, 0, 0, ctypes.byref(p))
    assert p.refused and p.msg.decode() == "qd_lvc_apply: null dims"
    # admitted at the edges: D = 2^31 - 1 is not reachable with nel >= 1 ints, 2^31 - 2 is; no steps with observables
    assert not plan_of(lib, 1, 2, (2 ** 30 - 1,)).refused
    assert not plan_of(lib, 65535, 8, (1,)).refused
    assert not plan_of(lib, 1, 3, (4, 4), nsteps=0, se=0, obs=1).refused


def test_typed_dispatch_reaches_every_nel(plan):
    lib = plan
    assert [lib.plan_lvc_dispatch(n) for n in range(0, 10)] == [-1, 1, 2, 3, 4, 5, 6, 7, 8, -1]
