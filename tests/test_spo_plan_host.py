"""The dispatch of the power-of-two split-operator path (pyqed_amd/csrc/spo_plan.hpp) on the host: the plan functions,
compiled with the host C++ compiler through tools/cpu_emu/spo_plan_c.cpp, over every shape the specialised kernels can
take.  Nothing of the rules is restated here: the tests enumerate, check that each planned launch is legal and that
the typed dispatch reaches a kernel for it, and compare the set of (family, template values) reached with the set
written below, which is the list of split-operator kernels that exist."""
import ctypes
import itertools
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

EMU_DIR = os.path.join(ROOT, "tools", "cpu_emu")
POW2 = (16, 32, 64, 128, 256, 512, 1024)
LDS_MAX = 160 * 1024


class Pass(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int) for n in ("kind", "L", "C", "NS", "ky", "gx", "gy", "gz", "block", "max_block")] + \
               [("lds", ctypes.c_size_t)]


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "c++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    so = str(tmp_path_factory.mktemp("plan") / "libspo_plan.so")
    subprocess.run([cxx, "-std=c++17", "-O1", "-shared", "-fPIC", "-Wall", "-Werror",
                    os.path.join(EMU_DIR, "spo_plan_c.cpp"), "-o", so], check=True)
    return ctypes.CDLL(so)


def key(lib, p, prefix):
    """(note name, L, C, NS, ky) of a planned pass."""
    buf = ctypes.create_string_buffer(64)
    lib.plan_pass_name(ctypes.byref(p), prefix.encode(), buf, len(buf))
    return (buf.value.decode(), p.L, p.C, p.NS, p.ky)


def legal(lib, p, lines, tiled, what):
    """`lines`: the rows / columns / inner indices the pass covers, `tiled` of them per workgroup."""
    assert 64 <= p.block <= p.max_block <= 1024 and p.block % 64 == 0, (what, p.block, p.max_block)
    assert p.lds <= LDS_MAX, (what, p.lds)
    assert tiled >= 1 and lines % tiled == 0 and p.gx * tiled == lines and p.gy >= 1 and p.gz >= 1, (what, lines, tiled)
    assert lib.plan_dispatch_hits(ctypes.byref(p)) == 1, (what, "dispatch miss")


# Every (family, L, C, NS, ky) the plans return: L the transform length, C the tile width (lines per workgroup; 0: the
# kernel has none), NS the compile-time states (0: run-time ns), ky the compiled-in Jacobi factor.
def _x(name, Ls, Cs=(0,), NSs=(0,), kys=(0,)):
    return {(name if not c else "%s_c%d" % (name, c), l, c, s, k) for l in Ls for c in Cs for s in NSs for k in kys}


SPO2 = (_x("spo2_row_q16", (256,), NSs=(1, 2), kys=(0, 1)) | _x("spo2_row64", (64,), NSs=(1, 2)) |
        _x("spo2_row_fast", (16, 32, 64, 128, 512), NSs=(1, 2)) | _x("spo2_row_fast", (1024,), NSs=(1,)) |
        _x("spo2_row_lds", POW2) |
        _x("spo2_col_q16", (256,), NSs=(1, 2)) |
        _x("spo2_col_fast", (16, 32, 64, 128), (2,), (1, 2)) | _x("spo2_col_fast", (512,), (2,), (1,)) |
        _x("spo2_col_lds", POW2, (1,)) | _x("spo2_col_lds", (16, 32, 64, 128), (2,)))
SPO2_BATCH = (_x("spo2_row_q16", (256,), NSs=(1,)) | _x("spo2_row_wave", (256,), (4,), (2,)) |
              _x("spo2_col_q16", (256,), NSs=(1,)) | _x("spo2_col_tile", (256,), (8,), (2,)))
SPO3 = (_x("spo3_row_q16", (256,), NSs=(1, 2)) | _x("spo3_row64", (64,), NSs=(1, 2)) |
        _x("spo3_row_fast", (16, 32, 128), NSs=(1, 2)) | _x("spo3_row_lds", (16, 32, 64, 128, 256)) |
        _x("spo3_mid_fast", (16, 32), (4, 8, 16)) | _x("spo3_mid64", (64,), (4, 8, 16)) |
        _x("spo3_mid_lds", (128,), (4, 8)) | _x("spo3_mid_lds", (256,), (4,)) |
        _x("spo3_col_q16", (256,), NSs=(1, 2)) |
        _x("spo3_col64", (64,), (4,), (2,)) | _x("spo3_col64", (64,), (8,), (1, 2)) |
        _x("spo3_col_fast", (16, 32, 64, 128), (2,), (1, 2)) | _x("spo3_col_fast", (16, 32), (4,), (2,)) |
        _x("spo3_col_fast", (32,), (8,), (1, 2)) |
        _x("spo3_col_lds", (16, 32, 64, 128), (2,)) | _x("spo3_col_lds", (16, 32, 64), (4,)))
SPO1D = _x("spo1d_lds", POW2)


def test_spo2_plans(plan):
    reached, out = set(), (Pass * 3)()
    for nx, ny, ns, jacobi in itertools.product(POW2, POW2, range(1, 9), (0, 1)):
        if not plan.plan_spo2(nx, ny, ns, jacobi, out):
            continue
        row, rowky, col = out
        for p in (row, rowky):
            legal(plan, p, nx, 16 if p.gx != nx else 1, ("spo2 row", nx, ny, ns, jacobi))
        legal(plan, col, ny, max(col.C, 1), ("spo2 col", nx, ny, ns, jacobi))
        assert rowky.ky in (0, jacobi) and not row.ky
        reached |= {key(plan, p, "spo2") for p in out}
    assert reached == SPO2, (sorted(reached - SPO2), sorted(SPO2 - reached))


def test_spo2_batch_plans(plan):
    reached, out = set(), (Pass * 2)()
    for ns, B, observed in itertools.product((1, 2), (1, 2, 5, 64), (0, 1)):
        assert plan.plan_spo2_batch(256, 256, ns, B, 0, observed, out) == (not observed or B > 1)
        if not plan.plan_spo2_batch(256, 256, ns, B, 0, observed, out):
            continue
        row, col = out
        legal(plan, row, 256, 1, ("batch row", ns, B))
        legal(plan, col, 256, max(col.C, 1), ("batch col", ns, B))
        assert row.gy * max(row.C, 1) >= B and col.gy * col.gz == B * (ns if not col.C else 1)
        reached |= {key(plan, p, "spo2") for p in out}
    assert reached == SPO2_BATCH, (sorted(reached - SPO2_BATCH), sorted(SPO2_BATCH - reached))
    assert not plan.plan_spo2_batch(256, 128, 2, 5, 0, 0, out) and not plan.plan_spo2_batch(256, 256, 3, 5, 0, 0, out)
    assert not plan.plan_spo2_batch(256, 256, 2, 5, 1, 0, out)


def test_spo3_plans(plan):
    reached, out, smallest = set(), (Pass * 3)(), {}
    axes = POW2[:5]
    for nx, ny, nz, ns in itertools.product(axes, axes, axes, range(1, 9)):
        if not plan.plan_spo3(nx, ny, nz, ns, out):
            continue
        row, mid, col = out
        what = (nx, ny, nz, ns)
        legal(plan, row, nx * ny, 16 if row.gx != nx * ny else 1, ("spo3 row",) + what)
        legal(plan, mid, nx * nz * ns, mid.C, ("spo3 mid",) + what)
        legal(plan, col, ny * nz, max(col.C, 1), ("spo3 col",) + what)
        for p in out:
            k = key(plan, p, "spo3")
            reached.add(k)
            smallest[k] = min(smallest.get(k, (1 << 40,)), (nx * ny * nz * ns,) + what)
    assert reached == SPO3, (sorted(reached - SPO3), sorted(SPO3 - reached))
    for k in sorted(smallest):
        print("smallest shape for %-34s %s" % (k, smallest[k][1:]))
    for nx, ny, nz in itertools.product((512, 1024), axes, axes):   # no axis above 256 in 3D
        assert not plan.plan_spo3(nx, ny, nz, 1, out) and not plan.plan_spo3(nz, ny, nx, 1, out)


def test_spo1d_plans(plan):
    reached, p = set(), Pass()
    for nx in POW2:
        assert plan.plan_spo1d(nx, 3, ctypes.byref(p))
        legal(plan, p, 3, 1, ("spo1d", nx))
        reached.add(key(plan, p, "spo1d"))
    assert reached == SPO1D
    for nx in (8, 24, 100, 2048):
        assert not plan.plan_spo1d(nx, 3, ctypes.byref(p))


def test_unplanned_passes_miss_the_dispatch(plan):
    """A pass no plan returns reaches no kernel: the dispatch reports the miss instead of launching nothing."""
    out = (Pass * 3)()
    assert plan.plan_spo3(64, 64, 64, 2, out)
    for field, value in (("L", 48), ("L", 2048), ("C", 3), ("kind", 99)):
        p = Pass.from_buffer_copy(out[1])
        setattr(p, field, value)
        assert plan.plan_dispatch_hits(ctypes.byref(p)) == 0, (field, value)
    col = Pass.from_buffer_copy(out[2])
    col.C = 2   # col64 exists for the tiles the 3D rule gives, not for two columns
    assert plan.plan_dispatch_hits(ctypes.byref(col)) == 0
