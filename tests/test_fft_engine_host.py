"""The any-size FFT engine (pyqed_amd/csrc/spo_gen.hip fft_lines) on the host: the flat-loop emulation
(tools/cpu_emu/emu_spo.cpp) compiled with the host C++ compiler runs the engine's planning (fft_plan.hpp; enumerated
on its own by test_fft_plan_host.py) and index arithmetic -- the Stockham stages, Bluestein, the four-step split, the
direct DFT, the column / row tiles -- unchanged, one thread per block.  White noise through every plan class and tile shape of tests/fft_cases.py against
numpy.fft, with the tolerance of the GPU conformance test.  What a serial run cannot show (a missing barrier, an LDS
overrun, device sincospi) is test_fft_conformance_gpu.py's part."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import fft_cases as fc
from conftest import ROOT

EMU_DIR = os.path.join(ROOT, "tools", "cpu_emu")


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "c++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    so = str(tmp_path_factory.mktemp("emu") / "libemu_spo.so")
    subprocess.run([cxx, "-O1", "-shared", "-fPIC", "-w", "-I", EMU_DIR, os.path.join(EMU_DIR, "emu_spo.cpp"), "-o", so],
                   check=True)
    lib = ctypes.CDLL(so)
    lib.emu_fft_lines.restype = ctypes.c_int
    lib.emu_fft_lines.argtypes = [ctypes.c_void_p, ctypes.c_long, ctypes.c_int, ctypes.c_long, ctypes.c_int,
                                  ctypes.POINTER(ctypes.c_int)]
    return lib


def emu_fft(lib, a, inverse):
    """fft_lines along axis 1 of a [O][n][I]; the four-step slot order undone with the returned l2."""
    o, n, i = a.shape
    x = np.ascontiguousarray(a, dtype=complex).copy()
    l2 = ctypes.c_int(-1)
    rc = lib.emu_fft_lines(x.ctypes.data_as(ctypes.c_void_p), o, n, i, int(inverse), ctypes.byref(l2))
    assert rc == 0, rc
    if l2.value:
        l1 = n // l2.value
        k = np.arange(n)
        x = x[:, (k % l1) * l2.value + k // l1, :]
    return x, l2.value


def worst_ratio(lib, cases, seed):
    rng = np.random.default_rng(seed)
    worst = (0.0, 0.0, None)
    for n, o, i in cases:
        a = fc.noise(rng, (o, n, i))
        for inverse in (False, True):
            got, _ = emu_fft(lib, a, inverse)
            r = fc.ratios(got, fc.reference(a, inverse), a, n)
            assert fc.within(*r), (n, o, i, inverse, r)
            if max(r) > max(worst[:2]):
                worst = (r[0], r[1], (n, o, i, inverse))
    return worst


@pytest.mark.parametrize("cls", list(fc.CLASSES))
def test_emulated_engine_by_plan_class(emu, cls):
    cases = [(n, 2, 3) for n in fc.CLASSES[cls]]
    l2r, pbr, at = worst_ratio(emu, cases, seed=11)
    print(f"host {cls}: worst err/tol L2 {l2r:.4f} per-bin {pbr:.4f} at {at}")
    assert at is not None and fc.within(l2r, pbr), at


def test_emulated_engine_dense_sweep(emu):
    l2r, pbr, at = worst_ratio(emu, [(n,) + fc.DENSE_SHAPE for n in fc.DENSE], seed=12)
    print(f"host dense 1..320: worst err/tol L2 {l2r:.4f} per-bin {pbr:.4f} at {at}")
    assert at is not None and fc.within(l2r, pbr), at


def test_emulated_engine_tile_shapes(emu):
    l2r, pbr, at = worst_ratio(emu, fc.shape_cases(), seed=13)
    print(f"host shapes: worst err/tol L2 {l2r:.4f} per-bin {pbr:.4f} at {at}")
    assert at is not None and fc.within(l2r, pbr), at


def test_emulated_engine_length_one_is_identity(emu):
    a = fc.noise(np.random.default_rng(14), (3, 1, 5))
    for inverse in (False, True):
        got, _ = emu_fft(emu, a, inverse)
        assert np.array_equal(got.view(np.int64), a.view(np.int64))


@pytest.mark.parametrize("n,l2", [(5120, 0), (2557, 0), (2579, 0), (5158, 0), (7919, 0), (8192, 128), (5121, 569),
                                  (6499, 97), (5114, 2557), (10201, 101), (12288, 128), (5125, 125), (6000, 80)])
def test_emulated_engine_fourstep_split(emu, n, l2):
    """The split fft_lines reports: natural order (0) for the LDS plans and the direct DFT, L2 = n / L1 with L1 the
    largest divisor <= sqrt(n) whose cofactor is also an LDS plan for the four-step lengths."""
    a = np.zeros((1, n, 1), complex)
    a[0, 1, 0] = 1.0
    _, got = emu_fft(emu, a, False)
    assert got == l2
