"""The any-grid split-operator runs (pyqed_amd/csrc/spo_gen.hip: spo_generic_run, spo1d_generic_run) on the host: the
flat-loop emulation (tools/cpu_emu/emu_spo.cpp) runs the plans of fft_plan.hpp, the pass sequence, the tiles and the
kernels' index arithmetic unchanged, one thread per block, against the oracle restatements of the reference
(oracle/spo.py).  Each axis length picks its own plan (mixed radix, Bluestein, four-step, direct); the grids with
ns = 9 on a 600- / 576-point axis are those whose whole-row tile does not fit the LDS (2 x 9 x 600 x 16 B > 160 KiB),
so the point-operator pass runs unfused around LDS transforms.  Bound: 1e-10 relative (L2), that of
test_spo_anygrid_gpu.py; tests/test_fft_engine_host.py runs the transforms alone through the same library."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT

EMU_DIR = os.path.join(ROOT, "tools", "cpu_emu")
TOL = 1e-10
P = ctypes.c_void_p


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "c++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    so = str(tmp_path_factory.mktemp("emu") / "libemu_spo.so")
    subprocess.run([cxx, "-O1", "-shared", "-fPIC", "-w", "-I", EMU_DIR, os.path.join(EMU_DIR, "emu_spo.cpp"), "-o", so],
                   check=True)
    return ctypes.CDLL(so)


def ptr(a):
    return None if a is None else a.ctypes.data_as(P)


def unitary_ops(shape, ns, rng):
    a = rng.standard_normal(shape + (ns, ns)) + 1j * rng.standard_normal(shape + (ns, ns))
    h = (a + np.conj(np.swapaxes(a, -1, -2))) / 4
    w, u = np.linalg.eigh(h)
    ud = np.conj(np.swapaxes(u, -1, -2))
    return (u * np.exp(-1j * w)[..., None, :]) @ ud, (u * np.exp(-0.5j * w)[..., None, :]) @ ud


def rel(a, b):
    return np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(b), 1e-300)


def nd_inputs(dims, ns, nt, nout, jacobi, seed=0):
    rng = np.random.default_rng(seed)
    shape = tuple(dims)
    eV, eVh = unitary_ops(shape, ns, rng)
    K = np.exp(-1j * rng.uniform(0, 6, shape))
    psi0 = rng.standard_normal(shape + (ns,)) + 1j * rng.standard_normal(shape + (ns,))
    Ky = None
    if jacobi:
        Kx = np.exp(-1j * rng.uniform(0, 6, dims[0]))
        Ky = np.exp(-1j * rng.uniform(0, 6, shape))
        K = np.ascontiguousarray(np.broadcast_to(Kx[:, None], shape))
    return eV, eVh, K, Ky, psi0


def run_nd(lib, dims, ns, nt, nout, merged, inputs):
    """(final state, snapshots [nt // nout]) of emu_spo_nd."""
    eV, eVh, K, Ky, psi0 = inputs
    psi = psi0.copy()
    nsnap = nt // nout
    snap = np.zeros((max(nsnap, 1),) + psi.shape, complex)
    d = (ctypes.c_int * len(dims))(*dims)
    rc = lib.emu_spo_nd(ptr(psi), ptr(eVh), ptr(eV) if merged else None, ptr(K), ptr(Ky), d, len(dims), ns,
                        (nt // nout) * nout, nout, ptr(snap) if nsnap else None)
    assert rc == 0, rc
    return psi, snap[:nsnap]


def check_nd(lib, dims, ns, nt=3, nout=1, merged=False, jacobi=False):
    from oracle import spo as osp
    inputs = nd_inputs(dims, ns, nt, nout, jacobi)
    eV, eVh, K, Ky, psi0 = inputs
    psi, snap = run_nd(lib, dims, ns, nt, nout, merged, inputs)
    if len(dims) == 3:
        ref_snaps, fin = osp.spo3_run(eVh, K, psi0, nt, nout)
    else:
        keo = osp.keo_jacobi(K[:, 0], Ky) if jacobi else osp.keo_linear(K)
        if merged:
            states, fin = osp.spo2_merged_run(eV, eVh, keo, psi0, nt, nout)
        else:
            states, fin = osp.spo2_strang_run(eVh, keo, psi0, nt, nout)
        ref_snaps = states[1:]
    return max([rel(psi, fin)] + [rel(snap[k], ref_snaps[k]) for k in range(len(snap))])


def run_1d(lib, nx, nt, nout, B, seed=0):
    """(x, V, initial states, final states, snapshots [B][nt // nout - 1]) of emu_spo1d."""
    from oracle import spo as osp
    rng = np.random.default_rng(seed)
    x = np.linspace(-8, 8, nx)
    V = 0.5 * x ** 2
    eV, eVh, eK = osp.spo1d_ops(x, V, 1.0, 0.01)
    psi0 = rng.standard_normal((B, nx)) + 1j * rng.standard_normal((B, nx))
    psi = psi0.copy()
    nsnap = max(nt // nout - 1, 0)
    snap = np.zeros((B, max(nsnap, 1), nx), complex)
    rc = lib.emu_spo1d(ptr(psi), ptr(eV), ptr(eVh), ptr(eK), nx, B, nt, nout, ptr(snap) if nsnap else None)
    assert rc == 0, rc
    return x, V, psi0, psi, snap[:, :nsnap]


ND_CASES = [
    ((20, 20), 2, {}), ((96, 80), 2, {}), ((7, 11), 3, {}), ((67, 5), 1, {}), ((12, 10), 5, {}), ((1, 9), 2, {}),
    ((24, 20, 18), 2, dict(nt=2)), ((5, 6, 7), 3, dict(nt=2)),
    ((20, 30), 2, dict(nt=4, nout=2, merged=True)), ((18, 14), 2, dict(nt=4, nout=2, jacobi=True)),
    # the whole row of the mixed-radix last axis does not fit the LDS: unfused point operators, LDS transforms
    ((6, 600), 9, {}), ((3, 576), 9, dict(merged=True)),
    # a direct-DFT axis first (2D, in-place layout) and last (3D)
    ((2579, 3), 2, {}), ((4, 5, 2579), 1, dict(nt=2)),
]


@pytest.mark.parametrize("dims,ns,kw", ND_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else None)
def test_emulated_nd_run_matches_oracle(emu, dims, ns, kw):
    err = check_nd(emu, dims, ns, **kw)
    print(f"host spo {dims} ns {ns} {kw}: rel err {err:.2e}")
    assert err < TOL


# 50, 200: mixed radix; 97, 127: Bluestein; 2048: mixed radix beyond the power-of-two kernels; 6000: four-step;
# 2 x 2053: no plannable split, the direct DFT
@pytest.mark.parametrize("nx,nt,nout,B", [(50, 5, 2, 2), (97, 5, 2, 2), (200, 5, 2, 2), (127, 5, 2, 2),
                                          (2048, 3, 1, 1), (6000, 3, 1, 1), (2 * 2053, 3, 1, 1)])
def test_emulated_1d_run_matches_oracle(emu, nx, nt, nout, B):
    from oracle import spo as osp
    x, V, psi0, psi, snap = run_1d(emu, nx, nt, nout, B)
    err = 0.0
    for b in range(B):
        sl, fin = osp.spo1d_run(x, V, psi0[b], 0.01, nt, nout)
        err = max([err, rel(psi[b], fin)] + [rel(snap[b, k], sl[k]) for k in range(snap.shape[1])])
    print(f"host spo1d {nx}: rel err {err:.2e}")
    assert err < TOL
