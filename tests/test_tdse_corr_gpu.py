"""SESolver multi-time correlation functions and propagator (qd_tdse_pair_corr, qd_tdse_rk4) vs the reference's
own results (tests/golden/sesolver_corr.npz, written by tests/golden/make_golden_sescorr.py) and vs a NumPy RK4."""
import functools

import numpy as np
import pytest

from conftest import load_golden, relerr

pytestmark = pytest.mark.gpu
TOL = 1e-11


def _case(tag):
    g = load_golden("sesolver_corr")
    return (g[f"{tag}_H"], list(g[f"{tag}_ops"]), g[f"{tag}_psi0"], float(g[f"{tag}_dt"]), int(g[f"{tag}_Nt"]),
            int(g[f"{tag}_Ntau"]), g)


@pytest.mark.parametrize("tag", ["a", "b", "c"])
def test_correlations_vs_reference(tag):
    """All four correlation methods against the reference (mol.py:1475-1566); case b has a non-Hermitian H, case c
    is the smallest legal call (Nt = Ntau = 1)."""
    from pyqed_amd.mol import SESolver
    H, ops, psi0, dt, Nt, Ntau, g = _case(tag)
    sol = SESolver(H)
    got = {"c3_1t": sol.correlation_3op_1t(psi0, ops[:3], dt, Ntau),
           "c3_2t": sol.correlation_3op_2t(psi0, ops[:3], dt, Nt, Ntau),
           "c4_1t": sol.correlation_4op_1t(psi0, ops, dt, Ntau),
           "c4_2t": sol.correlation_4op_2t(psi0, ops, dt, Nt, Ntau)}
    for k, v in got.items():
        ref = g[f"{tag}_{k}"]
        assert v.shape == ref.shape, k
        assert np.iscomplexobj(v), k
        err = relerr(v, ref)
        print(tag, k, f"relerr {err:.3e}")
        assert err < TOL, (k, err)


def test_correlations_accept_sparse_operators():
    """H and the operators go through to_numpy: scipy sparse inputs give the dense result."""
    from scipy.sparse import csr_matrix
    from pyqed_amd.mol import SESolver
    H, ops, psi0, dt, Nt, Ntau, g = _case("b")
    got = SESolver(csr_matrix(H)).correlation_4op_2t(psi0, [csr_matrix(o) for o in ops], dt, Nt, Ntau)
    assert relerr(got, g["b_c4_2t"]) < TOL


def test_propagator_vs_reference():
    """SESolver.propagator (mol.py:1468-1470, 1569-1600): [I, I, R, R^2, R^3] for Nt = 4."""
    from pyqed_amd.mol import SESolver
    H, ops, psi0, dt, Nt, Ntau, g = _case("b")
    U = SESolver(H).propagator(dt, int(g["b_prop_Nt"]))
    ref = g["b_prop"]
    N = H.shape[0]
    assert isinstance(U, list) and len(U) == 5 == len(ref)
    assert np.array_equal(U[0], np.eye(N)) and np.array_equal(U[1], np.eye(N))
    for k in range(5):
        assert U[k].shape == (N, N)
        err = relerr(U[k], ref[k])
        print("propagator", k, f"relerr {err:.3e}")
        assert err < TOL, (k, err)


# ---------------------------------------------------------------- the library call on both dispatch paths
def _pair_problem(N, B, ntau, hermitian=True):
    """Inputs and the NumPy result (oracle.tdse._rk4 per state), read-only; the small shapes, which several tests
    share, are computed once (the large ones are used once and are not kept)."""
    make = _make_pair_problem_cached if N <= 600 else _make_pair_problem
    return make(N, B, ntau, hermitian)


def _make_pair_problem(N, B, ntau, hermitian):
    from oracle import tdse as otd
    rng = np.random.default_rng(1000 * N + B)
    gin = lambda: (rng.standard_normal((N, N)) + 1j * rng.standard_normal((N, N))) / np.sqrt(N)  # noqa: E731
    H = gin()
    H = (H + H.conj().T) / 2
    if not hermitian:
        H = H - 0.5j * np.diag(rng.uniform(0.0, 0.3, N))
    A, Bop, C = gin(), gin(), gin()
    psi = rng.standard_normal((B, N)) + 1j * rng.standard_normal((B, N))
    psi /= np.linalg.norm(psi, axis=1, keepdims=True)
    dt = 0.02
    ref = np.zeros((B, ntau), complex)
    for b in range(B):
        ket, bra = C @ psi[b], A.conj().T @ psi[b]
        for j in range(ntau):
            if j:
                ket, bra = otd._rk4(ket, H, dt), otd._rk4(bra, H, dt)
            ref[b, j] = np.vdot(bra, Bop @ ket)
    for a in (H, A, Bop, C, psi, ref):
        a.setflags(write=False)
    return H, A, Bop, C, psi, dt, ref


_make_pair_problem_cached = functools.lru_cache(maxsize=None)(_make_pair_problem)


def _run_pair(H, A, Bop, C, psi, dt, ntau):
    import torch
    from pyqed_amd.mol import tdse_pair_corr
    dev = torch.device("cuda", 0)
    t = lambda a: torch.from_numpy(np.array(a)).to(dev)  # noqa: E731  (a copy: the cached inputs are read-only)
    psi_d = t(psi)
    corr = tdse_pair_corr(t(H), t(A), t(Bop), t(C), psi_d, dt, ntau)
    return corr.cpu().numpy(), psi_d.cpu().numpy()


@pytest.mark.parametrize("N,B,ntau,path", [(300, 3, 4, "tdse_pair_rows"), (256, 64, 3, "tdse_pair_rows"),
                                           (256, 87, 3, "tdse_pair_rows"), (256, 88, 3, "tdse_pair_gemm"),
                                           (512, 31, 3, "tdse_pair_rows"), (512, 32, 3, "tdse_pair_gemm"),
                                           (1024, 15, 3, "tdse_pair_rows"), (1024, 16, 3, "tdse_pair_gemm"),
                                           (2048, 8, 2, "tdse_pair_rows"), (2048, 9, 2, "tdse_pair_gemm"),
                                           (600, 70, 3, "tdse_pair_gemm")])
def test_pair_corr_paths_vs_numpy(N, B, ntau, path):
    """qd_tdse_pair_corr on the row path (N = 300: no multiple of 4 or 64) and on the MFMA GEMM path (N = 600,
    B = 70 pads both dimensions to multiples of 128) against a NumPy RK4 of every ket and bra.

    Measurement (tools/tdse_corr_bench.py) moved the pair dispatch away from the plain run's thresholds: the GEMM
    stages run when (N >= 2048 and 2B >= 18) or (N >= 1024 and 2B >= 32) or (N >= 512 and 2B >= 64) or
    (N >= 256 and 2B >= 176).  So the (256, 64) shape, 128 states, is a row-path case now, and the shapes are the
    smallest on each side of every threshold: (256, 87 | 88), (512, 31 | 32), (1024, 15 | 16), (2048, 8 | 9).
    (256, 88) and (1024, 16) keep their kets in one 128-row block inside a 256- and a 128-row state, the two
    layouts of the cross GEMM."""
    from conftest import took
    H, A, Bop, C, psi, dt, ref = _pair_problem(N, B, ntau)
    took("")
    corr, _ = _run_pair(H, A, Bop, C, psi, dt, ntau)
    hit, got = took(path)
    assert hit, got
    assert corr.shape == (B, ntau)
    err = relerr(corr, ref)
    print(N, B, ntau, path, f"relerr {err:.3e}")
    assert err < TOL, err
    # every wavefunction on its own, so one wrong row cannot hide in the norm of the rest
    worst = max(relerr(corr[b], ref[b]) for b in range(B))
    assert worst < TOL, worst


def test_pair_corr_nonhermitian_rows():
    """Non-Hermitian H (nothing derived by conjugation) on the row path at a tiny N with more than one block of
    64 columns in the bra start-up product (N = 70)."""
    H, A, Bop, C, psi, dt, ref = _pair_problem(70, 5, 4, hermitian=False)
    corr, _ = _run_pair(H, A, Bop, C, psi, dt, 4)
    assert relerr(corr, ref) < TOL


@pytest.mark.parametrize("N,B", [(256, 64), (256, 88)])
def test_pair_corr_invariants(N, B):
    """psi is read only, two calls agree bit for bit (no atomics), and the j = 0 column is
    <psi_b| A Bop C |psi_b>: at (N, B) = (256, 64), which the moved dispatch sends down the row path, and at
    (256, 88), the smallest GEMM-path shape at that N."""
    H, A, Bop, C, psi, dt, ref = _pair_problem(N, B, 3)
    c1, psi_after = _run_pair(H, A, Bop, C, psi, dt, 3)
    c2, _ = _run_pair(H, A, Bop, C, psi, dt, 3)
    assert np.array_equal(psi_after.view(np.float64), psi.view(np.float64))
    assert np.array_equal(c1.view(np.float64), c2.view(np.float64))
    M = A @ Bop @ C
    c0 = np.einsum("bi,ij,bj->b", psi.conj(), M, psi)
    assert relerr(c1[:, 0], c0) < 1e-12


def test_method_consistency():
    """Case a: the t = 0 row of correlation_3op_2t is correlation_3op_1t over tau, and correlation_4op_2t is
    correlation_3op_2t with [a, b @ c, d]."""
    from pyqed_amd.mol import SESolver
    H, ops, psi0, dt, Nt, Ntau, g = _case("a")
    sol = SESolver(H)
    c32 = sol.correlation_3op_2t(psi0, ops[:3], dt, Nt, Ntau)
    c31 = sol.correlation_3op_1t(psi0, ops[:3], dt, Ntau)
    assert relerr(c32[0], c31) < 1e-12
    c42 = sol.correlation_4op_2t(psi0, ops, dt, Nt, Ntau)
    c32b = sol.correlation_3op_2t(psi0, [ops[0], ops[1] @ ops[2], ops[3]], dt, Nt, Ntau)
    assert np.array_equal(c42, c32b)
