"""oracle/response.py earns its role on the host: the closed-form reference of the 2DES response kernels against the
reference implementation's recorded outputs (tests/golden: corr4_ensemble slices and sum, the three corr4_3level cubes,
the deom_corr4 frequency grids) and against a 1 x 1 case written out by hand.  The eigen factors are host setup
(numpy / scipy eig); no GPU, no library call."""
import numpy as np
import pytest

from conftest import load_golden, relerr
from oracle import response as orr

TOL = 1e-10     # the bound the GPU tests of the same fixtures use (tests/test_redfield_response_gpu.py)


def test_extended_precision_available():
    """The oracle's default working precision is the 80-bit long double; where np.longdouble is float64 the GPU
    edge tests would compare float64 with float64, and this refuses to pass."""
    assert orr.EXTENDED_OK
    assert np.finfo(np.longdouble).eps < 1.1e-19


def test_one_by_one_by_hand():
    """M = 1, one eigenvalue, one grid point: S = i alpha e^{lam t3} Mt beta e^{lam t1}; scale the moduli; the
    scan adds B e^{lam t2} C in place of Mt; the resolvent grid is a product of two fractions."""
    lam, alpha, mt, beta = -0.1 + 2.0j, 0.5 - 1.5j, 2.0 + 0.25j, -1.0 + 0.5j
    t3, t1, t2 = 3.0, 4.5, 0.75
    want = 1j * alpha * np.exp(lam * t3) * mt * beta * np.exp(lam * t1)
    mod = abs(alpha) * np.exp(-0.1 * t3) * abs(mt) * abs(beta) * np.exp(-0.1 * t1)
    L, A, Mt, Bt = (np.array(x, complex).reshape(s) for x, s in ((lam, (1, 1)), (alpha, (1, 1)), (mt, (1, 1, 1)),
                                                                  (beta, (1, 1))))
    S, sc = orr.ensemble_slice(L, A, Mt, Bt, L, [t3], [t1])
    assert S.shape == sc.shape == (1, 1) and S.dtype == np.complex128 and sc.dtype == np.float64
    assert abs(S[0, 0] - want) < 4e-16 * abs(want)
    assert abs(sc[0, 0] - mod) < 4e-16 * mod
    assert abs(abs(S[0, 0]) - sc[0, 0]) < 4e-16 * mod         # one term: |S| is the scale
    b, c = 0.3 + 0.7j, -1.25 + 0.5j
    S2, sc2 = orr.t2_scan(L, A, np.full((1, 1, 1), b), L, np.full((1, 1, 1), c), Bt, L, [t3], [0.0, t2], [t1])
    for j, tj in enumerate([0.0, t2]):
        w = 1j * alpha * np.exp(lam * t3) * b * np.exp(lam * tj) * c * beta * np.exp(lam * t1)
        assert abs(S2[j, 0, 0] - w) < 4e-16 * abs(w)
        assert abs(sc2[j, 0, 0] - abs(w)) < 4e-16 * abs(w)
    a, m, v, wx, wy = 1.5 - 0.5j, mt, 0.25 + 1.0j, 0.7, -1.9
    R, scr = orr.resolvent_grid([a], [[m]], [v], [lam], [wx], [wy])
    w = a / (-lam - 1j * wx) * m * v / (-lam - 1j * wy)
    assert abs(R[0, 0] - w) < 4e-16 * abs(w) and abs(scr[0, 0] - abs(w)) < 4e-16 * abs(w)


def test_rows_cols_and_float64_agree_with_full_extended():
    """rows / cols pick whole rows and columns of the full grid; the float64 pairwise form agrees with the
    extended one to a few eps of the scale."""
    rng = np.random.default_rng(2)
    M, nx, nz = 7, 5, 3
    lx = -rng.uniform(0.01, 0.2, (M, nx)) + 1j * rng.uniform(-2, 2, (M, nx))
    lz = -rng.uniform(0.01, 0.2, (M, nz)) + 1j * rng.uniform(-2, 2, (M, nz))
    al = rng.standard_normal((M, nx)) + 1j * rng.standard_normal((M, nx))
    be = rng.standard_normal((M, nz)) + 1j * rng.standard_normal((M, nz))
    Mt = rng.standard_normal((M, nx, nz)) + 1j * rng.standard_normal((M, nx, nz))
    t3, t1 = 3.7 + 0.5 * np.arange(21), 1.3 + 0.25 * np.arange(18)
    S, sc = orr.ensemble_slice(lx, al, Mt, be, lz, t3, t1)
    rows, cols = [0, 5, 20], [17, 3]
    Ss, scs = orr.ensemble_slice(lx, al, Mt, be, lz, t3, t1, rows=rows, cols=cols)
    assert np.array_equal(Ss, S[np.ix_(rows, cols)]) and np.array_equal(scs, sc[np.ix_(rows, cols)])
    S64, sc64 = orr.ensemble_slice(lx, al, Mt, be, lz, t3, t1, dtype=np.complex128)
    # float64: two exponentials with |lam| t <= 2.01 * 14 ulps of phase each, nx + nz + log2 M additions
    assert orr.entry_error(S64, S, sc) < (2 * 2.01 * 14 + nx + nz + 8) * 2.3e-16
    assert np.all(np.abs(S) <= sc * (1 + 1e-15))
    assert relerr(sc64, sc) < 1e-15


def _ensemble_inputs(E_list, t2):
    from pyqed_amd.response import ensemble_factors, redfield_superop_batch
    from pyqed_amd.superoperator import operator_to_superoperator
    dip = np.zeros((3, 3)); dip[0, 1] = dip[1, 0] = dip[1, 2] = dip[2, 1] = 1.0
    rho0 = np.zeros((3, 3), complex); rho0[0, 0] = 1
    E = np.asarray(E_list)
    R = redfield_superop_batch(E, np.diag([0.0, 1.0, 2.0]), np.full((len(E), 3, 3), 0.05))
    lam, U1 = np.linalg.eig(R)
    U2 = np.linalg.inv(U1)
    ops = [operator_to_superoperator(dip, s).toarray() for s in "lccc"]
    return lam, ensemble_factors(lam, U1, U2, ops, rho0.flatten(), t2)


def test_ensemble_slice_matches_recorded_slices_and_sum():
    g = load_golden("corr4_ensemble")
    tau = g["tau"]
    lam, (alpha, Mt, beta) = _ensemble_inputs(g["E"], tau[int(g["j"])])
    for m in range(len(g["E"])):
        S, sc = orr.ensemble_slice(lam[m:m + 1], alpha[m:m + 1], Mt[m:m + 1], beta[m:m + 1], lam[m:m + 1], tau, tau)
        assert relerr(S, g["slices"][m]) < TOL, m
        assert np.all(np.abs(S) <= sc * (1 + 1e-15))
    S, _ = orr.ensemble_slice(lam, alpha, Mt, beta, lam, tau, tau)
    assert relerr(S, g["ens_sum"]) < TOL
    sub, _ = orr.ensemble_slice(lam, alpha, Mt, beta, lam, tau, tau, rows=[31, 0], cols=[7])
    assert relerr(sub, g["ens_sum"][np.ix_([31, 0], [7])]) < TOL


@pytest.mark.parametrize("sig", ["lccc", "llll", "lrlr"])
def test_t2_scan_matches_recorded_cubes(sig):
    from pyqed_amd.response import eigen_factors, sos_eig
    g = load_golden("corr4_3level")
    lam, U1, U2 = sos_eig(g["R"])
    tau = g["tau16"]
    alpha, B, C, beta = eigen_factors(lam, U1, U2, [g["dip"]] * 4, sig, g["rho0"])
    L = lam[None]
    S, sc = orr.t2_scan(L, alpha[None], B[None], L, C[None], beta[None], L, tau, tau, tau)
    assert S.shape == (16, 16, 16)
    assert relerr(S.transpose(1, 0, 2), g["cube_" + sig]) < TOL          # the cube is [t3, t2, t1]
    assert np.all(np.abs(S) <= sc * (1 + 1e-15))


@pytest.mark.parametrize("lcr", ["llll", "lrlr", "lccc"])
def test_resolvent_grid_matches_recorded_deom_grids(lcr):
    """The recorded DEOM propagator's eigen form (host setup of DEOMSolver.correlation_4op_3t, if_full=True) through
    resolvent_grid against the reference's c_w grids."""
    import scipy.linalg as la
    from pyqed_amd.deom import _action_block
    g = load_golden("deom_corr4")
    sx = g["Q"][0]
    ns, nmax = 2, int(g["nmax"])
    n2 = ns * ns
    lam, V = la.eig(g["propagator"])
    Vi = la.pinv(V)
    A1, A2, A3, A4 = (_action_block(sx, c) for c in (lcr[3], lcr[2], lcr[1], lcr[0]))
    act = lambda b, X: np.einsum('xy,ayp->axp', b, X.reshape(nmax, n2, -1)).reshape(nmax * n2, -1)
    diag = np.arange(ns) * (ns + 1)
    a = (A1 @ V[:n2])[diag].sum(axis=0)
    M = (Vi @ act(A2, V)) @ (np.exp(lam * float(g["T"]))[:, None] * (Vi @ act(A3, V)))
    v = Vi[:, :n2] @ (A4 @ np.asarray(g["rho0"], dtype=complex).flatten())
    S, sc = orr.resolvent_grid(a, M, v, lam, g["wx"], g["wy"])
    assert S.shape == (len(g["wx"]), len(g["wy"]))
    assert relerr(S, g["cw_" + lcr]) < TOL
    assert np.all(np.abs(S) <= sc * (1 + 1e-15))
