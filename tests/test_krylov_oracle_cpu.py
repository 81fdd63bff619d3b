"""oracle/krylov.py, the host restatement of the Arnoldi kernels of pyqed_amd/csrc/krylov.hip, before the kernels are
judged by it (tests/test_krylov_kernels_gpu.py): a whole Arnoldi run satisfies the Arnoldi relation and orthonormality
to the working precision in fp64 and in extended precision, the fp64 and extended single steps agree 100 times inside
the 1e-13 the kernels are held to, and an exact breakdown gives zeros, not NaN."""
import numpy as np
import pytest

from conftest import relerr
from oracle import krylov as ok

assert np.finfo(np.longdouble).eps < 1e-18, "np.longdouble is not an extended format on this host"


def step_case(n, j, seed=0):
    """(V [j + 2, n], z [n], H [j + 2, j + 1]) entering step j: rows < j of V signed unit vectors on a permutation plus
    1e-3 dense noise (orthonormal to ~1e-2: the step is an algebraic map and needs no more), V[j] = u_j with about
    0.14 of its squared norm inside span(V_j) (|s|^2 <= alpha / 4 keeps rho = sqrt(alpha - |s|^2) free of
    cancellation), z dense, H random upper Hessenberg and exactly zero below the sub-diagonal; row j + 1 of V and
    row j and column j of H, which the step writes, hold NaN."""
    rng = np.random.default_rng([seed, n, j])
    cplx = lambda *sh: rng.standard_normal(sh + (2,)).view(np.complex128)[..., 0]
    V = np.full((j + 2, n), np.nan + 1j * np.nan)
    V[:j] = 1e-3 * cplx(j, n)
    V[np.arange(j), rng.permutation(n)[:j]] += rng.choice([-1.0, 1.0, 1j, -1j], j)
    u = cplx(n)
    for _ in range(3):   # outside span(V_j) first, then a known share of it back
        u -= V[:j].T @ (V[:j].conj() @ u)
    if j:
        c = cplx(j)
        u += V[:j].T @ (c * (0.4 * np.linalg.norm(u) / np.linalg.norm(c)))
    V[j] = u
    z = cplx(n)
    H = np.full((j + 2, j + 1), np.nan + 1j * np.nan)
    H[:j + 1, :j] = np.triu(cplx(j + 1, j), -1)
    H[j, :j] = 0.0
    if j:
        H[j, j - 1] = np.nan + 1j * np.nan
    return V, z, H


def step_outputs(Vn, Hn, j):
    """The pieces a step writes: v_j, u_{j+1}, column j, column j - 1 (with h_{j,j-1})."""
    return {"v_j": Vn[j], "u_j+1": Vn[j + 1], "col_j": Hn[:j + 1, j],
            "col_j-1": Hn[:j + 1, j - 1] if j else np.zeros(0, dtype=Hn.dtype)}


def step_errors(got, ref, n, j, z, rho):
    """Normwise relative difference of every piece of step_outputs.  Where the space is exhausted (n = j + 1) u_{j+1}
    is orthogonal to n basis vectors, zero in exact arithmetic and rounding noise otherwise: it is measured against
    ||z|| / rho, the size of the terms that cancel, there."""
    out = {}
    for name in ref:
        if not ref[name].size:
            continue
        if name == "u_j+1" and n == j + 1:
            den = np.linalg.norm(np.asarray(z)) / float(rho)
            out[name] = float(np.linalg.norm((np.asarray(got[name]) - ref[name]).astype(complex)) / den)
        else:
            out[name] = float(relerr(got[name], ref[name]))
    return out


def _arnoldi_run(P, b, m, dtype):
    n = len(b)
    V = np.zeros((m + 2, n), dtype=dtype)
    H = np.zeros((m + 2, m + 1), dtype=dtype)
    V[0] = b
    P = P.astype(dtype)
    for j in range(m + 1):
        V, H, _ = ok.dcgs2_step(V, j, P @ V[j], H, dtype)
    return V, H


@pytest.mark.parametrize("dtype,bound", [(np.complex128, 1e-14), (np.clongdouble, 1e-17)])
def test_dcgs2_run_satisfies_the_arnoldi_relation(dtype, bound):
    """Steps j = 0 .. 80 on a dense P = randn / 20 - 2 I, n = 400: k = 80 final basis vectors and Hessenberg columns.
    Measured: max |V_k^H V_k - I| = 5.8e-16 and ||P V_k - V_{k+1} Hbar_k||_F / ||P||_F = 2.2e-16 in fp64, 8.1e-19 and
    2.1e-19 in extended precision (judged in extended precision both times)."""
    rng = np.random.default_rng(11)
    n, k = 400, 80
    P = (rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))) / 20 - 2.0 * np.eye(n)
    b = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    V, H = _arnoldi_run(P, b, k, dtype)
    V = V.astype(np.clongdouble)
    H = H.astype(np.clongdouble)
    Vk = V[:k]
    orth = np.abs(Vk.conj() @ Vk.T - np.eye(k)).max()
    Pl = P.astype(np.clongdouble)
    arn = np.linalg.norm((Pl @ Vk.T - V[:k + 1].T @ H[:k + 1, :k]).astype(complex)) / np.linalg.norm(P)
    print(f"{np.dtype(dtype).name}: orthogonality {float(orth):.2e}, Arnoldi relation {float(arn):.2e}")
    assert orth < bound and arn < bound
    assert np.all(np.tril(H[:k + 1, :k], -2) == 0)
    sub = np.diag(H[:k + 1, :k], -1)
    assert np.all(sub.imag == 0) and np.all(sub.real > 0)


# the single steps of tests/test_krylov_kernels_gpu.py (what each reaches is said there)
STEP_CASES = [(1, 0), (257, 1), (255, 4), (12293, 8), (12293, 63), (12293, 64), (3077, 127), (3077, 128),
              (12293, 300), (4099, 513), (2051, 1100), (3100, 3073)]


# all of them but the largest, (3100, 3073), which would take the two restatements 8 s on the host
@pytest.mark.parametrize("n,j", STEP_CASES[:-1])
def test_single_step_fp64_against_extended(n, j):
    """The fp64 restatement against the extended one, normwise relative, on the inputs the kernels get.  Measured:
    at most 1.8e-15 over v_j, u_{j+1}, column j and column j - 1 of all cases (u_{j+1} at (12293, 8); 1.5e-15 at
    (2051, 1100), below 1e-15 elsewhere; 8.6e-15 for u_{j+1} of the omitted (3100, 3073), where 27 of 3100
    dimensions are left to it): the reference arithmetic stays 10 to 100 times inside the 1e-13 the kernels are held
    to, and the extended-precision oracle that judges them 2000 times further."""
    V, z, H = step_case(n, j)
    V64, H64, i64 = ok.dcgs2_step(V, j, z, H, np.complex128)
    Vx, Hx, ix = ok.dcgs2_step(V, j, z, H, np.clongdouble)
    assert np.sum(np.abs(ix["s"]) ** 2) <= ix["alpha"] / 4
    got, ref = step_outputs(V64, H64, j), step_outputs(Vx, Hx, j)
    for name, err in step_errors(got, ref, n, j, z, ix["rho"]).items():
        print(f"(n, j) = ({n}, {j}) {name}: {err:.2e}")
        assert err < 1e-14, name
    assert abs(float(i64["rho"] / ix["rho"]) - 1) < 1e-14
    # nothing else moved, and the inputs are untouched
    assert np.array_equal(V64[:j], V[:j]) and np.array_equal(H64[:j, :max(j - 1, 0)], H[:j, :max(j - 1, 0)])
    assert np.isnan(V[j + 1]).all() and np.isnan(H[:j + 1, j]).all()


@pytest.mark.parametrize("dtype", [np.complex128, np.clongdouble])
def test_exact_breakdown_gives_zeros(dtype):
    V, z, H = step_case(300, 5)
    V[5] = 0.0
    z[:] = 0.0
    Vn, Hn, info = ok.dcgs2_step(V, 5, z, H, dtype)
    assert info["rho"] == 0 and Hn[5, 4] == 0
    assert np.all(np.isfinite(Vn)) and np.all(np.isfinite(Hn[:6, :6]))
    assert not Vn[5].any() and not Vn[6].any() and not Hn[:6, 5].any()


def test_project_normalize_and_residual():
    """project and normalize against numpy in fp64; hess_residual is ~eps for numpy's own solution and of order one
    part in the perturbation for a perturbed one; the mpmath summation that stands in where np.longdouble is not an
    extended format gives the same products."""
    rng = np.random.default_rng(2)
    V = rng.standard_normal((5, 300)) + 1j * rng.standard_normal((5, 300))
    w = rng.standard_normal(300) + 1j * rng.standard_normal(300)
    assert relerr(ok.project(V, w).astype(complex), V.conj() @ w) < 1e-15
    assert relerr(ok._matvec_mp(V.conj(), w), ok.project(V, w).astype(complex)) < 1e-15
    nrm, v = ok.normalize(w)
    assert abs(float(nrm) - np.linalg.norm(w)) < 1e-14 * np.linalg.norm(w) and relerr(v.astype(complex), w / np.linalg.norm(w)) < 1e-15
    nrm, v = ok.normalize(np.zeros(7, complex))
    assert nrm == 0 and not v.any()
    k, beta, sft = 40, 1.7, 0.2 + 0.9j
    H = np.triu(rng.standard_normal((k + 1, k + 4)) + 1j * rng.standard_normal((k + 1, k + 4)), -1)
    y = np.linalg.solve(-H[:k, :k] - sft * np.eye(k), beta * np.eye(k)[:, 0])
    assert ok.hess_residual(H, k, beta, sft, y) < 1e-15
    y[3] *= 1 + 1e-6
    assert 1e-10 < ok.hess_residual(H, k, beta, sft, y) < 1e-5
