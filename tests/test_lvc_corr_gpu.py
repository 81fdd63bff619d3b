"""LVCSolver.correlation_3op_1t / _2t and correlation_4op_1t / _2t on the GPU, matrix-free (qd_lvc_apply for c and a^+,
qd_lvc_pair_rk4 for the propagation and the one block of b): against the reference's own results
(tests/golden/lvc_corr.npz) at the 1e-11 tests/test_tdse_corr_gpu.py holds the dense path to; LVCOp operands against the
same call with .toarray() operands on the inherited dense path, at D = 36 (pair resident) and at (3; 12, 10, 8), D = 2880
(pair staged; the dense H is 132 MB), to 1e-12 relative, both being the same Horner RK4 in float64; row 0 of the 2t
function is the 1t one; the 2t call in chunks of pairs equals the call in one chunk bit for bit; and one call at
(3; 16, 16, 16, 16), D = 196 608, where a dense H would be 618 GB."""
import numpy as np
import pytest

from conftest import relerr
from test_lvc_pair_host import golden_model

pytestmark = pytest.mark.gpu
TOL_REF = 1e-11
TOL_DENSE = 1e-12


def _model(trunc):
    from pyqed_amd import LVC, Mode
    modes = [Mode(0.074 + 0.02 * j, [[[1, 1], -0.05 + 0.02 * j], [[2, 2], 0.06 - 0.01 * j]] +
                  ([[[1, 2], 0.08]] if j == len(trunc) - 1 else []), truncate=n) for j, n in enumerate(trunc)]
    mol = LVC([0.0, 0.5, 0.62], modes)
    mol.add_coupling([[0, 1], 0.01])
    return mol


def _state(mol, seed=5):
    rng = np.random.default_rng(seed)
    psi = rng.standard_normal(mol.dim) + 1j * rng.standard_normal(mol.dim)
    return psi / np.linalg.norm(psi)


def _ops(mol):
    """[a, b, c] and [a, b, c, d]: a non-Hermitian electronic factor, a Herzberg-Teller factor A (x) x_j, a coordinate,
    a bare [nel, nel] array."""
    rng = np.random.default_rng(3)
    A = rng.standard_normal((mol.nel, mol.nel)) + 1j * rng.standard_normal((mol.nel, mol.nel))
    ht = mol.promote(A, "el") @ mol.coordinate(mol.nmodes - 1)
    ops3 = [mol.promote(A, "el"), mol.coordinate(0), ht]
    ops4 = [ht, mol.buildop(1, 2), mol.coordinate(mol.nmodes - 1), mol.promote(A.T.copy(), "el")]
    return ops3, ops4


@pytest.mark.parametrize("path", ["auto", "staged"])
def test_against_the_reference_fixture(path):
    mol, ops3, ops4, g = golden_model()
    sol = mol.wavepacket_dynamics()
    dt, Nt, Ntau, psi0 = float(g["dt"]), int(g["Nt"]), int(g["Ntau"]), g["psi0"]
    got = {"c3_1t": sol.correlation_3op_1t(psi0, ops3, dt, Ntau, path=path),
           "c3_2t": sol.correlation_3op_2t(psi0, ops3, dt, Nt, Ntau, path=path),
           "c4_1t": sol.correlation_4op_1t(psi0, ops4, dt, Ntau, path=path),
           "c4_2t": sol.correlation_4op_2t(psi0, ops4, dt, Nt, Ntau, path=path)}
    errs = {k: relerr(v, g[k]) for k, v in got.items()}
    print(f"lvc corr fixture {path}: " + ", ".join(f"{k} {e:.2e}" for k, e in errs.items()))
    assert all(v.shape == g[k].shape for k, v in got.items())
    assert all(e < TOL_REF for e in errs.values()), errs
    assert mol.H is None    # no H was needed


@pytest.mark.parametrize("trunc,noted", [((4, 3), "lvc_pair_resident"), ((12, 10, 8), "lvc_pair_staged")])
def test_factors_against_the_dense_path(trunc, noted):
    from pyqed_amd import _lib
    mol = _model(trunc)
    sol = mol.wavepacket_dynamics()
    psi0 = _state(mol)
    ops3, ops4 = _ops(mol)
    d3, d4 = [o.toarray() for o in ops3], [o.toarray() for o in ops4]
    dt, Nt, Ntau = 0.02, 3, 4
    _lib.take_path()
    c31 = sol.correlation_3op_1t(psi0, ops3, dt, Ntau)
    assert noted in _lib.take_path()
    pairs = {"c3_1t": (c31, sol.correlation_3op_1t(psi0, d3, dt, Ntau)),
             "c3_2t": (sol.correlation_3op_2t(psi0, ops3, dt, Nt, Ntau), sol.correlation_3op_2t(psi0, d3, dt, Nt, Ntau)),
             "c4_1t": (sol.correlation_4op_1t(psi0, ops4, dt, Ntau), sol.correlation_4op_1t(psi0, d4, dt, Ntau)),
             "c4_2t": (sol.correlation_4op_2t(psi0, ops4, dt, Nt, Ntau),
                       sol.correlation_4op_2t(psi0, d4, dt, Nt, Ntau))}
    errs = {k: relerr(a, b) for k, (a, b) in pairs.items()}
    print(f"lvc corr {trunc}: " + ", ".join(f"{k} {e:.2e}" for k, e in errs.items()))
    assert pairs["c3_2t"][0].shape == (Nt, Ntau) and pairs["c4_1t"][0].shape == (Ntau,)
    assert all(np.abs(a).max() > 1e-3 for a, _ in pairs.values())   # not a comparison of zeros
    assert all(e < TOL_DENSE for e in errs.values()), errs
    # a bare [nel, nel] array is A (x) 1; an LVCOp beside a D x D operand goes to the dense path as it is
    bare = sol.correlation_3op_1t(psi0, [ops3[0].A, ops3[1], ops3[2]], dt, Ntau)
    assert np.array_equal(bare, c31)
    mixed = sol.correlation_3op_1t(psi0, [ops3[0], d3[1], ops3[2]], dt, Ntau)
    assert np.array_equal(mixed, pairs["c3_1t"][1])


def test_two_time_rows_and_chunks():
    """Row 0 of correlation_3op_2t is correlation_3op_1t; pairs in chunks of 2 (the last chunk holds 1) equal the pairs
    in one chunk bit for bit, on both paths."""
    mol = _model((5, 4))
    sol = mol.wavepacket_dynamics()
    psi0 = _state(mol)
    ops3, ops4 = _ops(mol)
    dt, Nt, Ntau = 0.02, 5, 3
    for path in ("resident", "staged"):
        one = sol.correlation_3op_2t(psi0, ops3, dt, Nt, Ntau, path=path, _chunk=Nt)
        assert np.array_equal(one[0], sol.correlation_3op_1t(psi0, ops3, dt, Ntau, path=path))
        assert np.array_equal(one, sol.correlation_3op_2t(psi0, ops3, dt, Nt, Ntau, path=path, _chunk=2))
        assert np.array_equal(one, sol.correlation_3op_2t(psi0, ops3, dt, Nt, Ntau, path=path))
        four = sol.correlation_4op_2t(psi0, ops4, dt, Nt, Ntau, path=path, _chunk=Nt)
        assert np.array_equal(four, sol.correlation_4op_2t(psi0, ops4, dt, Nt, Ntau, path=path, _chunk=1))
        assert np.array_equal(four[0], sol.correlation_4op_1t(psi0, ops4, dt, Ntau, path=path))


def test_a_size_no_dense_path_could_hold():
    """(3; 16, 16, 16, 16), D = 196 608: the dipole correlation <mu(t) mu(0)> and a coordinate one run, are finite, and
    start at <psi0| a b c |psi0>."""
    mol = _model((16, 16, 16, 16))
    assert mol.dim == 196608
    sol = mol.wavepacket_dynamics()
    psi0 = _state(mol)
    mu, x = mol.buildop(0, 1), mol.coordinate(2)
    for ops in ([mol.promote(np.eye(3), "el"), mu, mu], [mu, x, mu]):
        c = sol.correlation_3op_1t(psi0, ops, 0.02, 4)
        start = np.vdot(psi0, ops[0].dot(ops[1].dot(ops[2].dot(psi0))))
        print(f"lvc corr D={mol.dim}: c[0] {c[0]:.6f}, |c[0] - <a b c>| {abs(c[0] - start):.2e}")
        assert c.shape == (4,) and np.all(np.isfinite(c)) and abs(start) > 1e-3
        assert abs(c[0] - start) < 1e-12 * max(1.0, abs(start))
        assert np.abs(c[1:] - c[0]).max() > 1e-6    # it moves
    assert mol.H is None
