"""LVC pair records and correlation functions on the host (no GPU): the pair record of tests/lvc_pair_models.py against
<bra| kron(A, .. x_j ..) |ket> from Kronecker products; the restated correlation functions against a dense-H RK4 and
against the reference's own results (tests/golden/lvc_corr.npz); the float64 restatement against the long-double one on
every case of tests/test_lvc_pair_kernels_gpu.py (what the 1e-12 of that test leaves to the kernels); every refusal of
the class surface, the NotImplementedError included, and of the C entries' argument checks that needs no device."""
import ctypes
import functools
import os
import tempfile

import numpy as np
import pytest

import lvc_models as lm
import lvc_pair_models as pm
from conftest import ROOT, relerr
from oracle import highprec as hp
from test_lvc_pair_plan_host import build_pair_plan_lib

GOLDEN = os.path.join(ROOT, "tests", "golden", "lvc_corr.npz")
SMALL = [(1, (3,)), (2, (3, 4)), (3, (2, 2, 2)), (3, (1, 4, 1)), (4, (2, 3)), (5, (3, 2))]


@pytest.mark.parametrize("nel,dims", SMALL)
def test_pair_record_against_kronecker_operators(nel, dims):
    """tr(A R_r) = <bra| A (x) (1 | x_j) |ket> for a random complex A and every block, and each entry of R_r is the
    matrix element of the jump |b><a|."""
    rng = np.random.default_rng(7)
    pairs = pm.random_pairs(2, nel, dims)
    M = len(dims)
    blocks = list(range(1 + M))
    dtypes = (np.complex128, np.clongdouble) if hp.EXTENDED_OK else (np.complex128,)
    for dtype in dtypes:
        R = pm.pair_record(pairs, nel, dims, blocks, dtype).astype(complex)
        assert R.shape == (2, 1 + M, nel, nel)
        A = rng.standard_normal((nel, nel)) + 1j * rng.standard_normal((nel, nel))
        for r in blocks:
            op = pm.factor_dense((A, r), nel, dims)
            want = np.array([np.vdot(p[1], op @ p[0]) for p in pairs])
            got = np.einsum("ab,Pba->P", A, R[:, r])
            assert np.abs(got - want).max() < 1e-14, (dtype, r, np.abs(got - want).max())
            for a in range(nel):
                for b in range(nel):
                    J = np.zeros((nel, nel))
                    J[b, a] = 1.0
                    want = np.array([np.vdot(p[1], pm.factor_dense((J, r), nel, dims) @ p[0]) for p in pairs])
                    assert np.abs(R[:, r, a, b] - want).max() < 1e-14
    # with bra = ket the blocks are the rho and X parts of the observable record
    same = np.stack([pairs[:, 0], pairs[:, 0]], axis=1)
    rec = lm.record(pairs[:, 0], nel, dims)[:, :nel * nel * (1 + M)].reshape(2, 1 + M, nel, nel)
    assert np.array_equal(pm.pair_record(same, nel, dims, blocks), rec)


def _facs(nel, M, rng, blocks):
    return [(rng.standard_normal((nel, nel)) + 1j * rng.standard_normal((nel, nel)), r) for r in blocks]


@pytest.mark.parametrize("nel,dims", [(2, (3, 4)), (3, (2, 2, 2)), (3, (3, 3))])
def test_correlation_restatements_against_dense_propagation(nel, dims):
    """All four functions, non-Hermitian model and operators, coordinate factors in every position."""
    rng = np.random.default_rng(11)
    M = len(dims)
    omega, Hel, W = lm.random_model(nel, dims)
    psi0 = lm.random_states(1, nel, dims)[0]
    dt = 0.5 / lm.h_bound(dims, omega, Hel, W)
    H = lm.dense_h(nel, dims, omega, Hel, W)
    Nt, Ntau = 3, 5
    for blocks in ((0, 0, 0), (1, M, 0), (0, 1, M), (M, 0, 1)):
        facs = _facs(nel, M, rng, blocks)
        ops = [pm.factor_dense(f, nel, dims) for f in facs]
        psi_t = pm.dense_states_t(H, psi0, dt, Nt)
        ref = pm.dense_corr_3op(H, psi_t, ops, dt, Ntau)
        got1 = pm.correlation_3op_1t(psi0, facs, nel, dims, omega, Hel, W, dt, Ntau)
        got2 = pm.correlation_3op_2t(psi0, facs, nel, dims, omega, Hel, W, dt, Nt, Ntau)
        scale = np.abs(ref).max()
        assert np.abs(got1 - ref[0]).max() < 1e-13 * scale and np.abs(got2 - ref).max() < 1e-13 * scale, blocks
        assert np.array_equal(got2[0], got1)
    for blocks in ((0, 1, 0, M), (M, 0, 1, 0), (0, 0, 0, 0)):
        facs = _facs(nel, M, rng, blocks)
        a, b, c, d = [pm.factor_dense(f, nel, dims) for f in facs]
        psi_t = pm.dense_states_t(H, psi0, dt, Nt)
        ref = pm.dense_corr_3op(H, psi_t, [a, b @ c, d], dt, Ntau)
        got1 = pm.correlation_4op_1t(psi0, facs, nel, dims, omega, Hel, W, dt, Ntau)
        got2 = pm.correlation_4op_2t(psi0, facs, nel, dims, omega, Hel, W, dt, Nt, Ntau)
        scale = np.abs(ref).max()
        assert np.abs(got1 - ref[0]).max() < 1e-13 * scale and np.abs(got2 - ref).max() < 1e-13 * scale, blocks
    with pytest.raises(NotImplementedError):
        pm.correlation_4op_1t(psi0, _facs(nel, M, rng, (0, 1, M, 0)), nel, dims, omega, Hel, W, dt, 2)


def golden_model():
    """(mol, ops3, ops4, fixture) with the pyqed_amd model and LVCOp operators of tests/golden/lvc_corr.npz."""
    from pyqed_amd import LVC, Mode
    g = np.load(GOLDEN)
    cps = [[] for _ in g["omega"]]
    for j, a, b, s in g["couplings"]:
        cps[int(j)].append([[int(a), int(b)], float(s)])
    mol = LVC(list(g["E"]), [Mode(float(w), c, truncate=int(n)) for w, c, n in zip(g["omega"], cps, g["trunc"])])
    make = lambda s: mol.buildop(int(s[1]), int(s[2])) if s[0] == 0 else mol.coordinate(int(s[1]))   # noqa: E731
    return mol, [make(s) for s in g["ops3_spec"]], [make(s) for s in g["ops4_spec"]], g


def test_restatement_against_the_reference_fixture():
    """The model and the LVCOp operators rebuilt from the fixture's parameters are the reference's H and operators, and
    the restated correlation functions give the reference's results to 1e-11."""
    mol, ops3, ops4, g = golden_model()
    H = np.zeros((mol.dim, mol.dim), dtype=complex)
    H[g["H_row"], g["H_col"]] = g["H_val"]
    assert np.abs(mol.buildH().toarray() - H).max() < 1e-15
    for ours, theirs in zip(ops3 + ops4, list(g["ops3"]) + list(g["ops4"])):
        assert np.abs(ours.toarray() - theirs).max() < 1e-15
    nel, dims = mol.nel, tuple(mol.fock_dims)
    args = (nel, dims, mol.omegas, mol.Hel(), mol.Wmats(), float(g["dt"]))
    f3 = [(o.A, 0 if o.mode is None else o.mode + 1) for o in ops3]
    f4 = [(o.A, 0 if o.mode is None else o.mode + 1) for o in ops4]
    Nt, Ntau = int(g["Nt"]), int(g["Ntau"])
    errs = {"c3_1t": relerr(pm.correlation_3op_1t(g["psi0"], f3, *args, Ntau), g["c3_1t"]),
            "c3_2t": relerr(pm.correlation_3op_2t(g["psi0"], f3, *args, Nt, Ntau), g["c3_2t"]),
            "c4_1t": relerr(pm.correlation_4op_1t(g["psi0"], f4, *args, Ntau), g["c4_1t"]),
            "c4_2t": relerr(pm.correlation_4op_2t(g["psi0"], f4, *args, Nt, Ntau), g["c4_2t"])}
    print(errs)
    assert np.abs(g["c3_1t"]).max() > 1e-3 and np.abs(g["c4_2t"]).max() > 1e-4   # not a comparison of zeros
    assert all(e < 1e-11 for e in errs.values()), errs


@functools.lru_cache(maxsize=None)
def _plan_lib():
    return build_pair_plan_lib(tempfile.mkdtemp(prefix="lvc_pair_plan_"))


def test_float64_restatement_on_the_gpu_cases():
    """On every case of the GPU kernel test the float64 restatement is within 1e-13 of the long-double one, a tenth
    of that test's 1e-12 (it measures 3e-16 at the small shapes and 1.2e-14 at the 262145-point one, where numpy's own
    float64 sum is the long one): that bound is about the kernels, not about the conditioning of the cases."""
    if not hp.EXTENDED_OK:
        pytest.skip("np.longdouble is not extended here")
    lib = _plan_lib()
    worst = (0.0, None)
    for nel, dims in pm.gpu_cases(lib.TILE, lib.limit) + [(1, (lib.TILE * lib.OBS_MAX_GRID + 1,))]:
        for P in (1, 3):
            omega, Hel, W, pairs, dt = pm.gpu_inputs(nel, dims, P)
            blocks = list(range(1 + len(dims)))
            lo = pm.pair_rk4(pairs, nel, dims, omega, Hel, W, dt, pm.NSTEPS, pm.SE, blocks)
            hi = pm.pair_rk4(pairs, nel, dims, omega, Hel, W, dt, pm.NSTEPS, pm.SE, blocks, dtype=np.clongdouble)
            e = max(hp.worst_member(a, b) for a, b in zip(lo, hi))
            worst = max(worst, (e, (nel, dims, P)))
    print(f"float64 against long double, worst over the GPU cases: {worst[0]:.2e} at {worst[1]}")
    assert worst[0] < 1e-13, worst


def test_class_refusals_before_any_device_work():
    from pyqed_amd import LVC, LVCOp, Mode
    mol = LVC([0.0, 1.0], [Mode(0.1, [], truncate=3), Mode(0.2, [], truncate=2)])
    sol = mol.wavepacket_dynamics()
    psi0 = mol.vertical(1)
    mu, x0, x1 = mol.buildop(0, 1), mol.coordinate(0), mol.coordinate(1)
    with pytest.raises(ValueError, match="correlation_3op_1t: oplist must hold 3 operators, got 2"):
        sol.correlation_3op_1t(psi0, [mu, mu], 0.1, 4)
    with pytest.raises(ValueError, match="correlation_3op_1t: Nt must be >= 1, got 0"):
        sol.correlation_3op_1t(psi0, [mu, mu, mu], 0.1, 0)
    with pytest.raises(ValueError, match="correlation_3op_2t: Ntau must be >= 1, got 0"):
        sol.correlation_3op_2t(psi0, [mu, mu, mu], 0.1, 2, 0)
    with pytest.raises(ValueError, match="correlation_4op_1t: oplist must hold 4 operators, got 3"):
        sol.correlation_4op_1t(psi0, [mu, mu, mu], 0.1, 2)
    with pytest.raises(ValueError, match="correlation_4op_2t: Nt must be >= 1, got -1"):
        sol.correlation_4op_2t(psi0, [mu, mu, mu, mu], 0.1, -1, 2)
    with pytest.raises(ValueError, match="correlation_3op_1t: operator 1 is an LVCOp of another space"):
        sol.correlation_3op_1t(psi0, [mu, LVCOp(np.eye(2), (3, 3)), mu], 0.1, 4)
    with pytest.raises(ValueError, match="correlation_4op_2t: operator 3 is an LVCOp of another space"):
        sol.correlation_4op_2t(psi0, [mu, mu, mu, LVCOp(np.eye(3), (3, 2))], 0.1, 2, 2)
    with pytest.raises(NotImplementedError, match="correlation_4op_1t: the product of two coordinate factors"):
        sol.correlation_4op_1t(psi0, [mu, x0, x1, mu], 0.1, 4)
    with pytest.raises(NotImplementedError, match="correlation_4op_2t: the product of two coordinate factors"):
        sol.correlation_4op_2t(psi0, [mu, x0, x0, mu], 0.1, 2, 2)
    with pytest.raises(ValueError, match="correlation_3op_1t: psi0 has 5 elements, expected 12"):
        sol.correlation_3op_1t(np.ones(5), [mu, x0, mu], 0.1, 4)
    with pytest.raises(ValueError, match="correlation_3op_2t: path='fast'"):
        sol.correlation_3op_2t(psi0, [mu, np.eye(2), mu], 0.1, 2, 2, path="fast")
    from pyqed_amd.mol import lvc_pair_observe
    with pytest.raises(ValueError, match="at least one block"):
        lvc_pair_observe(None, 2, (3, 2), [])


def test_c_refusals_before_any_device_work():
    """QD_EINVAL with the entry point's message; no pointer is read and no device call is made (this runs without a
    GPU).  The plan's messages are enumerated in tests/test_lvc_pair_plan_host.py."""
    from pyqed_amd import _lib
    lib = _lib.load()
    one = ctypes.c_void_p(16)    # never dereferenced
    ints = lambda *v: (ctypes.c_int * len(v))(*v)   # noqa: E731
    om = (ctypes.c_double * 6)(*([1.0] * 6))

    def run(P=1, nel=3, M=2, dims=ints(4, 4), nblk=2, blocks=ints(0, 2), nsteps=5, se=1, rec=one, path=0, psi=one,
            omega=om, Hel=one, W=one):
        return lib.qd_lvc_pair_rk4(psi, P, nel, M, dims, omega, Hel, W, 0.1, nsteps, se, nblk, blocks, rec, path, None)

    def observe(P=1, nel=3, M=2, dims=ints(4, 4), nblk=2, blocks=ints(0, 2), rec=one, psi=one):
        return lib.qd_lvc_pair_observe(psi, P, nel, M, dims, nblk, blocks, rec, None)

    shared = ((dict(P=0), "P=0 outside [1, 32767]"), (dict(P=32768), "P=32768 outside [1, 32767]"),
              (dict(nblk=0), "nblk=0 outside [1, 3]"), (dict(nblk=4), "nblk=4 outside [1, 3]"),
              (dict(blocks=ints(0, 3)), "blocks[1]=3 outside [0, 2]"),
              (dict(blocks=ints(-1, 0)), "blocks[0]=-1 outside [0, 2]"), (dict(blocks=None), "null blocks"),
              (dict(psi=None), "null pointer"), (dict(rec=None), "null pointer"), (dict(dims=None), "null dims"),
              (dict(nel=0), "nel=0 outside [1, 8]"), (dict(nel=9), "nel=9 outside [1, 8]"),
              (dict(M=0), "M=0 outside [1, 6]"), (dict(M=7), "M=7 outside [1, 6]"),
              (dict(dims=ints(2, 0)), "dims[1]=0 must be at least 1"),
              (dict(nel=2, M=3, dims=ints(1024, 1024, 1024)), "D = nel * prod(dims) must stay below 2^31"))
    for kw, msg in shared:
        assert run(**kw) == _lib.QD_EINVAL and _lib.last_error() == "qd_lvc_pair_rk4: " + msg, (kw, _lib.last_error())
        assert observe(**kw) == _lib.QD_EINVAL and _lib.last_error() == "qd_lvc_pair_observe: " + msg, \
            (kw, _lib.last_error())
    limit = _plan_lib().limit(2)
    for kw, msg in ((dict(omega=None), "null pointer"), (dict(Hel=None), "null pointer"), (dict(W=None), "null pointer"),
                    (dict(path=3), "path=3 outside [0, 2]"),
                    (dict(nsteps=-1), "nsteps=-1 and save_every=1 must not be negative"),
                    (dict(se=-1), "nsteps=5 and save_every=-1 must not be negative"),
                    (dict(se=0), "observables need save_every > 0"),
                    (dict(dims=ints(19, 18), path=2), f"the pair resident path needs D <= {limit} with 2 modes (D = 1026)")):
        assert run(**kw) == _lib.QD_EINVAL and _lib.last_error() == "qd_lvc_pair_rk4: " + msg, (kw, _lib.last_error())
