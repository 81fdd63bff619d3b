"""The LVC model on the host (no GPU): the matrix-free restatement of tests/lvc_models.py against the dense H assembled
from explicit Kronecker products and against the extended-precision RK4 of oracle/highprec.py, the LVC class of
pyqed_amd.mol against the reference's own class (tests/golden/lvc.npz, written by tests/golden/make_golden_lvc.py),
per-mode truncations, every refusal with its message, and LVCOp against its tocsr()."""
import ctypes

import numpy as np
import pytest
import scipy.sparse as sp

import lvc_models as lm
from conftest import load_golden
from oracle import highprec as hp

SHAPES = [(3, (4, 4)), (3, (3, 3, 3)), (2, (2, 2, 2, 2)), (3, (2, 5)), (1, (7,))]


@pytest.mark.parametrize("nel,dims", SHAPES)
def test_restatement_against_kron_h(nel, dims):
    """H psi, matrix-free, equals the kron-assembled H applied to psi; the record equals <psi| op |psi> of the
    kron-assembled operators.  Non-Hermitian Hel and W: a transposed read shows."""
    omega, Hel, W = lm.random_model(nel, dims)
    psi = lm.random_states(3, nel, dims)
    H = lm.dense_h(nel, dims, omega, Hel, W)
    ref = psi @ H.T
    got = lm.apply(psi, nel, dims, omega, Hel, W)
    assert np.abs(got - ref).max() < 1e-13 * max(1.0, np.abs(ref).max())
    if hp.EXTENDED_OK:
        ext = lm.apply(psi, nel, dims, omega, Hel, W, np.clongdouble).astype(np.complex128)
        assert np.abs(ext - ref).max() < 1e-13 * max(1.0, np.abs(ref).max())
    rho, X, nbar = lm.split_record(lm.record(psi, nel, dims), nel, len(dims))
    eyes = [np.eye(N) for N in dims]
    for b in range(3):
        for a1 in range(nel):
            for a2 in range(nel):
                A = np.zeros((nel, nel))
                A[a1, a2] = 1.0           # <A (x) 1> = tr(A rho) = rho[a2][a1]
                assert abs(np.vdot(psi[b], lm._kron(A, *eyes) @ psi[b]) - rho[b, a2, a1]) < 1e-13
                for j in range(len(dims)):
                    op = lm._kron(A, *(eyes[:j] + [lm.x_matrix(dims[j])] + eyes[j + 1:]))
                    assert abs(np.vdot(psi[b], op @ psi[b]) - X[b, j, a2, a1]) < 1e-13
        for j in range(len(dims)):
            op = lm._kron(np.eye(nel), *(eyes[:j] + [np.diag(np.arange(dims[j]))] + eyes[j + 1:]))
            assert abs(np.vdot(psi[b], op @ psi[b]) - nbar[b, j]) < 1e-13 and abs(nbar[b, j].imag) == 0


@pytest.mark.parametrize("nel,dims", SHAPES)
def test_restated_rk4_against_highprec_oracle(nel, dims):
    """The Horner RK4 of the restatement against oracle.highprec.tdse (classical RK4) on the dense H: the same
    polynomial of dt H, so they agree to rounding.  5 steps saved every 2."""
    omega, Hel, W = lm.random_model(nel, dims)
    psi0 = lm.random_states(2, nel, dims)
    dt = 0.5 / lm.h_bound(dims, omega, Hel, W)
    H = lm.dense_h(nel, dims, omega, Hel, W)
    dtype = np.clongdouble if hp.EXTENDED_OK else np.complex128
    rpsi, rsnap, _ = hp.tdse(H, psi0, dt, 5, 2, dtype=dtype)
    for dt_ in (np.complex128, dtype):
        psi, snap, obs = lm.rk4(psi0, nel, dims, omega, Hel, W, dt, 5, 2, dtype=dt_)
        assert snap.shape == rsnap.shape == (2, 2, lm.size(nel, dims)) and obs.shape == (2, 3, lm.nobs(nel, dims))
        assert hp.worst_member(psi, rpsi) < 1e-14 and hp.worst_member(snap, rsnap) < 1e-14
        # the records are those of the saved states
        assert np.array_equal(obs[:, 0], lm.record(psi0, nel, dims, dt_).astype(np.complex128))


def _model(g, tag):
    from pyqed_amd import LVC, Mode
    trunc = [int(n) for n in g[tag + "_trunc"]]
    cps = [[] for _ in trunc]
    for j, a, b, s in g[tag + "_couplings"]:
        cps[int(j)].append([[int(a), int(b)], float(s)])
    modes = [Mode(float(w), c, truncate=n) for w, c, n in zip(g[tag + "_omega"], cps, trunc)]
    mol = LVC(g[tag + "_E"], modes)
    ex = g[tag + "_extra"]
    return mol, [[int(ex[0]), int(ex[1])], float(ex[2])]


@pytest.mark.parametrize("tag", ["a", "b"])
def test_lvc_class_against_reference_fixture(tag):
    g = load_golden("lvc")
    mol, extra = _model(g, tag)
    D = mol.dim
    Href = sp.coo_matrix((g[tag + "_H_val"], (g[tag + "_H_row"], g[tag + "_H_col"])), shape=(D, D)).toarray()
    # add_coupling after buildH, as the reference needs it ...
    mol.buildH()
    H = mol.add_coupling(extra)
    assert sp.issparse(H) and np.abs(H.toarray() - Href).max() < 1e-13
    # ... and before: the same H
    mol2, _ = _model(g, tag)
    assert mol2.add_coupling(extra) is None
    assert np.abs(mol2.buildH().toarray() - Href).max() < 1e-13
    # the factors the device path takes reproduce it too
    dense = lm.dense_h(mol.nel, mol.fock_dims, mol.omegas, mol.Hel(), mol.Wmats())
    assert np.abs(dense - Href).max() < 1e-13
    assert np.abs(mol.vertical(1) - g[tag + "_vertical1"]).max() < 1e-13
    assert np.array_equal(mol.groundstate(), mol.vertical(0))
    for x, e in zip(g[tag + "_apes_x"], g[tag + "_apes"]):
        assert np.abs(mol.APES(x) - e).max() < 1e-13
    assert np.abs(mol.rdm_el(g[tag + "_psi_r"]) - g[tag + "_rdm"]).max() < 1e-13
    # the reference's run, restated on the host from the class's factors (the GPU run: tests/test_lvc_gpu.py)
    Nt, nout, dt = int(g["Nt"]), int(g["nout"]), float(g["dt"])
    psi, snap, obs = lm.rk4(g[tag + "_vertical1"][None], mol.nel, mol.fock_dims, mol.omegas, mol.Hel(), mol.Wmats(), dt,
                            (Nt // nout - 1) * nout, nout)
    states = np.concatenate([g[tag + "_vertical1"][None], snap[0]])
    assert states.shape == g[tag + "_states"].shape and np.abs(states - g[tag + "_states"]).max() < 1e-13
    rho, X, _ = lm.split_record(obs[0], mol.nel, mol.nmodes)
    ops = [mol.buildop(1), mol.coordinate(0)]
    got = np.stack([op.from_record(rho, X) for op in ops], axis=1)
    assert got.shape == g[tag + "_obs"].shape == (3, 2) and np.abs(got - g[tag + "_obs"]).max() < 1e-13


def test_per_mode_truncations_and_one_mode():
    from pyqed_amd import LVC, Mode
    mol = LVC([0.0, 1.0, 1.2], [Mode(0.1, [[[1, 1], 0.05]], truncate=3), Mode(0.2, [[[1, 2], 0.03]], truncate=4)])
    H = mol.buildH()
    assert H.shape[0] == mol.vertical().size == 36
    W = mol.Wmats()
    assert np.abs(H.toarray() - lm.dense_h(3, (3, 4), mol.omegas, mol.Hel(), W)).max() < 1e-15
    assert W[0, 1, 1] == 0.05 and W[1, 1, 2] == W[1, 2, 1] == 0.03 and np.count_nonzero(W) == 3
    one = LVC([0.0, 0.5], [Mode(0.3, [[[0, 1], 0.1]], truncate=5)])
    assert one.buildH().shape == (10, 10) and one.vertical(1)[5] == 1
    assert np.abs(one.H.toarray() - lm.dense_h(2, (5,), one.omegas, one.Hel(), one.Wmats())).max() < 1e-15
    sol = one.wavepacket_dynamics()
    assert type(sol).__name__ == "LVCSolver" and np.array_equal(sol.groundstate, one.vertical(0))
    fresh = LVC([0.0, 0.5], [Mode(0.3, [], truncate=2)])
    assert fresh.wavepacket_dynamics() is not None and fresh.H is None   # no buildH needed for a solver


def test_python_refusals():
    from pyqed_amd import LVC, LVCOp, Mode
    m = lambda n=2: Mode(0.1, [], truncate=n)   # noqa: E731
    for args, msg in ((([], [m()]), "0 electronic states, 1 to 8"), (([0] * 9, [m()]), "9 electronic states, 1 to 8"),
                      (([0, 1], []), "0 modes, 1 to 6"), (([0, 1], [m()] * 7), "7 modes, 1 to 6"),
                      (([0, 1], [m(0)]), "mode 0 is truncated to 0 levels"),
                      (([0, 1], [m(2 ** 10)] * 3 + [m(2)]), r"must stay below 2\^31"),
                      (([0, 1], [Mode(0.1, [[[0, 2], 0.1]])]), r"couples states \(0, 2\) outside \[0, 2\)")):
        with pytest.raises(ValueError, match=msg):
            LVC(*args)
    mol = LVC([0.0, 1.0], [m(3), m(2)])
    with pytest.raises(ValueError, match="The number of modes 2 is not"):
        mol.wavepacket_dynamics(method="SPO")
    with pytest.raises(ValueError, match=r"states \(2, 0\) outside"):
        mol.add_coupling([[2, 0], 0.1])
    with pytest.raises(ValueError, match=r"state 2 outside \[0, 2\)"):
        mol.vertical(2)
    with pytest.raises(ValueError, match="x has 1 coordinates for 2 modes"):
        mol.APES([0.1])
    with pytest.raises(ValueError, match=r"mode 2 outside \[0, 2\)"):
        LVCOp(np.eye(2), (3, 2), mode=2)
    big = LVC([0, 1, 2], [m(64)] * 4)
    with pytest.raises(ValueError, match="too large to assemble H on the host"):
        big.buildH()
    sol = mol.wavepacket_dynamics()
    with pytest.raises(TypeError, match=r"e_ops\[1\] is no LVCOp"):     # before any device work
        sol.run(dt=0.1, Nt=4, e_ops=[mol.buildop(1), np.eye(12)], store_states=False)
    with pytest.raises(ValueError, match=r"e_ops\[0\] has shape \(3, 3\)"):
        sol.run(dt=0.1, Nt=4, e_ops=[np.eye(3)])
    with pytest.raises(ValueError, match=r"psi0s must be \[B, 12\]"):
        sol.run_batch(np.zeros((2, 5)), dt=0.1, Nt=4)


def test_c_refusals_before_any_device_work():
    """QD_EINVAL with the entry point's message for everything the plan does not admit; no pointer is read and no
    device call is made (this runs without a GPU).  The messages themselves are enumerated in
    tests/test_lvc_plan_host.py."""
    from pyqed_amd import _lib
    lib = _lib.load()
    one = ctypes.c_void_p(16)    # never dereferenced
    ints = lambda *v: (ctypes.c_int * len(v))(*v)   # noqa: E731
    om = (ctypes.c_double * 6)(*([1.0] * 6))

    def rk4(B, nel, M, dims, nsteps=1, se=1, obs=None, path=0):
        return lib.qd_lvc_rk4(one, B, nel, M, dims, om, one, one, 0.1, nsteps, se, None, obs, path, None)

    L = lib
    cases = ((lambda: rk4(1, 0, 1, ints(2)), "qd_lvc_rk4: nel=0 outside [1, 8]"),
             (lambda: rk4(1, 9, 1, ints(2)), "qd_lvc_rk4: nel=9 outside [1, 8]"),
             (lambda: rk4(1, 3, 0, ints(2)), "qd_lvc_rk4: M=0 outside [1, 6]"),
             (lambda: rk4(1, 3, 7, ints(2)), "qd_lvc_rk4: M=7 outside [1, 6]"),
             (lambda: rk4(1, 3, 2, None), "qd_lvc_rk4: null dims"),
             (lambda: rk4(1, 3, 2, ints(2, 0)), "qd_lvc_rk4: dims[1]=0 must be at least 1"),
             (lambda: rk4(1, 2, 3, ints(1024, 1024, 1024)), "qd_lvc_rk4: D = nel * prod(dims) must stay below 2^31"),
             (lambda: rk4(65536, 3, 1, ints(2)), "qd_lvc_rk4: B=65536 outside [1, 65535]"),
             (lambda: rk4(0, 3, 1, ints(2)), "qd_lvc_rk4: B=0 outside [1, 65535]"),
             (lambda: rk4(1, 3, 1, ints(2), path=3), "qd_lvc_rk4: path=3 outside [0, 2]"),
             (lambda: rk4(1, 3, 1, ints(2), nsteps=-1), "qd_lvc_rk4: nsteps=-1 and save_every=1 must not be negative"),
             (lambda: rk4(1, 3, 1, ints(2), nsteps=2, se=0, obs=one), "qd_lvc_rk4: observables need save_every > 0"),
             (lambda: rk4(1, 3, 2, ints(37, 37), path=2), "qd_lvc_rk4: the resident path needs D <= 2048 (D = 4107)"),
             (lambda: L.qd_lvc_rk4(None, 1, 3, 1, ints(2), om, one, one, 0.1, 1, 1, None, None, 0, None),
              "qd_lvc_rk4: null pointer"),
             (lambda: L.qd_lvc_apply(one, None, 1, 3, 1, ints(2), om, one, one, None), "qd_lvc_apply: null pointer"),
             (lambda: L.qd_lvc_apply(one, one, 1, 3, 1, ints(2), om, one, one, None),
              "qd_lvc_apply: out must not be psi"),
             (lambda: L.qd_lvc_apply(one, ctypes.c_void_p(32), 1, 9, 1, ints(2), om, one, one, None),
              "qd_lvc_apply: nel=9 outside [1, 8]"),
             (lambda: L.qd_lvc_observe(one, 0, 3, 1, ints(2), one, None), "qd_lvc_observe: B=0 outside [1, 65535]"),
             (lambda: L.qd_lvc_observe(one, 1, 3, 1, ints(2), None, None), "qd_lvc_observe: null pointer"))
    for call, msg in cases:
        assert call() == _lib.QD_EINVAL and _lib.last_error() == msg, msg


def test_lvcop_against_its_csr():
    from pyqed_amd import LVC, LVCOp, Mode
    rng = np.random.default_rng(5)
    mol = LVC([0.0, 1.0, 1.3], [Mode(0.1, [], truncate=3), Mode(0.2, [], truncate=4), Mode(0.3, [], truncate=2)])
    D = mol.dim
    A = rng.standard_normal((3, 3)) + 1j * rng.standard_normal((3, 3))
    ops = [mol.buildop(1), mol.buildop(0, 2), mol.buildop(0, 2, isherm=False), mol.coordinate(0), mol.coordinate(2),
           mol.promote(A, "el"), LVCOp(A, mol.fock_dims, mode=1)]
    v = rng.standard_normal(D) + 1j * rng.standard_normal(D)
    V = rng.standard_normal((D, 2)) + 1j * rng.standard_normal((D, 2))
    for op in ops:
        C = op.tocsr()
        assert op.shape == C.shape == (D, D) and np.array_equal(op.toarray(), C.toarray())
        for x in (v, V, v.real):
            assert np.abs(op.dot(x) - C @ x).max() < 1e-14 and np.abs((op @ x) - C @ x).max() < 1e-14
        assert np.abs((v @ op) - v @ C).max() < 1e-14
    assert np.array_equal(mol.buildop(0, 2, isherm=False).A, np.array([[0, 0, 0], [0, 0, 0], [1, 0, 0]]))
    for p, q in [(a, b) for a in ops for b in ops]:
        prod = p @ q
        ref = (p.tocsr() @ q.tocsr()).toarray()
        if p.mode is None or q.mode is None:
            assert isinstance(prod, LVCOp) and np.abs(prod.toarray() - ref).max() < 1e-14
        else:
            assert sp.issparse(prod) and np.abs(prod.toarray() - ref).max() < 1e-14
    vib = mol.promote(sp.identity(mol.nvib), "vib")
    assert sp.issparse(vib) and vib.shape == (D, D)
    # expectation values from a record
    psi = v / np.linalg.norm(v)
    rho, X, _ = lm.split_record(lm.record(psi[None], 3, mol.fock_dims)[0], 3, 3)
    for op in ops:
        assert abs(op.from_record(rho, X) - np.vdot(psi, op.tocsr() @ psi)) < 1e-13
