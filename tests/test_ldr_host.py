"""Host tests of the local-diabatic-representation feature (no GPU): the two numpy restatements of tests/ldr_models.py
against every case of tests/golden/ldr.npz (the real reference's LDR2.run, LDRN.run, short_time_propagator, rdm_el and
get_population), dense against factorised at shapes the fixture does not hold, sine_dvr against the reference's
SineDVR, and every refusal of the classes that comes before device work.

Bounds: the fixture's states have norm one or below and come from complex128 arithmetic over at most npts ns = 442
terms per element; 1e-12 relative leaves three digits over the 6.7e-15 the issue measured for the factorised form
against the reference."""
import numpy as np
import pytest

from conftest import load_golden, relerr
from ldr_models import EXTENDED_OK, ldr_dense, ldr_factorised, random_case, worst_member

TOL = 1e-12


@pytest.fixture(scope="module")
def g():
    return load_golden("ldr")


def case_of(g, tag):
    dt = float(g["dt"])
    apes, U = g[f"{tag}_apes"], g[f"{tag}_U"]
    expK = [g[f"{tag}_expKx"], g[f"{tag}_expKy"]] if f"{tag}_expKx" in g else \
        [g[f"{tag}_expK{d}"] for d in range(3) if f"{tag}_expK{d}" in g]
    return dict(U=U, expV=np.exp(-1j * dt * apes), expVh=np.exp(-1j * 0.5 * dt * apes), expK=expK,
                psi0=g[f"{tag}_psi0"], states=g[f"{tag}_states"], nt=int(g["nt"]), nout=int(g["nout"]))


@pytest.mark.parametrize("tag", ["a", "b", "c", "d", "n"])
def test_restatements_against_the_reference(g, tag):
    c = case_of(g, tag)
    ref = c["states"]
    assert ref.shape[0] == c["nt"] // c["nout"] + 1 and np.array_equal(ref[0], c["psi0"])
    dense = ldr_dense(c["psi0"], c["U"], c["expV"], c["expVh"], c["expK"], c["nt"], c["nout"])
    assert relerr(dense, ref[1:]) < TOL
    for dtype in (np.complex128, np.clongdouble):
        fac = ldr_factorised(c["psi0"][None], c["U"], c["expV"], c["expVh"], c["expK"], c["nt"], c["nout"], dtype)
        assert fac.dtype == dtype and relerr(fac[0].astype(complex), ref[1:]) < TOL, dtype


def test_truncated_cases_lose_norm_and_full_ones_keep_it(g):
    """M = ns: the step is unitary; M = 3 kept 2: a projection, so the fixture is no accident of a unitary run."""
    na = np.linalg.norm(g["a_states"].reshape(g["a_states"].shape[0], -1), axis=1)
    nb = np.linalg.norm(g["b_states"].reshape(g["b_states"].shape[0], -1), axis=1)
    assert np.allclose(na, na[0], rtol=1e-12) and nb[-1] < 0.999 * nb[0]
    assert np.iscomplexobj(g["c_U"]) and np.abs(g["c_U"].imag).max() > 1e-3 and not np.iscomplexobj(g["b_U"])


@pytest.mark.parametrize("dims,M,ns,B", [((9,), 4, 3, 2), ((5, 4), 2, 1, 1), ((3, 4, 2), 5, 2, 3), ((1, 6), 3, 3, 2),
                                         ((7, 1, 2), 2, 2, 1)])
def test_dense_against_factorised_off_the_fixture(dims, M, ns, B):
    c = random_case(5, dims, M, ns, B)
    fac = ldr_factorised(c["psi"], c["U"], c["expV"], c["expVh"], c["expK"], 5, 2)
    assert fac.shape == (B, 2) + dims + (ns,)
    for b in range(B):
        dense = ldr_dense(c["psi"][b], c["U"], c["expV"], c["expVh"], c["expK"], 5, 2)
        assert relerr(fac[b], dense) < TOL
    if EXTENDED_OK:
        ext = ldr_factorised(c["psi"], c["U"], c["expV"], c["expVh"], c["expK"], 5, 2, np.clongdouble)
        assert worst_member(fac, ext.astype(complex)) < TOL


def test_short_time_propagator_is_one_step_on_the_identity(g):
    """The reference's exp_V_half exp_T exp_V_half equals a one-step run of unit vectors whose closing factor is the
    half step: the construction LDR2.short_time_propagator uses on the device."""
    dt = float(g["dt"])
    for tag, full in (("s", True), ("a", False)):
        apes, U = g[f"{tag}_apes"], g[f"{tag}_U"]
        sh = apes.shape
        D = int(np.prod(sh))
        from pyqed_amd.ldr import sine_dvr
        x, y = g[f"{tag}_x"], g[f"{tag}_y"]
        mass = (0.8, 1.1) if tag == "s" else (1.0, 1.7)
        expK = [sine_dvr(a[0], a[-1], len(a), m).expT(dt) for a, m in ((x, mass[0]), (y, mass[1]))]
        eh = np.exp(-1j * 0.5 * dt * apes)
        cols = np.arange(D) if full else g["a_stp_cols"]
        eye = np.zeros((len(cols), D), dtype=complex)
        eye[np.arange(len(cols)), cols] = 1.0
        out = ldr_factorised(eye.reshape((len(cols),) + sh), U, eh, eh, expK, 1, 1)[:, 0]
        got = np.moveaxis(out, 0, -1)
        ref = g["s_stp"].reshape(sh + (D,)) if full else g["a_stp"]
        assert relerr(got, ref) < TOL, tag


# ----------------------------------------------------------------------------- sine DVR
@pytest.mark.parametrize("n", [5, 16])
def test_sine_dvr_against_the_reference(g, n):
    from pyqed_amd.ldr import sine_dvr
    xmin, xmax, mass, dt = g["dvr_args"]
    d = sine_dvr(xmin, xmax, n, mass)
    assert d.x.shape == (n,) and np.allclose(d.x, g[f"dvr{n}_x"], rtol=0, atol=1e-15)
    assert relerr(d.t(), g[f"dvr{n}_t"]) < 1e-14
    assert relerr(d.fbr2dvr(), g[f"dvr{n}_U"]) < 1e-15
    assert relerr(d.expT(dt), g[f"dvr{n}_expT"]) < 1e-14


@pytest.mark.parametrize("n", [1, 2, 5, 16, 63])
def test_sine_dvr_propagator_is_unitary_and_generated_by_t(n):
    import scipy.linalg
    from pyqed_amd.ldr import sine_dvr
    d = sine_dvr(-2.0, 3.0, n, mass=1.7)
    E = d.expT(0.07)
    assert np.abs(E @ E.conj().T - np.eye(n)).max() < 1e-13
    assert np.abs(E - scipy.linalg.expm(-0.07j * d.t())).max() < 1e-12
    assert np.abs(E - E.T).max() < 1e-14   # complex symmetric, not Hermitian


# ----------------------------------------------------------------------------- the classes, before any device work
def test_result_ldr_population_against_the_reference(g):
    from pyqed_amd import ResultLDR
    from pyqed_amd.ldr import LDRN
    sol = LDRN([tuple(d) for d in g["m_domains"]], tuple(int(l) for l in g["m_levels"]), ndim=2, nstates=2,
               mass=list(g["m_mass"]))
    assert sol.nx == [7, 3] and sol.ntot == 21
    r = ResultLDR(dx=sol.dx, dt=float(g["dt"]), psi0=g["m_psi0"], Nt=int(g["nt"]), nout=int(g["nout"]))
    r.psilist = list(g["m_states"])
    p = r.get_population(plot=False)
    assert p.shape == g["m_pop"].shape and np.abs(p - g["m_pop"]).max() < 1e-15
    assert len(r.times) == len(r.psilist)


def test_ldrn_grid_is_the_references(g):
    from pyqed_amd.ldr import LDRN
    sol = LDRN([tuple(d) for d in g["n_domains"]], tuple(int(l) for l in g["n_levels"]), ndim=3, nstates=2,
               mass=list(g["n_mass"]))
    assert sol.nx == [7, 3, 3] and np.allclose(sol.dx, g["n_dx"], rtol=1e-15)
    sol.apes = g["n_apes"]
    sol.buildV(float(g["dt"]))
    for d, K in enumerate(sol.buildK(float(g["dt"]))):
        assert relerr(K, g[f"n_expK{d}"]) < 1e-14


def test_ldr2_setup_against_the_reference(g):
    """buildK's rule (the box is [x[0], x[-1]] with nx interior points), buildV and build_apes; the states of the build
    path in gauge-free quantities: the surfaces and the projector U U^+."""
    from pyqed_amd import LDR2
    dt = float(g["dt"])
    sol = LDR2(g["a_x"], g["a_y"], nstates=2, mass=[1.0, 1.7])
    sol.v = g["a_v"]
    sol.build_apes()
    assert relerr(sol.apes, g["a_apes"]) < 1e-14
    P, Pref = (np.einsum('...ma,...na->...mn', U, U.conj()) for U in (sol.adiabatic_states, g["a_U"]))
    assert relerr(P, Pref) < 1e-13
    sol.buildK(dt)
    sol.buildV(dt)
    assert relerr(sol.exp_K[0], g["a_expKx"]) < 1e-14 and relerr(sol.exp_K[1], g["a_expKy"]) < 1e-14
    assert np.array_equal(sol.exp_V, np.exp(-1j * dt * sol.apes))
    assert np.array_equal(sol.exp_V_half, np.exp(-1j * 0.5 * dt * sol.apes))
    assert len(sol.K) == 2 and sol.K[0].shape == (15, 15)
    A = sol.build_ovlp()
    assert A.shape == (15, 11, 2, 15, 11, 2) and sol.A is A
    assert np.abs(np.einsum('ijaijb->ijab', A) - np.eye(2)).max() < 1e-13


def test_build_path_in_gauge_free_quantities(g):
    """Case d: the class diagonalises v itself, so its states differ from the fixture's by a sign per point and state.
    chi = U psi and the populations do not depend on it: the factorised restatement with the class's states against
    the reference's snapshots."""
    from pyqed_amd import LDR2
    c = case_of(g, "d")
    sol = LDR2(g["d_x"], g["d_y"], nstates=2)
    sol.v = g["d_v"]
    sol.build_apes()
    U, Uref = sol.adiabatic_states, g["d_U"]
    # the same run in the class's gauge: psi0 is given in the reference's gauge, so carry it over through chi
    sign = np.einsum('...ma,...ma->...a', U.conj(), Uref)
    assert np.abs(np.abs(sign) - 1).max() < 1e-12
    psi0 = c["psi0"] * sign
    fac = ldr_factorised(psi0[None], U, c["expV"], c["expVh"], c["expK"], c["nt"], c["nout"])[0]
    chi = np.einsum('...ma,z...a->z...m', U, fac)
    chi_ref = np.einsum('...ma,z...a->z...m', Uref, c["states"][1:])
    assert relerr(chi, chi_ref) < TOL
    assert np.abs(np.abs(fac) ** 2 - np.abs(c["states"][1:]) ** 2).max() < 1e-13


def test_class_refusals():
    from pyqed_amd import LDR2, LDRN
    from pyqed_amd.ldr import DENSE_MAX_D, ldr_run
    x, y = np.linspace(-1, 1, 6), np.linspace(-1, 1, 5)
    with pytest.raises(NotImplementedError, match="two-dimensional"):
        LDR2(x, y, ndim=3)
    with pytest.raises(NotImplementedError, match="only 'sine'"):
        LDR2(x, y, dvr='sinc')
    sol = LDR2(x, y, nstates=2)
    with pytest.raises(AssertionError):
        sol.v = np.zeros((6, 5, 3, 3))
    for name, line in (("fast_run", "1613"), ("fast_LvN", "1679"), ("buildH", "1532"), ("HEOM", "1770")):
        with pytest.raises(NotImplementedError, match=line):
            getattr(sol, name)()
    psi0 = np.zeros((6, 5, 2), dtype=complex)
    with pytest.raises(ValueError, match="set v .* or apes and adiabatic_states"):
        sol.run(psi0, 0.1, 2)
    with pytest.raises(ValueError, match="build_apes: the diabatic potential v is not set"):
        sol.build_apes()
    sol.A = np.zeros((6, 5, 2, 6, 5, 2))
    with pytest.raises(ValueError, match="only the dense overlap A was given.*set adiabatic_states"):
        sol.run(psi0, 0.1, 2)
    sol.adiabatic_states = np.zeros((6, 5, 1, 2))
    with pytest.raises(ValueError, match="M >= nstates"):
        sol.run(psi0, 0.1, 2)
    sol.adiabatic_states = np.zeros((6, 5, 3, 2))
    with pytest.raises(ValueError, match="apes .* must be set"):
        sol.run(psi0, 0.1, 2)
    sol.apes = np.zeros((6, 5, 3))
    with pytest.raises(ValueError, match=r"apes must be \(6, 5, 2\)"):
        sol.run(psi0, 0.1, 2)
    # dense objects above the stated D
    nx = int(np.ceil(np.sqrt(DENSE_MAX_D / 2))) + 1
    big = LDR2(np.linspace(-1, 1, nx), np.linspace(-1, 1, nx), nstates=2)
    assert big._D() > DENSE_MAX_D
    big.adiabatic_states = np.zeros((nx, nx, 2, 2))
    big.apes = np.zeros((nx, nx, 2))
    for call in (big.build_ovlp, lambda: big.short_time_propagator(0.1)):
        with pytest.raises(ValueError, match=f"exceeds {DENSE_MAX_D}"):
            call()

    with pytest.raises(NotImplementedError, match="ndim 1 to 3"):
        LDRN([(-1, 1)] * 4, [2] * 4, ndim=4)
    with pytest.raises(NotImplementedError, match="only 'sine'"):
        LDRN([(-1, 1)] * 2, [2, 2], ndim=2, dvr_type='gauss_hermite', x0=[0, 0])
    with pytest.raises(AssertionError):
        LDRN([(-1, 1)] * 2, [2, 2, 2], ndim=2)
    soln = LDRN([(-1, 1)] * 2, [3, 2], ndim=2, nstates=2)
    with pytest.raises(ValueError, match="PES minimum is not 0"):
        soln.v = np.ones((7, 3, 2, 2))
    with pytest.raises(AssertionError):
        soln.v = np.zeros((7, 3, 2))
    soln.A = np.zeros((7, 3, 2, 7, 3, 2))
    with pytest.raises(ValueError, match="only the dense overlap A was given"):
        soln.run(np.zeros((7, 3, 2), dtype=complex), 0.1, 2)
    bign = LDRN([(-1, 1)] * 2, [6, 6], ndim=2, nstates=2)
    with pytest.raises(ValueError, match=f"rdm_nuc: D = npts \\* nstates = {63 * 63 * 2} exceeds {DENSE_MAX_D}"):
        bign.rdm_nuc(np.zeros((63, 63, 2)))
    f = np.arange(7 * 3 * 2).reshape(7, 3, 2) * (1 + 0.5j)
    assert np.allclose(soln.rdm_nuc(f), np.einsum('ija,kla->ijkl', f.conj(), f))

    with pytest.raises(ValueError, match="path='fast'"):
        ldr_run(None, None, None, [], 0.1, 1, path="fast")
    with pytest.raises(ValueError, match="torch complex128"):
        ldr_run(np.zeros((1, 3, 2)), None, None, [None], 0.1, 1)
