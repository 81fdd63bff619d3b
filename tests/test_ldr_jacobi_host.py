"""Host tests of the Jacobi-coordinate LDR feature (no GPU): the two numpy restatements of tests/ldr_jacobi_models.py
against every case of tests/golden/ldr_jacobi.npz (the real reference's LDR2_Jacobi.run), the factorisation
S diag(exp(-i E_m dt / I(x_i))) S against the reference's per-row exp_K[1], and the host side of the class: grids,
buildK, the constructor-dt quirk both ways, the 2^24 limit and every refusal with its message.

Bound: 1e-12 relative, as tests/test_ldr_host.py holds its restatements: states of norm one or below from complex128
sums of at most npts ns = 210 terms per element."""
import numpy as np
import pytest

from conftest import load_golden, relerr
from ldr_jacobi_models import EXTENDED_OK, jacobi_factorised, jacobi_rows, random_case, rows_of
from ldr_models import worst_member

TOL = 1e-12
TAGS = ["a", "b", "q"]
MASS_X = 1.3


def inertia(r):
    return 2.0 * r ** 2


@pytest.fixture(scope="module")
def g():
    return load_golden("ldr_jacobi")


def solver_of(g, tag, **kw):
    from pyqed_amd import LDR2_Jacobi
    levels = (4, 3) if tag == "b" else (3, 3)
    kw.setdefault("dt", float(g[f"{tag}_dt_ctor"]))
    return LDR2_Jacobi([tuple(d) for d in g["domains"]], levels, ['sine', 'sine'], mass=[MASS_X, inertia], nstates=2,
                       **kw)


def factors_of(g, tag):
    """S and the phase table from the fixture's grid and moment of inertia alone."""
    from pyqed_amd import sine_dvr
    d = sine_dvr(*g["domains"][1], len(g[f"{tag}_y"]))
    ph = np.exp(-1j * float(g[f"{tag}_dt_ctor"]) * d.levels()[None, :] / g[f"{tag}_I"][:, None])
    return d.fbr2dvr(), ph


def case_of(g, tag):
    dt = float(g["dt"])
    apes = g[f"{tag}_apes"]
    return dict(U=g[f"{tag}_U"], expV=np.exp(-1j * dt * apes), expVh=np.exp(-1j * 0.5 * dt * apes),
                psi0=g[f"{tag}_psi0"], states=g[f"{tag}_states"], nt=int(g["nt"]), nout=int(g["nout"]))


@pytest.mark.parametrize("tag", TAGS)
def test_restatements_against_the_reference(g, tag):
    c = case_of(g, tag)
    ref = c["states"]
    assert ref.shape[0] == c["nt"] // c["nout"] + 1 and np.array_equal(ref[0], c["psi0"])
    rows = jacobi_rows(c["psi0"][None], c["U"], c["expV"], c["expVh"], g[f"{tag}_expKy"], [g[f"{tag}_expKx"]],
                       c["nt"], c["nout"])
    assert relerr(rows[0], ref[1:]) < TOL
    S, ph = factors_of(g, tag)
    for dtype in (np.complex128, np.clongdouble):
        fac = jacobi_factorised(c["psi0"][None], c["U"], c["expV"], c["expVh"], S, S, ph, [g[f"{tag}_expKx"]],
                                c["nt"], c["nout"], dtype)
        assert fac.dtype == dtype and relerr(fac[0].astype(complex), ref[1:]) < TOL, dtype


@pytest.mark.parametrize("tag", TAGS)
def test_every_row_shares_the_sine_transform_as_eigenvectors(g, tag):
    S, ph = factors_of(g, tag)
    ref = g[f"{tag}_expKy"]
    assert ref.shape == (len(g[f"{tag}_x"]),) + (len(g[f"{tag}_y"]),) * 2
    assert np.abs(rows_of(S, S, ph) - ref).max() < 1e-14
    assert np.abs(S - S.T).max() < 1e-15 and np.abs(S @ S - np.eye(len(S))).max() < 1e-14
    # the rows differ: a single matrix for the whole axis would not do
    assert np.abs(ref[0] - ref[-1]).max() > 1e-3


def test_truncated_case_loses_norm_and_the_quirk_case_differs(g):
    nb = np.linalg.norm(g["b_states"].reshape(g["b_states"].shape[0], -1), axis=1)
    na = np.linalg.norm(g["a_states"].reshape(g["a_states"].shape[0], -1), axis=1)
    assert np.allclose(na, na[0], rtol=1e-12) and nb[-1] < 0.999 * nb[0]
    assert np.iscomplexobj(g["b_U"]) and np.abs(g["b_U"].imag).max() > 1e-3
    assert float(g["q_dt_ctor"]) == 0.03 and float(g["dt"]) == 0.05
    assert np.abs(g["q_expKy"] - g["a_expKy"]).max() > 1e-3 and np.array_equal(g["q_x"], g["a_x"])


@pytest.mark.parametrize("dims,M,ns,B", [((9,), 4, 3, 2), ((5, 4), 2, 1, 1), ((3, 4, 5), 5, 2, 3), ((1, 6), 3, 3, 2),
                                         ((7, 2, 1), 2, 2, 1)])
def test_rows_against_factorised_off_the_fixture(dims, M, ns, B):
    """General F, Fb and ph in one to three dimensions: the factorised form is the row form with Fb diag(ph) F."""
    c = random_case(5, dims, M, ns, B)
    fac = jacobi_factorised(c["psi"], c["U"], c["expV"], c["expVh"], c["F"], c["Fb"], c["ph"], c["expK"], 5, 2)
    assert fac.shape == (B, 2) + dims + (ns,)
    rows = jacobi_rows(c["psi"], c["U"], c["expV"], c["expVh"], rows_of(c["F"], c["Fb"], c["ph"]), c["expK"], 5, 2)
    assert worst_member(fac, rows) < TOL
    if EXTENDED_OK:
        ext = jacobi_factorised(c["psi"], c["U"], c["expV"], c["expVh"], c["F"], c["Fb"], c["ph"], c["expK"], 5, 2,
                                np.clongdouble)
        assert worst_member(fac, ext.astype(complex)) < TOL
    # the inputs are what the GPU tests rely on: nothing symmetric, orthogonal or inverse, moduli in [0.5, 1.5]
    n = dims[-1]
    if n > 1:
        assert np.abs(c["F"] - c["F"].T).max() > 1e-3 and np.abs(c["F"] - c["Fb"]).max() > 1e-3
        assert np.abs(c["Fb"] @ c["F"] - np.eye(n)).max() > 1e-3
    assert 0.5 <= np.abs(c["ph"]).min() and np.abs(c["ph"]).max() <= 1.5 and c["ph"].shape == dims


def test_class_grids_and_attributes(g):
    sol = solver_of(g, "b", nt=7, nout=3)
    assert np.array_equal(sol.x, g["b_x"]) and np.array_equal(sol.y, g["b_y"])
    assert (sol.nx, sol.ny, sol.nstates, sol.ndim, sol.npts) == (15, 7, 2, 2, 105)
    assert (sol.dt, sol.nt, sol.nout) == (0.05, 7, 3)
    assert [len(w) for w in sol.w] == [15, 7] and sol.w[0][0] == 1 / 15 and sol.w[1][-1] == 1 / 7
    assert sol.mass[0] == MASS_X and sol.mass[1] is inertia
    assert sol.apes is None and sol.A is None and sol.exp_K is None
    assert np.allclose(sol.metric((2.0, 0.3)), np.diag([1 / MASS_X, 1 / 8.0]))
    assert np.isclose(sol.dx, g["b_x"][1] - g["b_x"][0]) and np.isclose(sol.dy, g["b_y"][1] - g["b_y"][0])
    # 'sinc' is the reference's other name for the same uniform grid
    from pyqed_amd import LDR2_Jacobi
    s2 = LDR2_Jacobi([tuple(d) for d in g["domains"]], (4, 3), ['sinc', 'sine'], mass=[MASS_X, inertia])
    assert np.array_equal(s2.x, sol.x) and s2.mass[1] is inertia and s2.dt is None


def test_build_apes_and_buildV_on_the_host(g):
    sol = solver_of(g, "a")
    with pytest.raises(AssertionError):
        sol.v = g["a_v"][:-1]
    sol.v = g["a_v"]
    w = sol.build_apes()
    assert relerr(w, g["a_apes"]) < 1e-13 and w is sol.apes
    sign = np.einsum('...ma,...ma->...a', sol.adiabatic_states.conj(), g["a_U"])
    assert np.abs(np.abs(sign) - 1).max() < 1e-12
    sol.buildV(0.05)
    assert np.array_equal(sol.exp_V, np.exp(-1j * 0.05 * sol.apes))
    assert np.array_equal(sol.exp_V_half, np.exp(-1j * 0.025 * sol.apes))


@pytest.mark.parametrize("tag", TAGS)
def test_buildK_against_the_reference(g, tag):
    sol = solver_of(g, tag)
    eK = sol.buildK(float(g["dt"]))
    assert eK is sol.exp_K and len(eK) == 2 and eK[1].shape == g[f"{tag}_expKy"].shape
    assert np.abs(eK[0] - g[f"{tag}_expKx"]).max() < 1e-14 and np.abs(eK[1] - g[f"{tag}_expKy"]).max() < 1e-14


def test_constructor_dt_rules_the_kinetic_factor(g):
    """The quirk both ways: buildK takes the constructor's dt whatever it is given; with none, the argument."""
    sol = solver_of(g, "q")                                    # constructor dt 0.03
    eK = sol.buildK(0.05)
    assert np.abs(eK[1] - g["q_expKy"]).max() < 1e-14 and np.abs(eK[1] - g["a_expKy"]).max() > 1e-3
    sol = solver_of(g, "a", dt=None)
    eK = sol.buildK(0.03)
    assert np.abs(eK[0] - g["q_expKx"]).max() < 1e-14 and np.abs(eK[1] - g["q_expKy"]).max() < 1e-14
    eK = sol.buildK(0.05)
    assert np.abs(eK[1] - g["a_expKy"]).max() < 1e-14


def test_buildK_row_limit():
    from pyqed_amd import LDR2_Jacobi
    from pyqed_amd.ldr import JACOBI_ROWS_MAX
    assert JACOBI_ROWS_MAX == 2 ** 24
    dom = [(0.5, 3.5), (0.0, np.pi)]
    big = LDR2_Jacobi(dom, (9, 8), ['sine', 'sine'], mass=[1.0, inertia], dt=0.01)      # 511 x 255^2 > 2^24
    assert big.nx * big.ny ** 2 == 511 * 255 ** 2 > JACOBI_ROWS_MAX
    with pytest.raises(ValueError, match=r"LDR2_Jacobi.buildK: nx \* ny\^2 = 33227775 exceeds 16777216; the "
                                         r"\[511, 255, 255\] array of per-row propagators is not formed"):
        big.buildK(0.01)
    ok = LDR2_Jacobi(dom, (8, 8), ['sine', 'sine'], mass=[1.0, inertia], dt=0.01)       # 255^3 < 2^24
    assert ok.nx * ok.ny ** 2 <= JACOBI_ROWS_MAX


def test_refusals_carry_their_messages(g):
    from pyqed_amd import LDR2_Jacobi
    dom = [(0.5, 3.5), (0.0, np.pi)]
    with pytest.raises(NotImplementedError, match=r"'gauss_hermite': the reference's branch rebinds its own loop "
                                                  r"variable d \(ldr.py:1816\)"):
        LDR2_Jacobi(dom, (3, 3), ['gauss_hermite', 'sine'])
    with pytest.raises(NotImplementedError, match=r"'fourier': the reference's branch is `pass` \(ldr.py:1824\)"):
        LDR2_Jacobi(dom, (3, 3), ['sine', 'fourier'])
    with pytest.raises(ValueError, match="DVR legendre is not supported. Please use sinc."):
        LDR2_Jacobi(dom, (3, 3), ['sine', 'legendre'])
    with pytest.raises(NotImplementedError, match=r"LDR2_Jacobi is two-dimensional \(ndim=3\)"):
        LDR2_Jacobi(dom + [(0.0, 1.0)], (3, 3, 3), ['sine'] * 3, ndim=3)
    with pytest.raises(AssertionError):
        LDR2_Jacobi(dom, (3, 3, 3), ['sine'] * 2)
    psi0 = g["a_psi0"]
    # only the dense overlap: the existing message
    sol = solver_of(g, "a")
    sol.apes = g["a_apes"]
    sol.A = np.zeros((7, 7, 2, 7, 7, 2))
    with pytest.raises(ValueError, match="LDR2_Jacobi: only the dense overlap A was given; the propagation is "
                                         "matrix-free and needs the states it is built from"):
        sol.run(psi0, 0.05, 2)
    with pytest.raises(ValueError, match="LDR2_Jacobi: set v .* or apes and adiabatic_states first"):
        solver_of(g, "a").run(psi0, 0.05, 2)
    sol = solver_of(g, "a")
    sol.adiabatic_states = g["a_U"]
    with pytest.raises(ValueError, match=r"LDR2_Jacobi: apes \[\*nx, nstates\] must be set with adiabatic_states"):
        sol.run(psi0, 0.05, 2)
    sol.apes = g["a_apes"][:-1]
    with pytest.raises(ValueError, match=r"LDR2_Jacobi: apes must be \(7, 7, 2\); got \(6, 7, 2\)"):
        sol.run(psi0, 0.05, 2)
    sol.adiabatic_states = g["a_U"][..., :1]
    with pytest.raises(ValueError, match=r"LDR2_Jacobi: adiabatic_states must be \(7, 7, 'M', 2\)"):
        sol.run(psi0, 0.05, 2)
    # a moment of inertia that is no callable, or of the wrong shape
    sol = LDR2_Jacobi(dom, (3, 3), ['sine', 'sine'], mass=[1.3, 2.0], dt=0.05)
    with pytest.raises(TypeError, match=r"mass must be \[mx, I\] with I a callable of x"):
        sol.buildK(0.05)
    sol = LDR2_Jacobi(dom, (3, 3), ['sine', 'sine'], mass=[1.3, lambda r: 2.0], dt=0.05)
    with pytest.raises(ValueError, match=r"I\(x\) must have shape \(7,\)"):
        sol.buildK(0.05)
    # the dense propagator above its limit
    big = LDR2_Jacobi(dom, (6, 6), ['sine', 'sine'], mass=[1.3, inertia], dt=0.05)
    with pytest.raises(ValueError, match=r"LDR2_Jacobi.short_time_propagator: D = npts \* nstates = 7938 exceeds 4096"):
        big.short_time_propagator(0.05)


def test_c_entry_checks_come_before_any_device_work():
    """qd_ldr_jacobi_run refuses what its plan refuses and every null pointer it needs, with no GPU in the machine."""
    import ctypes
    from pyqed_amd import _lib
    lib = _lib.load()
    dims = (ctypes.c_int * 2)(5, 4)
    buf = ctypes.create_string_buffer(16 * 5 * 4 * 3 * 2)   # stands for every array: never read, the call is refused
    a = ctypes.addressof(buf)
    fn = "qd_ldr_jacobi_run"

    def call(psi=a, B=1, ndim=2, d=dims, M=3, ns=2, U=a, eV=a, eVh=a, F=a, Fb=a, ph=a, K0=a, K1=None, nsteps=2,
             nout=1, snap=a, path=0):
        rc = lib.qd_ldr_jacobi_run(psi, B, ndim, d, M, ns, U, eV, eVh, F, Fb, ph, K0, K1, nsteps, nout, snap, path,
                                   None)
        return rc, _lib.last_error()

    for kw, msg in ((dict(psi=None), "null psi, U, expV or expVh"), (dict(U=None), "null psi, U, expV or expVh"),
                    (dict(eV=None), "null psi, U, expV or expVh"), (dict(eVh=None), "null psi, U, expV or expVh"),
                    (dict(F=None), "null F, Fb or ph"), (dict(Fb=None), "null F, Fb or ph"),
                    (dict(ph=None), "null F, Fb or ph"), (dict(K0=None), "null K0 with ndim=2"),
                    (dict(snap=None), "null snap with 2 snapshots due"), (dict(d=None), "null dims"),
                    (dict(ndim=4), "ndim=4 outside [1, 3]"), (dict(M=33), "ns=2, M=33 outside 1 <= ns <= M <= 32"),
                    (dict(B=0), "B=0 must be at least 1"),
                    (dict(nout=0), "nsteps=2 must not be negative and nout=0 at least 1"),
                    (dict(path=5), "path=5 outside [0, 2]"),
                    (dict(M=17, path=1), "the fused path needs (16 / M) * M >= 12 columns of a tile (M = 17)")):
        rc, err = call(**kw)
        assert rc == _lib.QD_EINVAL and err == f"{fn}: {msg}", (kw, rc, err)
    # the plain matrices at or past ndim - 1 are ignored; no snapshot due: nothing to compute
    assert call(nsteps=1, nout=2, snap=None, K1=None)[0] == _lib.QD_OK
    assert call(ndim=1, d=(ctypes.c_int * 1)(5), K0=None, nsteps=0, snap=None)[0] == _lib.QD_OK
