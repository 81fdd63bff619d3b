"""Pin the CPU oracle against golden vectors produced by the real reference."""
import numpy as np
import pytest

from conftest import load_golden, relerr
from oracle import lindblad as olb

# oracle vs reference: same fp64 arithmetic up to summation order
TOL = 1e-12


@pytest.mark.parametrize("name", ["lindblad_n4", "lindblad_n16", "lindblad_n40_noc", "lindblad_n128"])
def test_lindblad_oracle_matches_reference(name):
    g = load_golden(name)
    Nt = int(g["Nt"])
    obs, rholist, rho = olb.lindblad(g["H"], g["rho0"], list(g["C"]), list(g["E"]), Nt, float(g["dt"]))
    assert obs.shape == g["observables"].shape
    assert relerr(obs, g["observables"]) < TOL
    if "rholist" in g:
        assert relerr(np.array(rholist), g["rholist"]) < TOL
    else:
        assert relerr(rho, g["rho_final"]) < TOL
    assert np.allclose(g["times"], np.arange(Nt + 1) * float(g["dt"]))


@pytest.mark.parametrize("name", ["redfield_n4", "redfield_n6_k2"])
def test_redfield_oracle_matches_reference(name):
    from conftest import SPECTRA
    from oracle import redfield as orf
    g = load_golden(name)
    spec = SPECTRA[str(g["spectrum"])]
    R, evecs = orf.redfield_tensor(g["H"], list(g["a_ops"]), [spec] * len(g["a_ops"]))
    assert relerr(R, g["R"]) < TOL
    assert relerr(evecs, g["evecs"]) < TOL
    obs, rholist = orf.redfield_evolve(R, g["rho0"], evecs, int(g["Nt"]), float(g["dt"]), list(g["E"]))
    assert obs.shape == g["observables"].shape          # (Nt, ne): t0 excluded
    assert relerr(obs, g["observables"]) < TOL
    assert relerr(np.array(rholist), g["rholist"]) < TOL


def test_correlation_4op_3t_oracle_matches_reference():
    from conftest import SPECTRA
    from oracle import redfield as orf
    g = load_golden("corr4_3level")
    R, _ = orf.redfield_tensor(g["H"], [g["a_op"]], [SPECTRA["flat005"]])
    assert relerr(R, g["R"]) < TOL
    dip = g["dip"]
    for sig in ["lccc", "llll", "lrlr"]:
        cube = orf.correlation_4op_3t(R, g["rho0"], [dip] * 4, sig, g["tau16"])
        assert relerr(cube, g["cube_" + sig]) < 1e-11, sig
    # closed-form slice at fixed tau2 (the 2DES grid evaluator's formula)
    from scipy.linalg import eig, inv
    lam, U1 = eig(R)
    U2 = inv(U1)
    a = b = c = d = None
    ops = [orf.op2sop(dip, s) for s in "lccc"]
    idm = np.identity(3).flatten()
    t = g["tau64"]
    for j, key in [(0, "slice64_j0"), (5, "slice64_j5")]:
        S = orf.response_slice_eig(lam, U1, U2, *ops, g["rho0"].flatten(), idm, t, t[j], t)
        assert relerr(S, g[key]) < 1e-11


def test_corr4_ensemble_oracle():
    from conftest import SPECTRA
    from oracle import redfield as orf
    g = load_golden("corr4_ensemble")
    dip = np.zeros((3, 3)); dip[0, 1] = dip[1, 0] = dip[1, 2] = dip[2, 1] = 1.0
    a = np.diag([0.0, 1.0, 2.0])
    rho0 = np.zeros((3, 3), complex); rho0[0, 0] = 1
    tot = 0
    for m, E in enumerate(g["E"]):
        R, _ = orf.redfield_tensor(np.diag(E), [a], [SPECTRA["flat005"]])
        cube = orf.correlation_4op_3t(R, rho0, [dip] * 4, "lccc", g["tau"])
        assert relerr(cube[:, int(g["j"]), :], g["slices"][m]) < 1e-11
        tot = tot + cube[:, int(g["j"]), :]
    assert relerr(tot, g["ens_sum"]) < 1e-11


@pytest.mark.parametrize("name", ["spo1d_256", "spo1d_256_nout3"])
def test_spo1d_oracle_matches_reference(name):
    from oracle import spo
    g = load_golden(name)
    psilist, psi = spo.spo1d_run(g["x"], g["x"] ** 2 / 2, g["psi0"], float(g["dt"]), int(g["nt"]), int(g["nout"]))
    assert len(psilist) == int(g["nt"]) // int(g["nout"]) - 1
    assert relerr(np.array(psilist).reshape(g["psilist"].shape), g["psilist"]) < TOL
    assert relerr(psi, g["psi"]) < TOL


@pytest.mark.parametrize("name", ["spo2_32", "spo2_64_complex"])
def test_spo2_oracle_matches_reference(name):
    from oracle import spo
    g = load_golden(name)
    n = len(g["x"])
    v = np.zeros((n, n, 2, 2), dtype=complex if np.iscomplexobj(g["coupling"]) else float)
    v[:, :, 0, 0], v[:, :, 1, 1] = g["v0"], g["v1"]
    v[:, :, 0, 1], v[:, :, 1, 0] = g["coupling"], np.conj(g["coupling"])
    eVh, eK = spo.spo2_build(g["x"], g["y"], v, g["masses"], float(g["dt"]))
    if "exp_V_half" in g:
        assert relerr(eVh, g["exp_V_half"]) < TOL
        assert relerr(eK, g["exp_K"]) < TOL
    psilist = spo.spo2_run(eVh, eK, g["psi0"], int(g["nt"]), int(g["nout"]))
    assert len(psilist) == int(g["nt"]) // int(g["nout"]) + 1
    assert relerr(np.array(psilist), g["psilist"]) < TOL


def test_deom_keys_oracle_bit_exact():
    from oracle import deom as od
    g = load_golden("deom_keys")
    for L, K in [(3, 2), (10, 3), (4, 3), (12, 5)]:
        keys, comb = od.gen_keys(L, K)
        assert np.array_equal(keys, g[f"keys_L{L}_K{K}"])
        # graded: tier non-decreasing with index, and hash(key) == index
        tiers = keys.sum(1)
        assert np.all(np.diff(tiers) >= 0)
        assert all(od.gen_hash_value(keys[n], comb) == n for n in range(0, len(keys), 97))


@pytest.mark.parametrize("name", ["deom_run_small", "deom_run_pulsed"])
def test_deom_run_oracle_matches_reference(name):
    from oracle import deom as od
    g = load_golden(name)
    pulses = bool(g["pulses"])
    fs = (lambda t: 0.3 * np.sin(2 * t)) if pulses else (lambda t: 0)
    fc = (lambda t: 0.1 * np.cos(t)) if pulses else (lambda t: 0)
    rho0 = np.zeros((2, 2), complex); rho0[0, 0] = 1
    p1 = np.array([[1, 0], [0, 0]], complex) if "trace_p1" in g else None
    t, saved, ddos = od.run(g["H"], g["sdip"], fs, g["Q"], g["cdip"], fc,
                            (g["etal"], g["etar"], g["etaa"], g["expn"]), int(g["lmax"]), rho0,
                            float(g["dt"]), int(g["nt"]), p1)
    assert np.allclose(t, g["t_save"])
    ref = g["trace_p1"] if p1 is not None else g["rho_sys"]
    assert relerr(saved, ref) < TOL
    assert relerr(ddos, g["ado_final"]) < 1e-12


@pytest.mark.parametrize("tag", ["a", "b"])
def test_tdse_oracle_matches_reference(tag):
    from oracle import tdse as ot
    g = load_golden("sesolver")
    obs, psil = ot.quantum_dynamics(g[f"{tag}_H"], g[f"{tag}_psi0"], float(g[f"{tag}_dt"]), int(g[f"{tag}_Nt"]),
                                    list(g[f"{tag}_E"]), int(g[f"{tag}_nout"]))
    assert relerr(obs, g[f"{tag}_obs"]) < 1e-12
    assert relerr(psil, g[f"{tag}_psilist"]) < 1e-12


@pytest.mark.parametrize("tag", ["a", "b"])
def test_tdse_driven_oracle_matches_reference(tag):
    from oracle import tdse as ot
    g = load_golden("tdse_driven")
    d = g[f"{tag}_d"]
    pulses = np.atleast_2d(g[f"{tag}_pulse"])
    dips = [d] if d.ndim == 2 else list(d)
    drives = [(dp, ot.gaussian_efield(*p)) for dp, p in zip(dips, pulses)]
    obs, psit, psil = ot.driven_dynamics(g[f"{tag}_H"], drives, g[f"{tag}_psi0"], float(g[f"{tag}_dt"]),
                                         int(g[f"{tag}_Nt"]), list(g[f"{tag}_E"]), int(g[f"{tag}_nout"]),
                                         float(g[f"{tag}_t0"]))
    assert relerr(obs, g[f"{tag}_obs"]) < 1e-12
    assert relerr(psit, g[f"{tag}_psit"]) < 1e-12
    assert relerr(psil, g[f"{tag}_psilist"]) < 1e-12


def test_spo2nh_oracle_matches_reference():
    from oracle import spo
    g = load_golden("spo2nh_32")
    eV, eVh = spo.spo2nh_build(g["v"], float(g["dt"]))
    assert relerr(eV, g["exp_V"]) < TOL
    assert relerr(eVh, g["exp_V_half"]) < TOL
    x, y = g["x"], g["y"]
    X, Y = np.meshgrid(x, y, indexing="ij")
    n = len(x)
    kx = 2 * np.pi * np.fft.fftfreq(n, x[1] - x[0])
    ky = 2 * np.pi * np.fft.fftfreq(n, y[1] - y[0])
    Kx, Ky = np.meshgrid(kx, ky, indexing="ij")
    keo = spo.keo_linear(np.exp(-1j * (Kx ** 2 / 2 + Ky ** 2 / 2) * float(g["dt"])))
    nt, nout = int(g["nt"]), int(g["nout"])
    pl, psi = spo.spo2_strang_run(eVh, keo, g["psi0"], nt, nout)
    assert relerr(np.array(pl), g["strang_psilist"]) < TOL
    assert relerr(psi, g["strang_psi"]) < TOL
    pl, psi = spo.spo2_merged_run(eV, eVh, keo, g["psi0"], nt, nout)
    assert relerr(np.array(pl), g["merged_psilist"]) < TOL
    assert relerr(psi, g["merged_psi"]) < TOL


def test_spo2_jacobi_oracle_matches_reference():
    from oracle import spo
    g = load_golden("spo2_jacobi_32")
    a, b = g["inertia"]
    eKx, eKy = spo.jacobi_ops(g["x"], g["y"], 1.0, lambda r: a + b * r ** 2, float(g["dt"]))
    assert relerr(eKx, g["exp_Kx"]) < TOL
    assert relerr(eKy, g["exp_Ky"]) < TOL
    n = len(g["x"])
    v = np.zeros((n, n, 2, 2))
    v[:, :, 0, 0], v[:, :, 1, 1] = g["v0"], g["v1"]
    v[:, :, 0, 1] = v[:, :, 1, 0] = g["coupling"]
    eVh, _ = spo.spo2_build(g["x"], g["y"], v, [1.0, 1.0], float(g["dt"]))
    pl, _ = spo.spo2_strang_run(eVh, spo.keo_jacobi(eKx, eKy), g["psi0"], int(g["nt"]), int(g["nout"]))
    assert relerr(np.array(pl), g["psilist"]) < TOL


def _parse_dat(text):
    rows = [ln.split() for ln in str(text).splitlines()]
    return np.array([float(r[0]) for r in rows]), np.array([[complex(v) for v in r[1:]] for r in rows])


def test_correlation_3p_1t_oracle_matches_reference():
    g = load_golden("corr3p_1t")
    assert bool(g["returned_none"])
    t, cor, rhos = olb.correlation_3p_1t(g["H"], g["rho0"], [g["A"], g["B"], g["Cop"]], [g["C"]], g["tlist"])
    tr, cr = _parse_dat(g["cordat"])
    assert np.array_equal(t, tr)                         # same float accumulation t += dt
    assert relerr(cor, cr[:, 0]) < TOL
    td, dm = _parse_dat(g["dmdat"])
    assert np.array_equal(td, tr) and relerr(rhos.reshape(len(t), -1), dm) < TOL


def test_deom_corr4_oracle_matches_reference():
    from oracle import deom as od
    g = load_golden("deom_corr4")
    K = len(g["expn"])
    keys, comb = od.gen_keys(int(g["lmax"]), K)
    P = od.propagator(keys, comb, int(g["lmax"]), g["expn"], g["etal"], g["etar"], g["etaa"], np.zeros(K, int),
                      g["H"], g["Q"])
    assert relerr(P, g["propagator"]) < 1e-14
    sx = g["Q"][0]
    sz = np.diag([1.0, -1.0]).astype(complex)
    args = (int(g["nmax"]), 2)
    for lcr in ["llll", "lrlr", "lccc"]:
        cw = od.correlation_4op_3t(P, *args, [sx] * 4, g["rho0"], float(g["T"]), g["wx"], g["wy"], lcr=lcr)
        assert relerr(cw, g["cw_" + lcr]) < 1e-12, lcr
    # The reference's default cuts (min(Re) * 0.5 < Re < max(Re) * 1.1) sit on two eigenvalues of this hierarchy to the
    # last bits, so the rounding of the eigensolver, which changes with the BLAS thread count and the CPU, decides what
    # is kept.  The fixture's run kept 100 of the 140: it dropped the eigenvalue at Re = min(Re) / 2 (its term is 7e-9
    # of the signal) and kept the steady state (Re = 0 up to rounding, 96 % of the signal), which `Re < 1.1 max(Re)`
    # keeps only when that rounding came out positive.  The cuts below select the fixture's set on every host: the
    # lower one 1e-6 higher, the upper one on the steady state's far side whatever its sign; the next eigenvalues are
    # 0.42 away from either cut.  With the set fixed, this run and the fixture's differ by the rounding of two eigen
    # decompositions: the signal chains two similarity transforms V^-1 A V, each good to eps cond(V), so the bound is
    # eps cond(V)^2 with a factor 10 for the sums over the 140 modes (cond(V) = 58: 7.5e-12).  The old 1e-12 held only
    # where the eigensolver's rounding repeated the fixture's bit for bit.
    import scipy.linalg as la
    lam, V = la.eig(P)                                   # the oracle's own eigensolver call
    top = np.real(lam).max()
    assert abs(top) < 1e-12
    bound = 10 * np.finfo(float).eps * np.linalg.cond(V) ** 2
    cw = od.correlation_4op_3t(P, *args, [sz, sx, sx, sz], g["rho0"], float(g["T"]), g["wx"], g["wy"], if_full=False,
                               cut_off_min=0.5 - 1e-6, cut_off_max=1.1 if top > 0 else 0.9)
    assert relerr(cw, g["cw_cut_llll"]) < bound < 1e-11


@pytest.mark.parametrize("name", ["spo2_20x20", "spo2_96x80", "spo2_67x45_ns3", "spo2_12x10_ns9"])
def test_spo2_rect_oracle_matches_reference(name):
    """Non-power-of-two grids and ns > 2 (make_golden _spo2_rect_case): the oracle's SPO2 restatement equals the
    reference run (scipy.fftpack takes every length, wpd.py:837-848)."""
    from oracle import spo
    from spo_models import spo2_model_rect, spo2_potential
    g = load_golden(name)
    nx, ny, ns = int(g["nx"]), int(g["ny"]), int(g["ns"])
    x, y, surfaces, couplings, psi0 = spo2_model_rect(nx, ny, ns)
    v = spo2_potential(surfaces, couplings, ns)
    eVh, eK = spo.spo2_build(x, y, v, (1.0, 1.3), float(g["dt"]))
    psilist = spo.spo2_run(eVh, eK, psi0, int(g["nt"]), int(g["nout"]))
    assert len(psilist) == int(g["n_psilist"])
    assert relerr(np.array(psilist), g["psilist"]) < 1e-12


def test_spo3_rect_oracle_matches_reference():
    from oracle import spo
    from spo_models import spo3_model
    g = load_golden("spo3_24x20x18")
    (x, y, z), masses, surfaces, couplings, psi0 = spo3_model()
    ns = 2
    v = np.zeros(psi0.shape + (ns,))
    v[..., 0, 0], v[..., 1, 1] = surfaces
    v[..., 0, 1] = v[..., 1, 0] = couplings[0][1]
    w, u = np.linalg.eigh(v)
    ud = np.conj(np.swapaxes(u, -1, -2))
    eVh = (u * np.exp(-1j * w * float(g["dt"]) / 2)[..., None, :]) @ ud
    from scipy.fftpack import fftfreq
    ks = [2 * np.pi * fftfreq(len(a), a[1] - a[0]) for a in (x, y, z)]
    Kx, Ky, Kz = np.meshgrid(*ks, indexing="ij")
    eK = np.exp(-1j * (Kx ** 2 / 2 / masses[0] + Ky ** 2 / 2 / masses[1] + Kz ** 2 / 2 / masses[2]) * float(g["dt"]))
    psilist, psi = spo.spo3_run(eVh, eK, psi0, int(g["nt"]), int(g["nout"]))
    assert relerr(np.array(psilist), g["psilist"]) < 1e-12
    assert relerr(psi, g["psi"]) < 1e-12


def test_spo1d_any_oracle_matches_reference():
    from oracle import spo
    from spo_models import spo1d_model
    g = load_golden("spo1d_any")
    for n in g["sizes"]:
        x, psi0 = spo1d_model(int(n))
        pl, psi = spo.spo1d_run(x, x ** 2 / 2, psi0, 0.01, int(g[f"n{n}_nt"]), int(g[f"n{n}_nout"]))
        assert relerr(psi, g[f"n{n}_psi"]) < 1e-12, n
        if len(pl):
            assert relerr(np.array(pl), g[f"n{n}_psilist"]) < 1e-12, n


@pytest.mark.parametrize("tag", ["ex", "mild"])
def test_heom_chain_oracle_matches_reference(tag):
    """oracle.heom restates HEOM/heom.py:275-347 (RK4) and oqs.py:1808-1875 (Euler sweep)."""
    from oracle import heom as oh
    g = load_golden("heom_chain")
    sx = np.array([[0, 1], [1, 0]], complex)
    args = (g["H"], g["Q"], g["rho0"], [g["Q"], sx], float(g[f"{tag}_temperature"]), float(g[f"{tag}_cutoff"]),
            float(g[f"{tag}_reorganization"]), int(g[f"{tag}_nado"]), float(g[f"{tag}_dt"]), int(g[f"{tag}_nt"]))
    assert relerr(oh.chain_rk4(*args), g[f"{tag}_rk4"]) < 1e-12
    assert relerr(oh.chain_euler(*args), g[f"{tag}_euler"]) < 1e-12


def test_oracle_fft_matches_reference_golden():
    """oracle/fft.py (the checker of pyqed_amd.fft) against the reference's own outputs at every fixture length,
    norm / n kwargs and axes (fft_phys, fft_any)."""
    from oracle import fft as of
    g = load_golden("fft_phys")
    assert relerr(of.fft(g["a"], g["x"])[0], g["fft_g"]) < 1e-12
    assert relerr(of.ifft(g["a"], g["x"])[0], g["ifft_g"]) < 1e-12
    assert relerr(of.fft(g["M"], x=np.linspace(0, 3.1, 32), axis=0)[0], g["fftax0_g"]) < 1e-12
    g = load_golden("fft_any")
    for n in (8, 1000, 2048, 4096, 5000, 7919, 12288):
        assert relerr(of.fft(g[f"a{n}"], g[f"x{n}"])[0], g[f"fft{n}_g"]) < 1e-12
        assert relerr(of.ifft(g[f"a{n}"], g[f"x{n}"])[0], g[f"ifft{n}_g"]) < 1e-12
    assert relerr(of.fft(g["a5000"], g["x5000"], norm="ortho")[0], g["fft5000_ortho_g"]) < 1e-12
    assert relerr(of.fft(g["a1000"], g["x1000"], n=1)[0], g["fft1000_n1_g"]) < 1e-12
    assert relerr(of.fft(g["T"], g["xt"], axis=0)[0], g["fftT0_g"]) < 1e-12
    assert relerr(of.ifft(g["T"], np.linspace(-1, 1, 7), axis=-1)[0], g["ifftTm1_g"]) < 1e-12
