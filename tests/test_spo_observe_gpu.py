"""Populations, mean positions and the electronic reduced density matrix reduced on the device (qd_spo_observe,
pyqed_amd/csrc/spo_observe.hip), after a run from states and inside the run loops (qd_spo2_run_observed /
qd_spo3_run_observed, run(..., observe=...)).

The comparator is the numpy einsum below.  Tolerances: both sides sum at most 2^17 products in fp64 in a tree-like
order, so each is within about log2(n) eps ~ 2e-15 of sum |terms|; 1e-13 leaves 50x (the moment axes are offset from
zero so that no row of mom is a near-cancellation).  Against the reference's own numbers on identical states only the
summation order differs: 1e-12.  In-run against post-hoc is the same kernel on the same bytes: bit for bit."""
import numpy as np
import pytest
import torch

from conftest import load_golden, relerr, took
from spo_models import spo2_model_rect, spo3_model

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


# ------------------------------------------------------------------ comparator
def np_observe(psi, axes, basis=None, weight=1.0):
    """psi [B, n0, ..., ns] -> rdm [B, ns, ns], mom [B, ndim, ns] (float64 einsum)."""
    nd = len(axes)
    chi = psi if basis is None else np.einsum('...ab,k...b->k...a', basis, psi)
    B, ns = chi.shape[0], chi.shape[-1]
    flat = chi.reshape(B, -1, ns)
    rdm = weight * np.einsum('kpa,kpb->kab', flat.conj(), flat)
    dens = np.abs(chi) ** 2
    mom = np.empty((B, nd, ns))
    for d, xd in enumerate(axes):
        shape = [1] * (nd + 2)
        shape[1 + d] = len(xd)
        mom[:, d] = weight * (dens * np.asarray(xd).reshape(shape)).reshape(B, -1, ns).sum(axis=1)
    return rdm, mom


def _axes(dims):
    return [np.linspace(1.0 + 0.5 * d, 2.5 + 0.7 * d, n) for d, n in enumerate(dims)]   # offset from zero


def _states(rng, B, dims, ns, weight):
    psi = rng.standard_normal((B,) + dims + (ns,)) + 1j * rng.standard_normal((B,) + dims + (ns,))
    for b in range(B):
        psi[b] /= np.sqrt(np.vdot(psi[b], psi[b]).real * weight)    # ||psi||^2 w = 1
    return psi


def _bases(rng, dims, ns):
    real = rng.standard_normal(dims + (ns, ns))
    return {"none": None, "real": real, "complex": real + 1j * rng.standard_normal(dims + (ns, ns))}


SHAPES = [((12, 10), 1, "spo_obs_reg"), ((12, 10), 2, "spo_obs_reg"), ((12, 10), 3, "spo_obs_reg"),
          ((12, 10), 4, "spo_obs_reg"),          # fewer points than one workgroup, idle lanes
          ((67, 45), 3, "spo_obs_reg"),          # 3015 points: ragged multi-block tail
          ((256, 256), 2, "spo_obs_reg"),        # many partial rows, chunked second stage
          ((24, 20, 18), 2, "spo_obs_reg"),      # 3-axis index decomposition, unequal dims
          ((100,), 1, "spo_obs_reg"),            # 1D
          ((12, 10), 9, "spo_obs_gen")]          # generic path (with and without the chi pre-pass)


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("dims,ns,path", SHAPES)
def test_observe_matches_numpy(dims, ns, path, B):
    from pyqed_amd.wpd import observe_states
    rng = np.random.default_rng(100 * len(dims) + 10 * ns + B)
    axes = _axes(dims)
    w = float(np.prod([a[1] - a[0] for a in axes]))
    psi = _states(rng, B, dims, ns, w)
    t = torch.from_numpy(psi).to(DEV)
    for name, basis in _bases(rng, dims, ns).items():
        ref_rdm, ref_mom = np_observe(psi, axes, basis, w)
        for moments in (True, False):
            took("")
            rdm, mom = observe_states(t if B > 1 else t[0], axes, basis=basis, moments=moments)
            hit, got = took(path)
            assert hit, got
            rdm2, mom2 = observe_states(t if B > 1 else t[0], axes, basis=basis, moments=moments)
            assert torch.equal(rdm, rdm2)
            r = rdm.cpu().numpy().reshape(B, ns, ns)
            e = relerr(r, ref_rdm)
            print(f"{dims} ns={ns} B={B} basis={name} mom={moments}: rdm {e:.2e}", end="")
            assert e < 1e-13, (name, moments, e)
            assert np.array_equal(r, np.conj(np.swapaxes(r, -1, -2)))            # lower triangle = conj(upper)
            assert np.all(np.einsum('kaa->ka', r).imag == 0.0)                    # exactly real diagonal
            if moments:
                assert torch.equal(mom, mom2)
                em = relerr(mom.cpu().numpy().reshape(B, len(dims), ns), ref_mom)
                print(f" mom {em:.2e}")
                assert em < 1e-13, (name, em)
            else:
                print()
                assert mom is None
        if name == "none":
            assert abs(np.einsum('kaa->', r).real - B) < 1e-12    # normalised input


def test_observe_weight_and_batch_layout():
    """An explicit weight scales both outputs; member b of a batch equals the same state observed alone, bit for bit
    (the partial rows of a member do not depend on the batch)."""
    from pyqed_amd.wpd import observe_states
    rng = np.random.default_rng(8)
    dims, ns = (67, 45), 3
    axes = _axes(dims)
    psi = torch.from_numpy(_states(rng, 3, dims, ns, 1.0)).to(DEV)
    rdm, mom = observe_states(psi, axes, weight=1.0)
    for b in range(3):
        r1, m1 = observe_states(psi[b], axes, weight=1.0)
        assert torch.equal(r1, rdm[b]) and torch.equal(m1, mom[b])
    r2, m2 = observe_states(psi, axes, weight=0.25)
    assert relerr(r2.cpu().numpy(), 0.25 * rdm.cpu().numpy()) < 1e-15
    assert relerr(m2.cpu().numpy(), 0.25 * mom.cpu().numpy()) < 1e-15


# ------------------------------------------------------------------ reference parity of the kernel alone
def _spo2_for(x, y, ns, mass=(1.0, 1.3)):
    from pyqed_amd import SPO2
    return SPO2(x, y, mass=list(mass), nstates=ns)


def _check_against_fixture(sol, states, g, tag):
    states = [np.asarray(s) for s in states]
    assert relerr(sol.population(states), g[f"{tag}_pop"]) < 1e-12
    sol.d2a = g[f"{tag}_d2a"]
    assert relerr(sol.population(states, 'adiabatic'), g[f"{tag}_pop_adiabatic"]) < 1e-12
    rho = sol.rdm_el(states)
    assert isinstance(rho, list) and len(rho) == len(states)
    assert relerr(np.array(rho), g[f"{tag}_rdm"]) < 1e-12
    from pyqed_amd.wpd import observe_states
    _, mom = observe_states(np.array(states), (sol.x, sol.y))
    mom = mom.cpu().numpy()
    assert relerr(mom[:, 0].sum(-1), g[f"{tag}_xAve"]) < 1e-12
    if tag == "a":
        assert relerr(mom[:, 1].sum(-1), g[f"{tag}_yAve"]) < 1e-12
    else:   # spo2_32 is symmetric in y: <y> is a cancellation to ~1e-17, bounded against sum |y| |psi|^2 w <= max |y|
        assert np.abs(mom[:, 1].sum(-1) - g[f"{tag}_yAve"]).max() < 1e-12 * np.abs(sol.y).max()
    # the other input forms: one ndarray -> [ns] / [ns, ns]; a stacked array; a device tensor (read in place)
    p1 = sol.population(states[-1])
    assert p1.shape == (sol.ns,) and relerr(p1, g[f"{tag}_pop"][-1]) < 1e-12
    assert relerr(sol.population(states[-1], 'adiabatic'), g[f"{tag}_pop_adiabatic"][-1]) < 1e-12
    r1 = sol.rdm_el(states[-1])
    assert r1.shape == (sol.ns, sol.ns) and relerr(r1, g[f"{tag}_rdm"][-1]) < 1e-12
    stacked = np.array(states)
    assert np.array_equal(sol.population(stacked), sol.population(states))
    assert np.array_equal(sol.population(torch.from_numpy(stacked).to(DEV)), sol.population(states))


def test_fixture_case_a():
    """24 x 20 x 3, packet displaced in x and y (tests/golden/make_golden_spoobs.py)."""
    g = load_golden("spo_observables")
    nx, ny, ns = int(g["a_nx"]), int(g["a_ny"]), int(g["a_ns"])
    x, y, _, _, _ = spo2_model_rect(nx, ny, ns)
    assert abs(g["a_yAve"]).min() > 0.5     # <y> is signal, not rounding noise
    _check_against_fixture(_spo2_for(x, y, ns), list(g["a_psilist"]), g, "a")


def test_fixture_case_b():
    """The states of spo2_32.npz."""
    g = load_golden("spo_observables")
    s = load_golden("spo2_32")
    _check_against_fixture(_spo2_for(s["x"], s["y"], 2, (1.0, 1.0)), list(s["psilist"]), g, "b")


@pytest.mark.parametrize("name,path", [("spo2_67x45_ns3", "spo_obs_reg"), ("spo2_12x10_ns9", "spo_obs_gen")])
def test_populations_of_stored_reference_states(name, path):
    g = load_golden(name)
    nx, ny, ns = int(g["nx"]), int(g["ny"]), int(g["ns"])
    x, y, _, _, _ = spo2_model_rect(nx, ny, ns)
    sol = _spo2_for(x, y, ns)
    took("")
    rho = np.array(sol.rdm_el(list(g["psilist"])))
    assert took(path)[0]
    assert relerr(np.einsum('kaa->ka', rho).real, g["populations"]) < 1e-12
    assert relerr(sol.population(list(g["psilist"])), g["populations"]) < 1e-12


def test_spo3_population_sums_the_whole_grid():
    from pyqed_amd import SPO3
    (x, y, z), masses, _, _, psi0 = spo3_model()
    sol = SPO3(x, y, z, masses=masses, nstates=2)
    w = (x[1] - x[0]) * (y[1] - y[0]) * (z[1] - z[0])
    ref = np.array([np.sum(np.abs(psi0[..., a]) ** 2) * w for a in range(2)])
    assert relerr(sol.population(psi0), ref) < 1e-13
    assert relerr(sol.population([psi0, 2 * psi0]), np.array([ref, 4 * ref])) < 1e-13
    assert relerr(sol.rdm_el(psi0), np_observe(psi0[None], (x, y, z), None, w)[0][0]) < 1e-13


# ------------------------------------------------------------------ in-run equals post-hoc, bit for bit
STEPS = [(3, 1),    # nout = 1: the slot is reused on consecutive steps
         (7, 3),    # nt // nout * nout < nt; the last recorded step is the last step (no V/2 reopen)
         (0, 1)]    # nothing recorded: row 0 only


def _spo2_case(nx, ny, ns, jacobi=False):
    from pyqed_amd import SPO2
    x, y, surfaces, couplings, psi0 = spo2_model_rect(nx, ny, ns)
    X, Y = np.meshgrid(x, y, indexing="ij")
    psi0 = psi0 * np.exp(-0.4j * Y - 0.3 * Y)[:, :, None]     # <y> != 0
    if jacobi:
        sol = SPO2(x, y, mass=[1.0, lambda q: 1.5 + 0.2 * q ** 2], nstates=ns, coords='jacobi')
    else:
        sol = SPO2(x, y, mass=[1.0, 1.3], nstates=ns)
    sol.set_DPES(surfaces, couplings)
    return sol, psi0


def _posthoc(states, axes, basis=None):
    """rdm, mom of host states through qd_spo_observe."""
    from pyqed_amd.wpd import observe_states
    rdm, mom = observe_states(np.array(states), axes, basis=basis)
    return rdm.cpu().numpy(), mom.cpu().numpy()


def _assert_recorded(ro, states, axes, basis=None):
    rdm, mom = _posthoc(states, axes, basis)
    assert ro.rdm.shape == rdm.shape and np.array_equal(ro.rdm, rdm)
    assert np.array_equal(ro.population, np.einsum('kaa->ka', rdm).real)
    assert len(ro.xAve) == len(axes)
    for d in range(len(axes)):
        assert np.array_equal(ro.xAve[d], mom[:, d].sum(axis=-1))


@pytest.mark.parametrize("nt,nout", STEPS)
@pytest.mark.parametrize("nx,ny,ns,jacobi,loop", [(32, 32, 2, False, "spo2_pow2"),     # fast row / column kernels
                                                  (16, 16, 4, False, "spo2_pow2"),     # LDS-row kernel
                                                  (30, 22, 2, False, "spo_any"),       # any-size engine, alternating
                                                  (32, 32, 2, True, "spo2_pow2")])     # Jacobi expKy
def test_spo2_run_observed_equals_posthoc(nx, ny, ns, jacobi, loop, nt, nout):
    sol, psi0 = _spo2_case(nx, ny, ns, jacobi)
    r = sol.run(psi0, dt=0.05, nt=nt, nout=nout)
    took("")
    ro = sol.run(psi0, dt=0.05, nt=nt, nout=nout, observe='diabatic', return_states=False)
    got = took("")[1]
    assert nt == 0 or (loop in got and "spo_obs_reg" in got), got     # a run of no steps launches nothing
    assert len(ro.psilist) == 1 and ro.psilist[0] is psi0
    assert np.array_equal(ro.psi, r.psi)
    assert ro.rdm.shape == (nt // nout + 1, ns, ns)
    _assert_recorded(ro, r.psilist, (sol.x, sol.y))
    assert ro.get_population() is ro.population


def test_spo2_any_grid_in_place_loop_observed():
    """A direct-DFT axis (2579 points, prime beyond the chirp-z plan) takes run_nd's in-place loop, the one 3D grids
    take too."""
    sol, psi0 = _spo2_case(2579, 12, 2)
    r = sol.run(psi0, dt=0.05, nt=3, nout=1)
    took("")
    ro = sol.run(psi0, dt=0.05, nt=3, nout=1, observe='diabatic', return_states=False)
    got = took("")[1]
    assert "spo_layout_in_place" in got and "spo_obs_reg" in got, got
    assert np.array_equal(ro.psi, r.psi)
    _assert_recorded(ro, r.psilist, (sol.x, sol.y))


@pytest.mark.parametrize("observe", ["adiabatic", "explicit"])
def test_spo2_run_observed_with_a_basis(observe):
    """observe='adiabatic' applies d2a as the reference's population does (M = d2a); an explicit array is applied as
    given (here the adjoint: projections on the eigenvector columns)."""
    sol, psi0 = _spo2_case(30, 22, 3)
    r = sol.run(psi0, dt=0.05, nt=4, nout=2)
    d2a = np.asarray(sol.d2a)
    M = d2a if observe == "adiabatic" else np.conj(np.swapaxes(d2a, -1, -2))
    ro = sol.run(psi0, dt=0.05, nt=4, nout=2, return_states=False, observe=observe if observe == "adiabatic" else M)
    _assert_recorded(ro, r.psilist, (sol.x, sol.y), basis=M)
    ref_rdm, _ = np_observe(np.array(r.psilist), (sol.x, sol.y), M, sol.dx * sol.dy)
    assert relerr(ro.rdm, ref_rdm) < 1e-13
    if observe == "adiabatic":
        assert np.array_equal(ro.population, sol.population(r.psilist, 'adiabatic'))


@pytest.mark.parametrize("nt,nout", STEPS)
def test_spo2_run_batch_observed_equals_posthoc(nt, nout):
    """256 x 256 x 2 with B = 3: the batch loop (that shape alone reaches it), one slot per member."""
    from pyqed_amd import SPO2
    from pyqed_amd.wpd import observe_states
    n, B = 256, 3
    x, y, surfaces, couplings, psi0 = spo2_model_rect(n, n, 2)
    sol = SPO2(x, y, mass=[1.0, 1.3], nstates=2)
    sol.set_DPES(surfaces, couplings)
    X, Y = np.meshgrid(x, y, indexing="ij")
    psi0s = np.stack([psi0 * np.exp(1j * 0.3 * b * Y - 0.1 * b * Y)[:, :, None] for b in range(B)])
    took("")
    psi, snap = sol.run_batch(psi0s, dt=0.05, nt=nt, nout=nout)
    assert nt == 0 or took("spo2_batch256")[0]
    took("")
    psi2, none, obs = sol.run_batch(psi0s, dt=0.05, nt=nt, nout=nout, observe='diabatic', keep_states=False)
    got = took("")[1]
    assert nt == 0 or ("spo2_batch256" in got and "spo_obs_reg" in got), got
    assert none is None and torch.equal(psi, psi2)
    nsnap = nt // nout
    assert obs["rdm"].shape == (B, nsnap, 2, 2) and obs["mom"].shape == (B, nsnap, 2, 2)
    if nsnap:
        rdm, mom = observe_states(snap.reshape((B * nsnap,) + tuple(snap.shape[2:])), (x, y))
        assert torch.equal(obs["rdm"], rdm.reshape(B, nsnap, 2, 2))
        assert torch.equal(obs["mom"], mom.reshape(B, nsnap, 2, 2))
        assert torch.equal(obs["population"], torch.diagonal(obs["rdm"], dim1=-2, dim2=-1).real)
        # and with the states kept: the same three outputs
        psi3, snap3, obs3 = sol.run_batch(psi0s, dt=0.05, nt=nt, nout=nout, observe='diabatic')
        assert torch.equal(psi3, psi) and torch.equal(snap3, snap)
        assert torch.equal(obs3["rdm"], obs["rdm"]) and torch.equal(obs3["mom"], obs["mom"])


def _spo3_case(n, path):
    from pyqed_amd import SPO3
    if n is None:
        (x, y, z), masses, surfaces, couplings, psi0 = spo3_model()
    else:
        x, y, z = np.linspace(-6, 6, n), np.linspace(-5, 5, n), np.linspace(-5.5, 5.5, n)
        X, Y, Z = np.meshgrid(x, y, z, indexing="ij")
        surfaces = [0.5 * ((X + 1) ** 2 + Y ** 2 + Z ** 2), 0.5 * ((X - 1) ** 2 + Y ** 2 + Z ** 2)]
        couplings = [[[0, 1], 0.2 * X]]
        masses = [1.0, 1.2, 0.9]
        psi0 = np.zeros((n, n, n, 2), dtype=complex)
        psi0[..., 1] = np.exp(-((X + 1) ** 2 + (Y - 0.5) ** 2 + (Z + 0.7) ** 2) / 2 + 0.3j * Y) / np.pi ** 0.75
    sol = SPO3(x, y, z, masses=masses, nstates=2)
    sol.kinetic_path = path
    sol.set_DPES(surfaces, couplings)
    return sol, psi0


@pytest.mark.parametrize("nt,nout", STEPS)
@pytest.mark.parametrize("n,path,loop", [(16, "fft", "spo3_pow2"), (None, "axes", "spo3_axes"),
                                         (None, "fft", "spo_any"),       # 24 x 20 x 18: run_nd's in-place loop
                                         (64, "axes", "spo3_sep64")])    # 8 MiB states
def test_spo3_run_observed_equals_posthoc(n, path, loop, nt, nout):
    if n == 64 and nout == 1:
        nt = 2
    sol, psi0 = _spo3_case(n, path)
    r = sol.run(psi0, dt=0.1, nt=nt, nout=nout)
    took("")
    ro = sol.run(psi0, dt=0.1, nt=nt, nout=nout, observe='diabatic', return_states=False)
    got = took("")[1]
    assert nt == 0 or (loop in got and "spo_obs_reg" in got), got
    assert ro.psilist == []
    assert np.array_equal(ro.psi, r.psi)
    assert ro.rdm.shape == (nt // nout + 1, 2, 2)
    _assert_recorded(ro, [psi0] + list(r.psilist), (sol.x, sol.y, sol.z))


# ------------------------------------------------------------------ in-run against the reference
def test_spo2_256_populations_without_states():
    from pyqed_amd import SPO2
    g = load_golden("spo2_256")
    n = int(g["n"])
    x = np.linspace(-6, 6, n)
    X, Y = np.meshgrid(x, x, indexing="ij")
    sol = SPO2(x, x, mass=[1.0, 1.0], nstates=2)
    sol.set_DPES([0.5 * ((X + 1) ** 2 + Y ** 2), 0.5 * ((X - 1) ** 2 + Y ** 2) + 0.1], [[[0, 1], 0.2 * X]])
    psi0 = np.zeros((n, n, 2), complex)
    psi0[:, :, 0] = np.exp(-((X + 1.5) ** 2 + Y ** 2) / 2 + 0.5j * X) / np.sqrt(np.pi)
    r = sol.run(psi0, dt=float(g["dt"]), nt=int(g["nt"]), nout=int(g["nout"]), observe='diabatic', return_states=False)
    assert len(r.psilist) == 1
    assert relerr(r.population, g["populations"]) < 1e-10
    assert relerr(r.get_population(), g["populations"]) < 1e-10
    assert relerr(r.psi, g["psi_final"]) < 1e-10


def test_spo2_67x45_ns3_populations_without_states():
    g = load_golden("spo2_67x45_ns3")
    x, y, surfaces, couplings, psi0 = spo2_model_rect(67, 45, 3)
    sol = _spo2_for(x, y, 3)
    sol.set_DPES(surfaces, couplings)
    r = sol.run(psi0, dt=float(g["dt"]), nt=int(g["nt"]), nout=int(g["nout"]), observe='diabatic', return_states=False)
    assert len(r.psilist) == 1
    assert relerr(r.population, g["populations"]) < 1e-10


def test_spo2nh_populations_decay(tmp_path, monkeypatch):
    """Non-unit norm: the absorbing potential of spo2nh_32; populations against those of the reference's Strang states."""
    from pyqed_amd import SPO2NH
    monkeypatch.chdir(tmp_path)
    g = load_golden("spo2nh_32")
    x, y = g["x"], g["y"]
    sol = SPO2NH(x, y, mass=[1.0, 1.0], nstates=2)
    sol.set_dpes(g["v"])
    r = sol.run(g["psi0"], dt=float(g["dt"]), nt=int(g["nt"]), nout=int(g["nout"]), observe='diabatic',
                return_states=False)
    assert len(r.psilist) == 1
    w = (x[1] - x[0]) * (y[1] - y[0])
    states = g["strang_psilist"]
    ref = np.array([[np.vdot(p[:, :, k], p[:, :, k]).real * w for k in range(2)] for p in states])
    assert relerr(r.population, ref) < 1e-10
    tot = r.population.sum(axis=1)
    assert tot[-1] < tot[0] and tot[-1] < 1.0 and np.all(np.diff(tot) < 0)
    xr = np.array([np.einsum('ijn,i->', np.abs(p) ** 2, x) * w for p in states])
    assert relerr(r.position()[0], xr) < 1e-10


# ------------------------------------------------------------------ both outputs together
@pytest.mark.parametrize("kind", ["spo2_pow2", "spo_any", "spo3_axes"])
def test_states_and_observables_together(kind):
    if kind == "spo3_axes":
        sol, psi0 = _spo3_case(None, "axes")
        kw = dict(dt=0.1, nt=4, nout=2)
    else:
        sol, psi0 = _spo2_case(*((32, 32, 2) if kind == "spo2_pow2" else (30, 22, 2)))
        kw = dict(dt=0.05, nt=4, nout=2)
    r = sol.run(psi0, **kw)
    ro = sol.run(psi0, observe='diabatic', return_states=False, **kw)
    both = sol.run(psi0, observe='diabatic', return_states=True, **kw)
    assert len(both.psilist) == len(r.psilist)
    assert all(np.array_equal(a, b) for a, b in zip(both.psilist, r.psilist))
    assert np.array_equal(both.psi, r.psi)
    assert np.array_equal(both.rdm, ro.rdm) and np.array_equal(both.population, ro.population)
    assert all(np.array_equal(a, b) for a, b in zip(both.xAve, ro.xAve))


# ------------------------------------------------------------------ graph capture
def test_observed_run_replays_from_a_graph():
    """qd_spo2_run_observed at 32 x 32 x 2 without snapshots (the slot and the partial rows are buffers the graph
    owns), captured once; an uncaptured library call between the replays takes arena scratch of its own; every replay
    equals the direct call bit for bit."""
    from pyqed_amd import _lib
    lib = _lib.load()
    n, ns, nsteps, nout = 32, 2, 6, 2
    rng = np.random.default_rng(4)
    a = rng.standard_normal((n, n, ns, ns)) + 1j * rng.standard_normal((n, n, ns, ns))
    w_, u = np.linalg.eigh((a + np.conj(np.swapaxes(a, -1, -2))) / 4)
    t = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(DEV)
    U = t((u * np.exp(-0.5j * w_)[..., None, :]) @ np.conj(np.swapaxes(u, -1, -2)))
    K = t(np.exp(-1j * rng.uniform(0, 6, (n, n))))
    psi0 = t(rng.standard_normal((n, n, ns)) + 1j * rng.standard_normal((n, n, ns)))
    x, y = t(np.linspace(1.0, 2.0, n)), t(np.linspace(-3.0, -1.0, n))
    nrec = nsteps // nout
    s = torch.cuda.Stream(DEV)

    def run(psi, rdm, mom):
        _lib.check(lib.qd_spo2_run_observed(psi.data_ptr(), 1, U.data_ptr(), K.data_ptr(), None, n, n, ns, nsteps, nout,
                                            None, None, x.data_ptr(), y.data_ptr(), 0.01, rdm.data_ptr(),
                                            mom.data_ptr(), s.cuda_stream), "qd_spo2_run_observed")

    def outputs():
        return (torch.zeros((nrec, ns, ns), dtype=torch.complex128, device=DEV),
                torch.zeros((nrec, 2, ns), dtype=torch.float64, device=DEV))
    ref = psi0.clone()
    ref_rdm, ref_mom = outputs()
    with torch.cuda.stream(s):
        run(ref, ref_rdm, ref_mom)
    torch.cuda.synchronize()
    assert float(ref_rdm.abs().sum()) > 0
    psi = psi0.clone()
    rdm, mom = outputs()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        run(psi, rdm, mom)
    for k in range(3):
        other = psi0.clone()   # an uncaptured call between the replays
        o_rdm, o_mom = outputs()
        with torch.cuda.stream(s):
            run(other, o_rdm, o_mom)
        psi.copy_(psi0)
        rdm.zero_()
        mom.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(psi, ref), k
        assert torch.equal(rdm, ref_rdm) and torch.equal(mom, ref_mom), k
        assert torch.equal(other, ref) and torch.equal(o_rdm, ref_rdm)
