"""Curvilinear (G-matrix) wavepacket propagation on coupled surfaces on the GPU: qd_wp2_gmat_ms_apply /
qd_wp2_gmat_ms_rk4 and their Python front (pyqed_amd.wpd hpsi, curvilinear_run with a potential [nx, ny, ns, ns];
SPO2(coords='curvilinear', G=G)) against the numpy restatement of tests/gmat_ms_models.py (fft2 form per state, an
einsum for the potential, classical RK4: not the arithmetic under test) and the reference's single-surface outputs in
tests/golden/gmat2d.npz.

Inputs are normalised white noise per state and the bounds are those of test_gmat_gpu.py, in units of
fft_cases.tol(n) = 64 2^-53 (1 + log2 n), n the longer axis: 5 for one application, nt * 20 for a run.  The sum
sum_b V_ab y_b adds ns - 1 roundings of 2^-53 to the point-wise product that bound already counts as one unit of tol,
far below that unit, so the margin is unchanged.

The states are planes on the device, so a call on B members of ns states takes the column tile of B ns single-surface
members (test_gmat_gpu.py); every case asserts wp2_gmat_ms, the path and the tile it must note and the ones it must
not."""
import numpy as np
import pytest
import torch

from conftest import load_golden, relerr, took
import fft_cases as fc
import gmat_models as gm
import gmat_ms_models as gms
from test_gmat_gpu import _expect, _wide_batch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)

CASES = [(nx, ny, ns) for nx, ny in [(16, 16), (32, 16), (16, 32)] for ns in (1, 2, 3)] \
    + [(256, 16, 3)]                        # 16 row workgroups per plane: an update of y in place would show here
CASES += [(16, 1024, 2), (1024, 16, 2)]
CASES += [(24, 20, 2), (67, 45, 2), (1, 8, 2), (8, 1, 2), (12, 10, 3)]   # any grid


def _took(nx, ny, members):
    """The calls since the last check noted wp2_gmat_ms and exactly the path and tile `members` planes must take."""
    got = took("")[1]
    want, never = _expect(nx, ny, members)
    return all(w in got for w in want + ["wp2_gmat_ms"]) and not any(n in got for n in never), got


def _noise(nx, ny, ns, seed, batch=None):
    """White noise [nx, ny, ns] with every state normalised, or a batch [batch, nx, ny, ns] of different members."""
    w = fc.noise(np.random.default_rng(seed), (batch or 1, nx, ny, ns))
    w /= np.linalg.norm(w, axis=(1, 2), keepdims=True)
    return w if batch else w[0]


def _run_ratios(psi, snap, ref, bound):
    """err / bound of the final state and the two snapshots of an nt = 4, nout = 2 run against run_ms_ref's states."""
    return [relerr(psi, ref[3]) / bound, relerr(snap[0], ref[1]) / bound, relerr(snap[1], ref[3]) / bound]


@pytest.mark.parametrize("nx,ny,ns", CASES)
def test_operator_and_run_on_white_noise(nx, ny, ns):
    from pyqed_amd.wpd import curvilinear_run, hpsi
    m = gms.model_ms(nx, ny, ns)
    nt, nout = 4, 2
    w = _noise(nx, ny, ns, 400 + nx + 3 * ny + 7 * ns)
    took("")
    got_h = hpsi(w, m["kx"], m["ky"], m["V"], m["G"])
    hit, paths = _took(nx, ny, ns)
    assert hit, paths
    assert isinstance(got_h, np.ndarray) and got_h.shape == (nx, ny, ns)
    psi, snap = curvilinear_run(m["x"], m["y"], w, m["V"], m["G"], m["dt"], nt, nout)
    hit, paths = _took(nx, ny, ns)
    assert hit, paths
    assert tuple(psi.shape) == (1, nx, ny, ns) and tuple(snap.shape) == (1, nt // nout, nx, ny, ns)
    assert psi.is_cuda and snap.is_cuda and psi.is_contiguous() and snap.is_contiguous()
    n = max(nx, ny)
    r_h = relerr(got_h, gms.hpsi_ms_ref(w, m["kx"], m["ky"], m["V"], m["G"])) / (5.0 * fc.tol(n))
    ref = gms.run_ms_ref(w, m["dt"], nt, m["kx"], m["ky"], m["V"], m["G"])
    rs = _run_ratios(psi.cpu().numpy()[0], snap.cpu().numpy()[0], ref, nt * 20.0 * fc.tol(n))
    print(f"gmat ms {nx}x{ny} ns={ns}: err/bound hpsi {r_h:.3e} run final {rs[0]:.3e} snapshots {rs[1]:.3e} {rs[2]:.3e}")
    assert fc.within(r_h, *rs), (r_h, rs)


def test_wide_column_tile_counts_the_planes():
    """512 x 16, ns = 2 with the smallest batch whose B ns planes take the wide column tile (half the single-surface
    batch): operator and run of the first and last member within the white-noise bounds."""
    from pyqed_amd.wpd import curvilinear_run, hpsi
    nx, ny, ns, nt, nout = 512, 16, 2, 4, 2
    B = -(-_wide_batch(ny) // ns)
    m = gms.model_ms(nx, ny, ns)
    w = _noise(nx, ny, ns, 500, batch=B)
    ws = torch.from_numpy(w).to(DEV)
    took("")
    H = hpsi(ws, m["kx"], m["ky"], m["V"], m["G"])
    hit, paths = _took(nx, ny, B * ns)
    assert hit and "wp2_gmat_col_wide" in paths, paths
    psi, snap = curvilinear_run(m["x"], m["y"], ws, m["V"], m["G"], m["dt"], nt, nout)
    hit, paths = _took(nx, ny, B * ns)
    assert hit and "wp2_gmat_col_wide" in paths, paths
    assert H.is_cuda and tuple(H.shape) == (B, nx, ny, ns) and tuple(snap.shape) == (B, nt // nout, nx, ny, ns)
    assert torch.equal(ws, torch.from_numpy(w).to(DEV))   # the input batch is not modified
    for b in (0, B - 1):
        r_h = relerr(H[b].cpu().numpy(), gms.hpsi_ms_ref(w[b], m["kx"], m["ky"], m["V"], m["G"])) / (5.0 * fc.tol(nx))
        ref = gms.run_ms_ref(w[b], m["dt"], nt, m["kx"], m["ky"], m["V"], m["G"])
        rs = _run_ratios(psi[b].cpu().numpy(), snap[b].cpu().numpy(), ref, nt * 20.0 * fc.tol(nx))
        print(f"gmat ms wide tile {nx}x{ny} ns={ns} B={B} member {b}: err/bound hpsi {r_h:.3e} run {rs[0]:.3e} "
              f"snapshots {rs[1]:.3e} {rs[2]:.3e}")
        assert fc.within(r_h, *rs), (b, r_h, rs)
    assert not torch.equal(psi[0], psi[B - 1])


@pytest.mark.parametrize("nx,ny", [(32, 16), (24, 20)])
def test_one_state_is_the_single_surface_call_bit_for_bit(nx, ny):
    from pyqed_amd.wpd import curvilinear_run, hpsi
    m = gm.model(nx, ny)
    w = _noise(nx, ny, 1, 11, batch=2)
    took("")
    p1, s1 = curvilinear_run(m["x"], m["y"], w[..., 0], m["v"], m["G"], m["dt"], 4, 2)
    assert "wp2_gmat_ms" not in took("")[1]
    pm, sm = curvilinear_run(m["x"], m["y"], w, m["v"][..., None, None], m["G"], m["dt"], 4, 2)
    hit, paths = _took(nx, ny, 2)
    assert hit, paths
    assert tuple(pm.shape) == (2, nx, ny, 1) and tuple(sm.shape) == (2, 2, nx, ny, 1)
    assert np.array_equal(pm.cpu().numpy()[..., 0], p1.cpu().numpy())
    assert np.array_equal(sm.cpu().numpy()[..., 0], s1.cpu().numpy())
    assert np.array_equal(hpsi(w, m["kx"], m["ky"], m["v"][..., None, None], m["G"])[..., 0],
                          hpsi(w[..., 0], m["kx"], m["ky"], m["v"], m["G"]))


def test_uncoupled_states_follow_their_own_surfaces():
    """Block-diagonal V, ns = 3: every state is its single-surface run within the run bound."""
    from pyqed_amd.wpd import curvilinear_run
    nx, ny, ns, nt = 32, 16, 3, 4
    m = gms.model_ms(nx, ny, ns)
    V = gms.block_diagonal(m["V"])
    w = _noise(nx, ny, ns, 21)
    psi, snap = curvilinear_run(m["x"], m["y"], w, V, m["G"], m["dt"], nt, 2)
    psi, snap = psi.cpu().numpy()[0], snap.cpu().numpy()[0]
    bound = nt * 20.0 * fc.tol(nx)
    for a in range(ns):
        p1, s1 = curvilinear_run(m["x"], m["y"], w[..., a], V[..., a, a], m["G"], m["dt"], nt, 2)
        p1, s1 = p1.cpu().numpy()[0], s1.cpu().numpy()[0]
        rs = [relerr(psi[..., a], p1) / bound, relerr(snap[..., a], s1) / bound]
        same = np.array_equal(psi[..., a], p1) and np.array_equal(snap[..., a], s1)
        print(f"gmat ms uncoupled state {a}: err/bound final {rs[0]:.3e} snapshots {rs[1]:.3e} bit-equal {same}")
        assert fc.within(*rs), (a, rs)


def test_coupling_moves_population():
    """From psi0 on state 0 alone, state 1 is populated after 4 steps, by the restatement's amount (relative 1e-12;
    the population's own rounding is a few tol(32) ~ 4e-14 relative, as every error of psi_1 is relative to psi_1 or
    to V_10 psi_0, its source)."""
    from pyqed_amd.wpd import curvilinear_run
    nx, ny, ns, nt = 32, 16, 3, 4
    m = gms.model_ms(nx, ny, ns)
    w = _noise(nx, ny, ns, 22)
    w[..., 1:] = 0.0
    psi, _ = curvilinear_run(m["x"], m["y"], w, m["V"], m["G"], m["dt"], nt, 2)
    psi = psi.cpu().numpy()[0]
    ref = gms.run_ms_ref(w, m["dt"], nt, m["kx"], m["ky"], m["V"], m["G"])[-1]
    pop, pop_ref = np.sum(np.abs(psi) ** 2, axis=(0, 1)), np.sum(np.abs(ref) ** 2, axis=(0, 1))
    print(f"gmat ms coupling: populations {pop} restatement {pop_ref} rel diff {np.abs(pop - pop_ref) / pop_ref}")
    assert pop[1] > 0.0 and pop_ref[1] > 1e-12
    assert np.all(np.abs(pop - pop_ref) <= 1e-12 * pop_ref)
    off, _ = curvilinear_run(m["x"], m["y"], w, gms.block_diagonal(m["V"]), m["G"], m["dt"], nt, 2)
    assert np.all(off.cpu().numpy()[0][..., 1:] == 0.0)


def test_runs_repeat_and_members_equal_their_single_calls():
    from pyqed_amd.wpd import curvilinear_run
    nx, ny, ns, B = 256, 16, 3, 4
    m = gms.model_ms(nx, ny, ns)
    ws = torch.from_numpy(_noise(nx, ny, ns, 23, batch=B)).to(DEV)
    args = (m["V"], m["G"], m["dt"], 4, 2)
    psi, snap = curvilinear_run(m["x"], m["y"], ws, *args)
    again, snap2 = curvilinear_run(m["x"], m["y"], ws, *args)
    assert torch.equal(psi, again) and torch.equal(snap, snap2)
    for b in range(B):
        p1, s1 = curvilinear_run(m["x"], m["y"], ws[b], *args)
        assert torch.equal(psi[b], p1[0]) and torch.equal(snap[b], s1[0]), b
    assert not torch.equal(psi[0], psi[1])


@pytest.mark.parametrize("tag", ["a", "b", "c"])
def test_spo2_one_state_reproduces_the_reference_fixture(tag):
    """The reference's own curvilinear outputs through SPO2(nstates=1, coords='curvilinear'); case c has the absorbing
    potential, so this is the complex-V path."""
    from pyqed_amd.wpd import SPO2
    g = load_golden("gmat2d")
    c = {k[2:]: v for k, v in g.items() if k.startswith(tag + "_")}
    psi0 = c["psi0"][..., None].copy()
    nt = int(c["nt"])
    sol = SPO2(c["x"], c["y"], nstates=1, coords="curvilinear", G=c["G"])
    sol.set_dpes(c["v"][..., None, None])
    took("")
    r = sol.run(psi0, dt=float(c["dt"]), nt=nt, nout=nt)
    hit, paths = _took(*c["psi0"].shape, 1)
    assert hit, paths
    assert len(r.psilist) == 2 and r.psi.shape == psi0.shape
    assert relerr(r.psi[..., 0], c["psi"]) < 1e-11 and relerr(r.psilist[-1][..., 0], c["psi"]) < 1e-11
    assert np.array_equal(psi0[..., 0], c["psi0"]) and r.psilist[0] is psi0


def _observe_ref(states, x, y, basis=None):
    """rdm [N, ns, ns], xAve, yAve [N] of states [N, nx, ny, ns]: the einsum of test_spo_observe_gpu.py's comparator."""
    w = (x[1] - x[0]) * (y[1] - y[0])
    chi = states if basis is None else np.einsum("ijab,kijb->kija", basis, states)
    rdm = w * np.einsum("kija,kijb->kab", chi.conj(), chi)
    dens = np.abs(chi) ** 2
    return rdm, w * np.einsum("kija,i->k", dens, x), w * np.einsum("kija,j->k", dens, y)


def test_spo2_curvilinear_surface():
    """SPO2(coords='curvilinear').run / run_batch at 32 x 16, ns = 2, nt = 6, nout = 2.  Observables against the numpy
    einsum on the recorded states with test_spo_observe_gpu.py's 1e-13; white noise has <x> ~ 0, a cancellation, so the
    mean positions are bounded against sum |x| |psi|^2 w <= max |x| tr rdm, as that file does for a symmetric <y>."""
    from pyqed_amd.wpd import SPO2
    nx, ny, ns, nt, nout = 32, 16, 2, 6, 2
    m = gms.model_ms(nx, ny, ns)
    x, y = m["x"], m["y"]
    w = _noise(nx, ny, ns, 31, batch=2)
    psi0, keep = w[0], w[0].copy()
    sol = SPO2(x, y, nstates=ns, coords="curvilinear", G=m["G"])
    sol.set_dpes(m["V"])
    took("")
    r = sol.run(psi0, dt=m["dt"], nt=nt, nout=nout)
    hit, paths = _took(nx, ny, ns)
    assert hit, paths
    ref = gms.run_ms_ref(psi0, m["dt"], nt, m["kx"], m["ky"], m["V"], m["G"])
    bound = nt * 20.0 * fc.tol(nx)
    assert len(r.psilist) == 4 and r.psilist[0] is psi0 and np.array_equal(psi0, keep)
    rs = [relerr(r.psilist[k], ref[2 * k - 1]) / bound for k in (1, 2, 3)] + [relerr(r.psi, ref[-1]) / bound]
    print(f"gmat ms SPO2 run: err/bound snapshots {rs[0]:.3e} {rs[1]:.3e} {rs[2]:.3e} final {rs[3]:.3e}")
    assert all(p.shape == (nx, ny, ns) for p in r.psilist) and fc.within(*rs), rs
    assert np.array_equal(r.psi, r.psilist[-1])
    assert sol.exp_K is None and sol.exp_V is None

    r0 = sol.run(psi0, dt=m["dt"], nt=nt, nout=nout, return_states=False)
    assert len(r0.psilist) == 1 and r0.psilist[0] is psi0 and np.array_equal(r0.psi, r.psi)

    states = np.array(r.psilist)
    for observe, basis in (("diabatic", None), ("adiabatic", "d2a")):
        ro = sol.run(psi0, dt=m["dt"], nt=nt, nout=nout, observe=observe)
        assert all(np.array_equal(a, b) for a, b in zip(ro.psilist, r.psilist)) and np.array_equal(ro.psi, r.psi)
        rdm, xa, ya = _observe_ref(states, x, y, None if basis is None else sol.d2a)
        pop = np.einsum("kaa->ka", rdm).real
        assert ro.population.shape == (4, ns) and ro.rdm.shape == (4, ns, ns)
        e = [relerr(ro.rdm, rdm), relerr(ro.population, pop),
             np.abs(ro.xAve[0] - xa).max() / (np.abs(x).max() * pop.sum(axis=1).max()),
             np.abs(ro.xAve[1] - ya).max() / (np.abs(y).max() * pop.sum(axis=1).max())]
        print(f"gmat ms SPO2 observe={observe}: rdm {e[0]:.3e} population {e[1]:.3e} xAve {e[2]:.3e} yAve {e[3]:.3e}")
        assert max(e) < 1e-13, e
        rn = sol.run(psi0, dt=m["dt"], nt=nt, nout=nout, observe=observe, return_states=False)
        assert len(rn.psilist) == 1 and np.array_equal(rn.population, ro.population) and np.array_equal(rn.rdm, ro.rdm)
        assert np.array_equal(rn.get_population(), ro.population) and np.array_equal(rn.psi, r.psi)
        if basis is None:
            assert relerr(sol.population(r.psilist), pop) < 1e-13
            assert relerr(np.array(sol.rdm_el(r.psilist)), rdm) < 1e-13

    took("")
    pb, sb = sol.run_batch(w, dt=m["dt"], nt=nt, nout=nout)
    hit, paths = _took(nx, ny, 2 * ns)
    assert hit, paths
    assert tuple(pb.shape) == (2, nx, ny, ns) and tuple(sb.shape) == (2, 3, nx, ny, ns)
    assert np.array_equal(pb[0].cpu().numpy(), r.psi) and np.array_equal(sb[0].cpu().numpy(), states[1:])
    r1 = sol.run(w[1], dt=m["dt"], nt=nt, nout=nout)
    assert np.array_equal(pb[1].cpu().numpy(), r1.psi) and np.array_equal(sb[1].cpu().numpy(), np.array(r1.psilist[1:]))
    ro = sol.run(psi0, dt=m["dt"], nt=nt, nout=nout, observe="diabatic")
    pb2, none, obs = sol.run_batch(w, dt=m["dt"], nt=nt, nout=nout, observe="diabatic", keep_states=False)
    assert none is None and torch.equal(pb2, pb)
    assert np.array_equal(obs["rdm"][0].cpu().numpy(), ro.rdm[1:])
    assert np.array_equal(obs["population"][0].cpu().numpy(), ro.population[1:])
    assert tuple(obs["mom"].shape) == (2, 3, 2, ns)


def test_spo2_curvilinear_absorbing_potential_propagates():
    """abc=True: set_DPES's complex diagonal -i eta (X - 9)^2 runs, and the norm falls from snapshot to snapshot."""
    from pyqed_amd.wpd import SPO2
    nx, ny, ns, nt, nout = 32, 16, 2, 6, 2
    m = gms.model_ms(nx, ny, ns)
    X, Y = np.meshgrid(m["x"], m["y"], indexing="ij")
    sol = SPO2(m["x"], m["y"], nstates=ns, coords="curvilinear", G=m["G"], abc=True)
    V = sol.set_DPES([m["v"], 0.8 * m["v"] + 0.3], [[[0, 1], 0.1 * np.exp(-X ** 2 - Y ** 2)]], eta=0.05)
    assert np.iscomplexobj(V) and np.all(V[..., 0, 0].imag < 0)
    dt = 1.0 / (m["lam"] + np.abs(V[..., 0, 0]).max())
    psi0 = _noise(nx, ny, ns, 32)
    r = sol.run(psi0, dt=dt, nt=nt, nout=nout, observe="diabatic")
    norms = [np.linalg.norm(p) for p in r.psilist]
    print(f"gmat ms SPO2 abc: norms {norms}")
    assert len(norms) == 4 and all(b < a for a, b in zip(norms, norms[1:])) and norms[-1] > 0
    ref = gms.run_ms_ref(psi0, dt, nt, m["kx"], m["ky"], V, m["G"])
    assert relerr(r.psi, ref[-1]) <= nt * 20.0 * fc.tol(nx)
    assert np.all(np.diff(r.population.sum(axis=1)) < 0)


def test_ms_rk4_call_replays_from_a_graph():
    """qd_wp2_gmat_ms_rk4 (32 x 32, ns = 2, B = 2, 4 steps) captured on one side stream, no parallel branches, and
    replayed twice from a restored input: both replays equal the eager call bit for bit."""
    from pyqed_amd import _lib
    _lib.ensure_device(DEV)
    lib = _lib.load()
    nx, ny, ns, B = 32, 32, 2, 2
    m = gms.model_ms(nx, ny, ns)
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(DEV)
    G, kx, ky = t(m["G"], float), t(m["kx"], float), t(m["ky"], float)
    V = t(m["V"].transpose(2, 3, 0, 1), complex)                               # [ns][ns][nx][ny]
    psi0 = t(_noise(nx, ny, ns, 9, batch=B).transpose(0, 3, 1, 2), complex)    # [B][ns][nx][ny]
    s = torch.cuda.Stream(DEV)

    def run(x, sn):
        _lib.check(lib.qd_wp2_gmat_ms_rk4(x.data_ptr(), B, ns, G.data_ptr(), V.data_ptr(), kx.data_ptr(), ky.data_ptr(),
                                          nx, ny, float(m["dt"]), 4, 2, sn.data_ptr(), s.cuda_stream),
                   "qd_wp2_gmat_ms_rk4")
    ref, ref_sn = psi0.clone(), torch.zeros((B, 2, ns, nx, ny), dtype=torch.complex128, device=DEV)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        run(ref, ref_sn)
    torch.cuda.synchronize()
    x, sn = psi0.clone(), torch.zeros_like(ref_sn)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    took("")
    with torch.cuda.graph(g, stream=s):
        run(x, sn)
    hit, paths = _took(nx, ny, B * ns)
    assert hit, paths
    for _ in range(2):
        x.copy_(psi0)
        sn.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(x, ref) and torch.equal(sn, ref_sn)
    assert not torch.equal(ref, psi0)
    # the eager call is the Python front's numbers: plane layout in, state-innermost layout out
    from pyqed_amd.wpd import curvilinear_run
    pf, sf = curvilinear_run(m["x"], m["y"], psi0.permute(0, 2, 3, 1), m["V"], m["G"], m["dt"], 4, 2)
    assert torch.equal(pf, ref.permute(0, 2, 3, 1)) and torch.equal(sf, ref_sn.permute(0, 1, 3, 4, 2))
