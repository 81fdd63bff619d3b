"""Three-dimensional curvilinear (3 x 3 G-matrix) wavepacket propagation on the GPU: the four qd_wp3_gmat_* entry
points and their Python front (pyqed_amd.wpd KEO3, hpsi3, curvilinear_run3, SPO3(coords='curvilinear')) against the
numpy restatement of tests/gmat3_models.py (fftn form, an einsum for the metric, classical RK4: not the arithmetic
under test), against closed forms, and against the reference's own two-dimensional outputs in tests/golden/gmat2d.npz
carried through the 3-D entry points.

Inputs are white noise as in test_gmat_gpu.py, normalised per member.  Bounds, in units of fft_cases.tol(n), n the
longest axis, by that suite's rule:
  operator: 6 = four chained transforms on the longest path plus two for the three-term point-wise sums;
  run:      nt * 24 = four stages a step, each at most one application's error since dt ||H|| <= 1.
A numpy emulation of the kernels' arithmetic sits near 2e-3 of the operator bound and 1e-4 of the run bound
(test_gmat3_host.py), so the bounds are caps a correct kernel does not approach.  Every test asserts the path names
its calls noted: wp3_gmat_pow2 (every axis a power of two in [16, 256]) or wp3_gmat_any, and wp3_gmat_ms for the
coupled entry points."""
import numpy as np
import pytest
import torch
from scipy.fftpack import fftfreq

from conftest import load_golden, relerr, took
import fft_cases as fc
import gmat3_models as g3

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)

FUSED_SHAPES = [(16, 16, 16), (16, 32, 64), (64, 16, 32), (32, 64, 16), (128, 16, 16), (16, 128, 16), (16, 16, 128),
                (256, 16, 16), (16, 256, 16), (16, 16, 256)]
ANY_SHAPES = [(24, 20, 18), (12, 10, 7), (67, 5, 3), (3, 5, 2), (1, 8, 8), (8, 1, 8), (8, 8, 1), (32, 20, 16),
              (16, 16, 8), (512, 16, 16), (5125, 2, 2), (2, 5125, 2), (2, 2, 5125)]   # the last three: four-step order
RUN_SHAPES = [(16, 16, 16), (16, 32, 64), (64, 16, 32), (256, 16, 16), (16, 16, 256), (24, 20, 18), (67, 5, 3),
              (1, 8, 8)]


def _fused(shape):
    return all(16 <= n <= 256 and n & (n - 1) == 0 for n in shape)


def _took(shape, ms):
    """The calls since the last check noted exactly the path this shape must take, and wp3_gmat_ms iff coupled."""
    got = took("")[1]
    want, never = ("wp3_gmat_pow2", "wp3_gmat_any") if _fused(shape) else ("wp3_gmat_any", "wp3_gmat_pow2")
    return want in got and never not in got and ("wp3_gmat_ms" in got) == ms, got


def _noise(shape, seed, ns=0, batch=None):
    """White noise [nx, ny, nz(, ns)] with every state of every member normalised, or a batch of different members."""
    w = fc.noise(np.random.default_rng(seed), (batch or 1,) + tuple(shape) + ((ns,) if ns else ()))
    w /= np.sqrt(np.sum(np.abs(w) ** 2, axis=(1, 2, 3), keepdims=True))
    return w if batch else w[0]


def _seed(shape, ns=0):
    return 100 + shape[0] + 3 * shape[1] + 7 * shape[2] + 11 * ns


def _run_ratios(psi, snap, ref, bound):
    """err / bound of the final state and the two snapshots of an nt = 4, nout = 2 run against run_ref's states."""
    return [relerr(psi, ref[3]) / bound, relerr(snap[0], ref[1]) / bound, relerr(snap[1], ref[3]) / bound]


@pytest.mark.parametrize("shape", FUSED_SHAPES + ANY_SHAPES, ids=str)
def test_operator_on_white_noise(shape):
    from pyqed_amd.wpd import KEO3, hpsi3
    m = g3.model3(*shape)
    w = _noise(shape, _seed(shape))
    took("")
    got_h = hpsi3(w, *m["ks"], m["v"], m["G"])
    hit, paths = _took(shape, False)
    assert hit, paths
    got_k = KEO3(w, *m["ks"], m["G"])
    hit, paths = _took(shape, False)
    assert hit, paths
    assert isinstance(got_h, np.ndarray) and got_h.shape == shape and got_k.shape == shape
    bound = 6.0 * fc.tol(max(shape))
    r_h = relerr(got_h, g3.hpsi3_ref(w, m["ks"], m["v"], m["G"])) / bound
    r_k = relerr(got_k, g3.keo3_ref(w, m["ks"], m["G"])) / bound
    print(f"gmat3 operator {shape}: hpsi3 err/bound {r_h:.3e}  KEO3 err/bound {r_k:.3e}")
    assert fc.within(r_h, r_k), (r_h, r_k)


@pytest.mark.parametrize("shape", RUN_SHAPES, ids=str)
def test_runs_on_white_noise(shape):
    from pyqed_amd.wpd import curvilinear_run3
    m = g3.model3(*shape)
    nt, nout = 4, 2
    w = _noise(shape, 100 + _seed(shape))
    ref = g3.run_ref(w, m["dt"], nt, m["ks"], m["v"], m["G"])
    took("")
    psi, snap = curvilinear_run3(m["x"], m["y"], m["z"], w, m["v"], m["G"], m["dt"], nt, nout)
    hit, paths = _took(shape, False)
    assert hit, paths
    assert tuple(psi.shape) == (1,) + shape and tuple(snap.shape) == (1, nt // nout) + shape
    assert psi.is_cuda and snap.is_cuda
    rs = _run_ratios(psi.cpu().numpy()[0], snap.cpu().numpy()[0], ref, nt * 24.0 * fc.tol(max(shape)))
    print(f"gmat3 run {shape}: err/bound final {rs[0]:.3e} snapshots {rs[1]:.3e} {rs[2]:.3e}")
    assert fc.within(*rs), rs


def _lift(c, nz):
    """A 2-D fixture case carried to 3-D: psi0, v (and the noise) replicated along z, and a z-independent metric whose
    upper 2 x 2 block is the fixture's G; the five z entries are arbitrary non-zero functions of (x, y).  D_z of a
    line that is constant along z is zero, so every z slice of the 3-D result is the 2-D result."""
    nx, ny = c["psi0"].shape
    X, Y = np.meshgrid(c["x"], c["y"], indexing="ij")
    G = np.empty((nx, ny, nz, 3, 3))
    G[..., :2, :2] = c["G"][:, :, None]
    for (r, s), f in {(0, 2): 0.3 + 0.1 * np.cos(X), (2, 0): -0.2 + 0.05 * np.sin(Y), (1, 2): 0.25 * np.cos(X + Y) + 0.4,
                      (2, 1): 0.1 + 0.05 * X * Y / 30.0, (2, 2): 1.1 + 0.2 * np.sin(X) * np.cos(Y)}.items():
        assert np.all(f != 0)
        G[..., r, s] = f[:, :, None]
    z = 0.25 * np.arange(nz)
    rep = lambda a: np.ascontiguousarray(np.broadcast_to(a[:, :, None], (nx, ny, nz)))
    ks = [2.0 * np.pi * fftfreq(n, a[1] - a[0]) for n, a in ((nx, c["x"]), (ny, c["y"]), (nz, z))]
    return z, G, rep, ks


@pytest.mark.parametrize("tag,nz", [("a", 3), ("b", 16), ("c", 16)])
def test_reference_fixture_through_the_3d_entry_points(tag, nz):
    """The reference's own 2-D numbers: every z slice equals b_psi / c_psi (fused path, c with a complex potential)
    or a_hpsi, a_keo and a_psi (any-grid path) within the 2-D suite's bounds, 5 tol for the operator and nt * 20 tol
    for the run."""
    from pyqed_amd.wpd import KEO3, curvilinear_run3, hpsi3
    g = load_golden("gmat2d")
    c = {k[2:]: v for k, v in g.items() if k.startswith(tag + "_")}
    nx, ny = c["psi0"].shape
    shape, nt = (nx, ny, nz), int(c["nt"])
    z, G, rep, ks = _lift(c, nz)
    t = fc.tol(max(shape))
    took("")
    psi, _ = curvilinear_run3(c["x"], c["y"], z, rep(c["psi0"]), rep(c["v"]), G, float(c["dt"]), nt, nt)
    hit, paths = _took(shape, False)
    assert hit and _fused(shape) == (tag != "a"), paths
    psi = psi.cpu().numpy()[0]
    rs = [relerr(psi[:, :, k], c["psi"]) / (nt * 20.0 * t) for k in range(nz)]
    assert ("noise" in c) == (tag == "a"), sorted(c)   # fixture a carries the operator's reference numbers
    if tag == "a":
        H = hpsi3(rep(c["noise"]), *ks, rep(c["v"]), G)
        K = KEO3(rep(c["noise"]), *ks, G)
        hit, paths = _took(shape, False)
        assert hit, paths
        rs += [relerr(H[:, :, k], c["hpsi"]) / (5.0 * t) for k in range(nz)]
        rs += [relerr(K[:, :, k], c["keo"]) / (5.0 * t) for k in range(nz)]
    print(f"gmat3 fixture {tag} {shape} nt={nt}: worst err/bound {max(rs):.3e}")
    assert fc.within(*rs), rs


@pytest.mark.parametrize("shape", [(16, 32, 16), (24, 20, 18)], ids=str)
def test_constant_metric_is_the_taylor_symbol(shape):
    from pyqed_amd.wpd import curvilinear_run3
    m = g3.model3(*shape)
    G0 = np.array([[1.0, 0.2, -0.1], [0.2, 0.8, 0.15], [-0.1, 0.15, 0.9]])
    G = np.broadcast_to(G0, shape + (3, 3)).copy()
    nt = 4
    w = _noise(shape, 300 + _seed(shape))
    took("")
    psi, snap = curvilinear_run3(m["x"], m["y"], m["z"], w, None, G, m["dt"], nt, 2)
    hit, paths = _took(shape, False)
    assert hit, paths
    bound = nt * 24.0 * fc.tol(max(shape))
    rs = [relerr(psi.cpu().numpy()[0], g3.taylor_run(w, m["dt"], nt, m["ks"], G0)) / bound,
          relerr(snap.cpu().numpy()[0, 0], g3.taylor_run(w, m["dt"], 2, m["ks"], G0)) / bound]
    print(f"gmat3 constant metric {shape}: err/bound final {rs[0]:.3e} snapshot {rs[1]:.3e}")
    assert fc.within(*rs), rs


@pytest.mark.parametrize("shape", [(16, 32, 16), (12, 10, 7)], ids=str)
@pytest.mark.parametrize("ns", [2, 3])
def test_coupled_operator_and_run_on_white_noise(shape, ns):
    from pyqed_amd.wpd import curvilinear_run3, hpsi3
    m = g3.model3(*shape, ns=ns)
    nt, nout = 4, 2
    w = _noise(shape, _seed(shape, ns), ns=ns)
    took("")
    got_h = hpsi3(w, *m["ks"], m["V"], m["G"])
    hit, paths = _took(shape, True)
    assert hit, paths
    psi, snap = curvilinear_run3(m["x"], m["y"], m["z"], w, m["V"], m["G"], m["dt"], nt, nout)
    hit, paths = _took(shape, True)
    assert hit, paths
    assert got_h.shape == shape + (ns,) and tuple(psi.shape) == (1,) + shape + (ns,)
    assert tuple(snap.shape) == (1, nt // nout) + shape + (ns,) and psi.is_contiguous() and snap.is_contiguous()
    t = fc.tol(max(shape))
    ref_h = g3.hpsi3_ref(w, m["ks"], m["V"], m["G"])
    ref = g3.run_ref(w, m["dt"], nt, m["ks"], m["V"], m["G"])
    psi, snap = psi.cpu().numpy()[0], snap.cpu().numpy()[0]
    rs = []
    for a in range(ns):   # per state
        rs.append(relerr(got_h[..., a], ref_h[..., a]) / (6.0 * t))
        rs += _run_ratios(psi[..., a], snap[..., a], ref[..., a], nt * 24.0 * t)
    print(f"gmat3 ms {shape} ns={ns}: worst err/bound per state {max(rs):.3e}")
    assert fc.within(*rs), rs


@pytest.mark.parametrize("shape", [(32, 16, 16), (24, 20, 18)], ids=str)
def test_one_state_is_the_single_surface_call_bit_for_bit(shape):
    from pyqed_amd.wpd import curvilinear_run3, hpsi3
    m = g3.model3(*shape)
    w = _noise(shape, 11, ns=1, batch=2)
    axes = (m["x"], m["y"], m["z"])
    took("")
    p1, s1 = curvilinear_run3(*axes, w[..., 0], m["v"], m["G"], m["dt"], 4, 2)
    hit, paths = _took(shape, False)
    assert hit, paths
    pm, sm = curvilinear_run3(*axes, w, m["V"], m["G"], m["dt"], 4, 2)
    hit, paths = _took(shape, True)
    assert hit, paths
    assert tuple(pm.shape) == (2,) + shape + (1,) and tuple(sm.shape) == (2, 2) + shape + (1,)
    assert np.array_equal(pm.cpu().numpy()[..., 0], p1.cpu().numpy())
    assert np.array_equal(sm.cpu().numpy()[..., 0], s1.cpu().numpy())
    assert np.array_equal(hpsi3(w, *m["ks"], m["V"], m["G"])[..., 0], hpsi3(w[..., 0], *m["ks"], m["v"], m["G"]))


def test_uncoupled_states_follow_their_own_surfaces():
    """Block-diagonal V, ns = 2: every state is its single-surface run within the run bound."""
    from pyqed_amd.wpd import curvilinear_run3
    shape, ns, nt = (16, 32, 16), 2, 4
    m = g3.model3(*shape, ns=ns)
    V = g3.block_diagonal(m["V"])
    assert relerr(V[..., 1, 1], V[..., 0, 0]) > 1e-2   # different surfaces
    axes = (m["x"], m["y"], m["z"])
    w = _noise(shape, 21, ns=ns)
    took("")
    psi, snap = curvilinear_run3(*axes, w, V, m["G"], m["dt"], nt, 2)
    hit, paths = _took(shape, True)
    assert hit, paths
    psi, snap = psi.cpu().numpy()[0], snap.cpu().numpy()[0]
    bound = nt * 24.0 * fc.tol(max(shape))
    for a in range(ns):
        p1, s1 = curvilinear_run3(*axes, w[..., a], V[..., a, a], m["G"], m["dt"], nt, 2)
        hit, paths = _took(shape, False)
        assert hit, paths
        rs = [relerr(psi[..., a], p1.cpu().numpy()[0]) / bound, relerr(snap[..., a], s1.cpu().numpy()[0]) / bound]
        print(f"gmat3 ms uncoupled state {a}: err/bound final {rs[0]:.3e} snapshots {rs[1]:.3e}")
        assert fc.within(*rs), (a, rs)


def test_coupling_moves_population():
    """From psi0 on state 0 alone, state 1 is populated after 4 steps by the restatement's amount and the total norm
    follows the restatement (relative 1e-12, as test_gmat_ms_gpu.py argues); without the coupling it stays empty."""
    from pyqed_amd.wpd import curvilinear_run3
    shape, ns, nt = (16, 32, 16), 2, 4
    m = g3.model3(*shape, ns=ns)
    axes = (m["x"], m["y"], m["z"])
    w = _noise(shape, 22, ns=ns)
    w[..., 1:] = 0.0
    took("")
    psi, _ = curvilinear_run3(*axes, w, m["V"], m["G"], m["dt"], nt, 2)
    hit, paths = _took(shape, True)
    assert hit, paths
    psi = psi.cpu().numpy()[0]
    ref = g3.run_ref(w, m["dt"], nt, m["ks"], m["V"], m["G"])[-1]
    pop, pop_ref = np.sum(np.abs(psi) ** 2, axis=(0, 1, 2)), np.sum(np.abs(ref) ** 2, axis=(0, 1, 2))
    print(f"gmat3 ms coupling: populations {pop} restatement {pop_ref}")
    assert pop[1] > 0.0 and pop_ref[1] > 1e-12
    assert np.all(np.abs(pop - pop_ref) <= 1e-12 * pop_ref) and abs(pop.sum() - pop_ref.sum()) <= 1e-12 * pop_ref.sum()
    off, _ = curvilinear_run3(*axes, w, g3.block_diagonal(m["V"]), m["G"], m["dt"], nt, 2)
    hit, paths = _took(shape, True)
    assert hit, paths
    assert np.all(off.cpu().numpy()[0][..., 1:] == 0.0)


@pytest.mark.parametrize("shape", [(32, 16, 16), (24, 20, 18)], ids=str)
def test_batch_members_equal_their_single_calls_bit_for_bit(shape):
    from pyqed_amd.wpd import curvilinear_run3, hpsi3
    m = g3.model3(*shape)
    axes = (m["x"], m["y"], m["z"])
    w = _noise(shape, 7, batch=3)
    ws = torch.from_numpy(w).to(DEV)
    took("")
    H = hpsi3(ws, *m["ks"], m["v"], m["G"])
    hit, paths = _took(shape, False)
    assert hit, paths
    psi, snap = curvilinear_run3(*axes, ws, m["v"], m["G"], m["dt"], 4, 2)
    hit, paths = _took(shape, False)
    assert hit, paths
    again, snap2 = curvilinear_run3(*axes, ws, m["v"], m["G"], m["dt"], 4, 2)
    hit, paths = _took(shape, False)
    assert hit, paths
    assert torch.equal(psi, again) and torch.equal(snap, snap2)            # a repeated call gives the same bits
    assert torch.equal(H, hpsi3(ws, *m["ks"], m["v"], m["G"]))
    assert torch.equal(ws, torch.from_numpy(w).to(DEV))                    # the input batch is unmodified
    assert H.is_cuda and tuple(H.shape) == (3,) + shape and tuple(snap.shape) == (3, 2) + shape
    for b in range(3):
        took("")
        assert torch.equal(H[b], hpsi3(ws[b], *m["ks"], m["v"], m["G"])), b
        hit, paths = _took(shape, False)
        assert hit, paths
        p1, s1 = curvilinear_run3(*axes, ws[b], m["v"], m["G"], m["dt"], 4, 2)
        hit, paths = _took(shape, False)
        assert hit, paths
        assert torch.equal(psi[b], p1[0]) and torch.equal(snap[b], s1[0]), b
    assert not torch.equal(psi[0], psi[1])


def test_ms_rk4_call_replays_from_a_graph():
    """qd_wp3_gmat_ms_rk4 (16 x 32 x 16, ns = 2, B = 2, 4 steps) captured on one side stream, no parallel branches, and
    replayed twice from a restored input: both replays equal the eager call bit for bit."""
    from pyqed_amd import _lib
    _lib.ensure_device(DEV)
    lib = _lib.load()
    shape, ns, B = (16, 32, 16), 2, 2
    m = g3.model3(*shape, ns=ns)
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(DEV)
    G, ks = t(m["G"], float), [t(k, float) for k in m["ks"]]
    V = t(np.moveaxis(m["V"], (-2, -1), (0, 1)), complex)             # [ns][ns][nx][ny][nz]
    psi0 = t(np.moveaxis(_noise(shape, 9, ns=ns, batch=B), -1, 1), complex)   # [B][ns][nx][ny][nz]
    s = torch.cuda.Stream(DEV)

    def run(x, sn):
        _lib.check(lib.qd_wp3_gmat_ms_rk4(x.data_ptr(), B, ns, G.data_ptr(), V.data_ptr(), *(k.data_ptr() for k in ks),
                                          *shape, float(m["dt"]), 4, 2, sn.data_ptr(), s.cuda_stream),
                   "qd_wp3_gmat_ms_rk4")
    ref, ref_sn = psi0.clone(), torch.zeros((B, 2, ns) + shape, dtype=torch.complex128, device=DEV)
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
    hit, paths = _took(shape, True)
    assert hit, paths
    for _ in range(2):
        x.copy_(psi0)
        sn.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(x, ref) and torch.equal(sn, ref_sn)
    assert not torch.equal(ref, psi0)
    # the eager call is the Python front's numbers: plane layout in, state-innermost layout out
    from pyqed_amd.wpd import curvilinear_run3
    pf, sf = curvilinear_run3(m["x"], m["y"], m["z"], psi0.permute(0, 2, 3, 4, 1), m["V"], m["G"], m["dt"], 4, 2)
    assert torch.equal(pf, ref.permute(0, 2, 3, 4, 1)) and torch.equal(sf, ref_sn.permute(0, 1, 3, 4, 5, 2))


def test_spo3_curvilinear_surface():
    """SPO3(coords='curvilinear').run at 32 x 16 x 16, ns = 2, nt = 6, nout = 2: states against the restatement, the
    observables against numpy sums over the restatement's states with psi0 in row 0.  The observables' own rounding is
    1e-13 (test_spo_observe_gpu.py); the states they are reduced from differ from the restatement's by at most the
    run bound, and |psi|^2 sums carry twice that.  White noise has <x> ~ 0, a cancellation, so the mean positions are
    bounded against max |x| tr rdm."""
    from pyqed_amd.wpd import SPO3
    shape, ns, nt, nout = (32, 16, 16), 2, 6, 2
    m = g3.model3(*shape, ns=ns)
    axes = (m["x"], m["y"], m["z"])
    psi0 = _noise(shape, 31, ns=ns)
    keep = psi0.copy()
    sol = SPO3(*axes, [1.0, 1.0, 1.0], nstates=ns, coords="curvilinear", G=m["G"])
    sol.V = m["V"]
    took("")
    r = sol.run(psi0, dt=m["dt"], nt=nt, nout=nout)
    hit, paths = _took(shape, True)
    assert hit, paths
    ref = g3.run_ref(psi0, m["dt"], nt, m["ks"], m["V"], m["G"])
    bound = nt * 24.0 * fc.tol(max(shape))
    assert len(r.psilist) == 3 and np.array_equal(psi0, keep)
    rs = [relerr(r.psilist[k], ref[2 * k + 1]) / bound for k in range(3)] + [relerr(r.psi, ref[-1]) / bound]
    print(f"gmat3 SPO3 run: err/bound snapshots {rs[0]:.3e} {rs[1]:.3e} {rs[2]:.3e} final {rs[3]:.3e}")
    assert all(p.shape == shape + (ns,) for p in r.psilist) and fc.within(*rs), rs
    assert np.array_equal(r.psi, r.psilist[-1])
    assert sol.exp_K is None and sol.exp_V is None

    states = np.concatenate([psi0[None], ref[1::2]])
    w = np.prod([a[1] - a[0] for a in axes])
    rdm = w * np.einsum("kxyza,kxyzb->kab", states.conj(), states)
    pop = np.einsum("kaa->ka", rdm).real
    dens = np.abs(states) ** 2
    xave = [w * np.einsum("kxyza,x->k", dens, axes[0]), w * np.einsum("kxyza,y->k", dens, axes[1]),
            w * np.einsum("kxyza,z->k", dens, axes[2])]
    ro = sol.run(psi0, dt=m["dt"], nt=nt, nout=nout, observe="diabatic")
    assert len(ro.psilist) == 3 and all(np.array_equal(a, b) for a, b in zip(ro.psilist, r.psilist))
    assert np.array_equal(ro.psi, r.psi)
    assert ro.population.shape == (4, ns) and ro.rdm.shape == (4, ns, ns) and len(ro.xAve) == 3
    cap = 1e-13 + 2.0 * bound
    e = [relerr(ro.rdm, rdm), relerr(ro.population, pop)] + \
        [np.abs(ro.xAve[d] - xave[d]).max() / (np.abs(axes[d]).max() * pop.sum(axis=1).max()) for d in range(3)]
    print(f"gmat3 SPO3 observe: rdm {e[0]:.3e} population {e[1]:.3e} xAve {e[2]:.3e} {e[3]:.3e} {e[4]:.3e} cap {cap:.3e}")
    assert max(e) <= cap, e
    assert relerr(ro.rdm[0], rdm[0]) < 1e-13   # row 0 is psi0 itself
    rn = sol.run(psi0, dt=m["dt"], nt=nt, nout=nout, observe="diabatic", return_states=False)
    assert rn.psilist == [] and np.array_equal(rn.population, ro.population) and np.array_equal(rn.rdm, ro.rdm)
    assert np.array_equal(rn.psi, r.psi)
