"""Curvilinear (G-matrix) wavepacket propagation on the GPU: qd_wp2_gmat_apply / qd_wp2_gmat_rk4 and their Python
front (pyqed_amd.wpd KEO, hpsi, adiabatic_2d, curvilinear_run) against the numpy restatement of tests/gmat_models.py
(fft2 form, classical RK4: not the arithmetic under test) and the reference's own outputs in tests/golden/gmat2d.npz.

White-noise inputs, as in test_spo_whitenoise_gpu.py: every bin of every transform carries weight, so one wrong
element (1/128 of the norm on a 16 x 1024 grid) cannot hide in the L2 norm.  Bounds, in units of fft_cases.tol(n),
n the longer axis:
  operator: 5 = four chained transforms on the longest path (D_x, then D_x again: forward, inverse, forward, inverse)
            plus one for the point-wise products;
  run:      nt * 20 = four stages a step, each at most one application's error since dt ||H|| <= 1.

The power-of-two path has two column tiles (wp_gmat.hip): the wide one runs for nx >= 512 once B (ny / 4) reaches the
device's compute-unit count, and the library notes the tile it took (wp2_gmat_col_narrow / wp2_gmat_col_wide).  Every
test asserts the tile it expects; the wide one is reached with one large member (ny = 1024) and with a batch of
16-column members, whose narrow-tile single-member calls it must match bit for bit."""
import numpy as np
import pytest
import torch
from scipy.fftpack import fftfreq

from conftest import load_golden, relerr, took
import fft_cases as fc
import gmat_models as gm

pytestmark = pytest.mark.gpu

POW2_SHAPES = [(16, 16), (16, 32), (32, 16), (64, 128), (128, 64), (256, 16), (16, 256), (512, 16), (16, 512),
               (1024, 16), (16, 1024)]
ANY_SHAPES = [(24, 20), (67, 45), (12, 10), (50, 50), (61, 7), (5, 509), (3, 5), (8, 8), (1, 8), (8, 1), (32, 20),
              (20, 32), (2048, 4), (5125, 3), (3, 5125)]   # the last two take the four-step order
RUN_SHAPES = [(16, 16), (32, 16), (16, 1024), (1024, 16), (128, 64), (24, 20), (67, 45), (1, 8)]
WIDE_SHAPES = [(512, 1024), (1024, 1024)]   # B = 1: 256 wide workgroups
WIDE_BATCH_SHAPES = [(512, 16), (1024, 16)]   # B = _wide_batch(ny): the smallest batch that takes the wide tile


def _pow2(nx, ny):
    ok = lambda n: 16 <= n <= 1024 and n & (n - 1) == 0
    return ok(nx) and ok(ny)


def _path(nx, ny):
    return "wp2_gmat_pow2" if _pow2(nx, ny) else "wp2_gmat_any"


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _wide_batch(ny):
    """The smallest batch of [nx >= 512, ny] members that takes the wide column tile (64 at ny = 16 on 256 CUs)."""
    return -(-_cus() // (ny // 4))


def _expect(nx, ny, batch=1):
    """The path names a call on this shape must note, and the one tile name it must not."""
    if not _pow2(nx, ny):
        return ["wp2_gmat_any"], ["wp2_gmat_pow2", "wp2_gmat_col_narrow", "wp2_gmat_col_wide"]
    wide = nx >= 512 and batch * (ny // 4) >= _cus()
    tiles = ["wp2_gmat_col_narrow", "wp2_gmat_col_wide"]
    return ["wp2_gmat_pow2", tiles[wide]], ["wp2_gmat_any", tiles[not wide]]


def _took(nx, ny, batch=1):
    """The calls since the last check noted exactly the path (and tile) this shape must take."""
    got = took("")[1]
    want, never = _expect(nx, ny, batch)
    return all(w in got for w in want) and not any(n in got for n in never), got


def _noise(nx, ny, seed, batch=None):
    """Normalised white noise [nx, ny], or a batch [batch, nx, ny] of different members."""
    w = fc.noise(np.random.default_rng(seed), (batch or 1, nx, ny))
    w /= np.linalg.norm(w.reshape(len(w), -1), axis=1)[:, None, None]
    return w if batch else w[0]


@pytest.mark.parametrize("nx,ny", POW2_SHAPES + WIDE_SHAPES + ANY_SHAPES)
def test_operator_on_white_noise(nx, ny):
    from pyqed_amd.wpd import KEO, hpsi
    m = gm.model(nx, ny)
    w = _noise(nx, ny, 100 + nx + 3 * ny)
    took("")
    got_h = hpsi(w, m["kx"], m["ky"], m["v"], m["G"])
    hit, paths = _took(nx, ny)
    assert hit, paths
    got_k = KEO(w, m["kx"], m["ky"], m["G"])
    hit, paths = _took(nx, ny)
    assert hit, paths
    bound = 5.0 * fc.tol(max(nx, ny))
    r_h = relerr(got_h, gm.hpsi_ref(w, m["kx"], m["ky"], m["v"], m["G"])) / bound
    r_k = relerr(got_k, gm.keo_ref(w, m["kx"], m["ky"], m["G"])) / bound
    print(f"gmat operator {nx}x{ny}: hpsi err/bound {r_h:.3e}  KEO err/bound {r_k:.3e}")
    assert fc.within(r_h, r_k), (r_h, r_k)


@pytest.mark.parametrize("nx,ny", RUN_SHAPES + WIDE_SHAPES[:1])
def test_runs_on_white_noise(nx, ny):
    from pyqed_amd.wpd import curvilinear_run
    m = gm.model(nx, ny)
    nt, nout = 4, 2
    w = _noise(nx, ny, 200 + nx + 3 * ny)
    ref = gm.run_ref(w, m["dt"], nt, m["kx"], m["ky"], m["v"], m["G"])
    took("")
    psi, snap = curvilinear_run(m["x"], m["y"], w, m["v"], m["G"], m["dt"], nt, nout)
    hit, paths = _took(nx, ny)
    assert hit, paths
    assert tuple(psi.shape) == (1, nx, ny) and tuple(snap.shape) == (1, nt // nout, nx, ny)
    psi, snap = psi.cpu().numpy()[0], snap.cpu().numpy()[0]
    bound = nt * 20.0 * fc.tol(max(nx, ny))
    rs = [relerr(psi, ref[-1]) / bound, relerr(snap[0], ref[1]) / bound, relerr(snap[1], ref[3]) / bound]
    print(f"gmat run {nx}x{ny}: err/bound final {rs[0]:.3e} snapshots {rs[1]:.3e} {rs[2]:.3e}")
    assert fc.within(*rs), rs


@pytest.mark.parametrize("nx,ny", [(32, 16), (24, 20)])
def test_batch_members_equal_their_single_calls_bit_for_bit(nx, ny):
    from pyqed_amd.wpd import curvilinear_run, hpsi
    m = gm.model(nx, ny)
    dev = torch.device("cuda", 0)
    ws = torch.from_numpy(_noise(nx, ny, 7, batch=3)).to(dev)
    H = hpsi(ws, m["kx"], m["ky"], m["v"], m["G"])
    psi, snap = curvilinear_run(m["x"], m["y"], ws, m["v"], m["G"], m["dt"], 4, 2)
    assert tuple(H.shape) == (3, nx, ny) and tuple(snap.shape) == (3, 2, nx, ny)
    for b in range(3):
        assert torch.equal(H[b], hpsi(ws[b], m["kx"], m["ky"], m["v"], m["G"])), b
        p1, s1 = curvilinear_run(m["x"], m["y"], ws[b], m["v"], m["G"], m["dt"], 4, 2)
        assert torch.equal(psi[b], p1[0]) and torch.equal(snap[b], s1[0]), b
    assert not torch.equal(psi[0], psi[1])


@pytest.mark.parametrize("nx,ny", WIDE_BATCH_SHAPES)
def test_wide_column_tile_on_a_batch(nx, ny):
    """A batch large enough for the wide column tile: hpsi, KEO and a run (final state, both snapshots) of its first
    and last members within the white-noise bounds of the restatement, and every member of hpsi, three of the run,
    bit for bit equal to their single-member calls, which take the narrow tile."""
    from pyqed_amd.wpd import KEO, curvilinear_run, hpsi
    m = gm.model(nx, ny)
    B, nt, nout = _wide_batch(ny), 4, 2
    dev = torch.device("cuda", 0)
    w = _noise(nx, ny, 300 + nx, batch=B)
    ws = torch.from_numpy(w).to(dev)
    took("")
    H = hpsi(ws, m["kx"], m["ky"], m["v"], m["G"])
    hit, paths = _took(nx, ny, B)
    assert hit and "wp2_gmat_col_wide" in paths, paths
    K = KEO(ws, m["kx"], m["ky"], m["G"])
    psi, snap = curvilinear_run(m["x"], m["y"], ws, m["v"], m["G"], m["dt"], nt, nout)
    hit, paths = _took(nx, ny, B)
    assert hit and "wp2_gmat_col_wide" in paths, paths
    assert tuple(H.shape) == (B, nx, ny) and tuple(snap.shape) == (B, nt // nout, nx, ny)
    b_op, b_run = 5.0 * fc.tol(max(nx, ny)), nt * 20.0 * fc.tol(max(nx, ny))
    for b in (0, B - 1):
        ref = gm.run_ref(w[b], m["dt"], nt, m["kx"], m["ky"], m["v"], m["G"])
        rs = [relerr(H[b].cpu().numpy(), gm.hpsi_ref(w[b], m["kx"], m["ky"], m["v"], m["G"])) / b_op,
              relerr(K[b].cpu().numpy(), gm.keo_ref(w[b], m["kx"], m["ky"], m["G"])) / b_op,
              relerr(psi[b].cpu().numpy(), ref[-1]) / b_run, relerr(snap[b, 0].cpu().numpy(), ref[1]) / b_run,
              relerr(snap[b, 1].cpu().numpy(), ref[3]) / b_run]
        print(f"gmat wide tile {nx}x{ny} B={B} member {b}: err/bound hpsi {rs[0]:.3e} KEO {rs[1]:.3e} "
              f"run {rs[2]:.3e} snapshots {rs[3]:.3e} {rs[4]:.3e}")
        assert fc.within(*rs), (b, rs)
    took("")
    for b in range(B):
        assert torch.equal(H[b], hpsi(ws[b], m["kx"], m["ky"], m["v"], m["G"])), b
    for b in (0, B // 2, B - 1):
        assert torch.equal(K[b], KEO(ws[b], m["kx"], m["ky"], m["G"])), b
        p1, s1 = curvilinear_run(m["x"], m["y"], ws[b], m["v"], m["G"], m["dt"], nt, nout)
        assert torch.equal(psi[b], p1[0]) and torch.equal(snap[b], s1[0]), b
    hit, paths = _took(nx, ny, 1)
    assert hit and "wp2_gmat_col_narrow" in paths, paths
    assert not torch.equal(psi[0], psi[B - 1])


@pytest.mark.parametrize("tag", ["a", "b", "c"])
def test_adiabatic_2d_reproduces_the_reference_fixture(tag):
    from pyqed_amd.wpd import KEO, adiabatic_2d, hpsi
    g = load_golden("gmat2d")
    c = {k[2:]: v for k, v in g.items() if k.startswith(tag + "_")}
    psi0 = c["psi0"].copy()
    args = dict(Nt=int(c["nt"]), coords="curvilinear", G=c["G"])
    took("")
    out = adiabatic_2d(c["x"], c["y"], psi0, c["v"], float(c["dt"]), **args)
    assert took(_path(*psi0.shape))[0]
    assert isinstance(out, np.ndarray) and out.shape == psi0.shape
    assert relerr(out, c["psi"]) < 1e-11
    assert np.array_equal(psi0, c["psi0"])
    # a device tensor in gives a device tensor out, with the same numbers, and is not modified either
    t0 = torch.from_numpy(c["psi0"]).to("cuda:0")
    keep = t0.clone()
    out_t = adiabatic_2d(c["x"], c["y"], t0, c["v"], float(c["dt"]), **args)
    assert isinstance(out_t, torch.Tensor) and out_t.is_cuda
    assert np.array_equal(out_t.cpu().numpy(), out) and torch.equal(t0, keep)
    # a host tensor in gives a host tensor out
    out_c = adiabatic_2d(c["x"], c["y"], torch.from_numpy(c["psi0"]), c["v"], float(c["dt"]), **args)
    assert isinstance(out_c, torch.Tensor) and not out_c.is_cuda and np.array_equal(out_c.numpy(), out)
    # Nt = 0 returns a copy
    z = adiabatic_2d(c["x"], c["y"], psi0, c["v"], float(c["dt"]), Nt=0, coords="curvilinear", G=c["G"])
    assert z is not psi0 and np.array_equal(z, psi0)
    if "noise" in c:
        nx, ny = psi0.shape
        kx = 2.0 * np.pi * fftfreq(nx, c["x"][1] - c["x"][0])
        ky = 2.0 * np.pi * fftfreq(ny, c["y"][1] - c["y"][0])
        assert relerr(hpsi(c["noise"], kx, ky, c["v"], c["G"]), c["hpsi"]) < 1e-11
        assert relerr(KEO(c["noise"], kx, ky, c["G"]), c["keo"]) < 1e-11


@pytest.mark.parametrize("nx,ny,wide", [(32, 32, False), (512, 16, True)])
def test_rk4_call_replays_from_a_graph(nx, ny, wide):
    """qd_wp2_gmat_rk4 (32 x 32, B = 2, 4 steps; and 512 x 16 with a batch that takes the wide column tile) captured on
    a side stream and replayed twice from a restored input: both replays equal the eager call bit for bit (graph-owned
    scratch, no memset / memcpy nodes)."""
    from pyqed_amd import _lib
    dev = torch.device("cuda", 0)
    _lib.ensure_device(dev)
    lib = _lib.load()
    B = _wide_batch(ny) if wide else 2
    m = gm.model(nx, ny)
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)
    G, v, kx, ky = t(m["G"], float), t(m["v"], complex), t(m["kx"], float), t(m["ky"], float)
    psi0 = t(_noise(nx, ny, 9, batch=B), complex)
    s = torch.cuda.Stream(dev)

    def run(x, sn):
        _lib.check(lib.qd_wp2_gmat_rk4(x.data_ptr(), B, G.data_ptr(), v.data_ptr(), kx.data_ptr(), ky.data_ptr(), nx, ny,
                                       float(m["dt"]), 4, 2, sn.data_ptr(), s.cuda_stream), "qd_wp2_gmat_rk4")
    ref, ref_sn = psi0.clone(), torch.zeros((B, 2, nx, ny), dtype=torch.complex128, device=dev)
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
    hit, paths = _took(nx, ny, B)
    assert hit and ("wp2_gmat_col_wide" in paths) == wide, paths
    for _ in range(2):
        x.copy_(psi0)
        sn.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(x, ref) and torch.equal(sn, ref_sn)
    assert not torch.equal(ref, psi0)
