"""Sum-over-states signals on the GPU (csrc/sos_signals.hip behind pyqed_amd.sos and Mol): every public function against
the reference fixture, the factorised GSB + SE + ESA against the existing photon-echo kernel, edge shapes at every tile
constant against the NumPy restatement (tests/sos_models.py), the pole-sum primitive directly, and one graph capture.
The bound is the one tests/test_sos_gpu.py asserts for this module: norm-wise relerr < 1e-12."""
import ctypes

import numpy as np
import pytest
import torch

import sos_models as sm
from conftest import load_golden, relerr, took

pytestmark = pytest.mark.gpu

TOL = 1e-12

# pyqed_amd/csrc/sos_signals_tiles.hpp; each edge test below names the constant its sizes are there for
SOS_THREADS = 256   # inner pass: y points per workgroup; build pass: (p, q) entries per workgroup; TPA: points per group
SOS_QCHUNK = 256    # inner pass: (zy, W) pairs of a row staged per round
SOS_TILE = 16       # outer pass: output tile edge, along x and along y
SOS_PCHUNK = 64     # outer pass: poles staged per round


def around(c):
    return [c - 1, c, c + 1]


@pytest.fixture(scope="module")
def fx():
    return load_golden("sos_signals")


def check(got, ref, what=""):
    assert np.shape(got) == np.shape(ref), (what, np.shape(got), np.shape(ref))
    err = relerr(got, ref)
    print(f"{what}: relerr {err:.2e}")
    assert np.all(np.isfinite(got)), what
    assert err < TOL, (what, err)


def fresh_path():
    from pyqed_amd import _lib
    _lib.take_path()


# ------------------------------------------------------------------------------------------------ the fixture
def _mol(fx, tag):
    from pyqed_amd.mol import Mol
    mol = Mol(np.diag(fx[f"{tag}_E"]), fx[f"{tag}_dip"])
    mol.edip_rms = fx[f"{tag}_dip"]
    mol.set_decay(fx[f"{tag}_gamma"])
    mol.set_dephasing(float(fx[f"{tag}_pe_deph"]))
    return mol


def _fixture_calls(fx, tag):
    """name -> (callable returning the port's value, kernel path prefixes it must take, dtype)."""
    from pyqed_amd import sos
    v = lambda k: fx[f"{tag}_{k}"]
    E, dip, gamma, g, e, f = (v(k) for k in ("E", "dip", "gamma", "g", "e", "f"))
    mol = _mol(fx, tag)
    tau2, t3, deph, tau = float(v("tau2")), float(v("t3")), float(v("deph")), float(v("dq_tau"))
    kw = dict(g_idx=g, e_idx=e, f_idx=f, gamma=gamma)
    c, r = np.complex128, np.float64
    lw, lg = float(v("abs_linewidth")), float(v("la_gamma"))
    return {
        "GSB": (lambda: sos.GSB(E, dip, v("w1s"), v("w3s"), tau2, g, e, gamma), ["sos_gsb", "sos_polesum_ifast"], c),
        "SE": (lambda: sos.SE(E, dip, v("w1s"), v("w3s"), tau2, g, e, gamma), ["sos_se", "sos_polesum_ifast"], c),
        "ESA": (lambda: sos.ESA(E, dip, v("w1s"), v("w3s"), tau2, g, e, f, gamma), ["sos_esa", "sos_polesum_ifast"], c),
        "SE_t3": (lambda: sos._SE(E, dip, v("w1"), v("w2"), t3, g, e, gamma, dephasing=deph), ["sos_se_t3"], c),
        "ESA_t3": (lambda: sos._ESA(E, dip, v("w1"), v("w2"), t3, g, e, f, gamma, dephasing=deph), ["sos_esa_t3"], c),
        "SE_t3_default": (lambda: sos._SE(E, dip, v("w1"), v("w2"), t3, g, e, gamma), ["sos_se_t3"], c),
        "PE2": (lambda: mol.PE2(v("pe_w1"), v("w2"), t3=t3), ["sos_se_t3", "sos_esa_t3"], c),
        "PE2_se": (lambda: mol.PE2(v("pe_w1"), v("w2"), t3=t3, separate=True)[0], ["sos_se_t3", "sos_esa_t3"], c),
        "PE2_esa": (lambda: mol.PE2(v("pe_w1"), v("w2"), t3=t3, separate=True)[1], ["sos_se_t3", "sos_esa_t3"], c),
        "PE2_se_lists": (lambda: mol.PE2(v("pe_w1"), v("w2"), t3=t3, separate=True, g_idx=g, e_idx=e, f_idx=f)[0],
                         ["sos_se_t3"], c),
        "PE2_esa_lists": (lambda: mol.PE2(v("pe_w1"), v("w2"), t3=t3, separate=True, g_idx=g, e_idx=e, f_idx=f)[1],
                          ["sos_esa_t3"], c),
        "DQC_R1_t3": (lambda: sos.DQC_R1(E, dip, omega1=v("dq_w1"), omega2=v("dq_w2"), tau3=tau, **kw),
                      ["sos_dqc_r1_t3", "sos_polesum_jfast"], c),
        "DQC_R1_t1": (lambda: sos.DQC_R1(E, dip, omega2=v("dq_w2"), omega3=v("dq_w3"), tau1=tau, **kw),
                      ["sos_dqc_r1_t1", "sos_polesum_jfast"], c),
        "DQC_R2_t3": (lambda: sos.DQC_R2(E, dip, omega1=v("dq_w1"), omega2=v("dq_w2"), tau3=tau, **kw),
                      ["sos_dqc_r2_t3"], c),
        "DQC_R2_t1": (lambda: sos.DQC_R2(E, dip, omega2=v("dq_w2"), omega3=v("dq_w3"), tau1=tau, **kw),
                      ["sos_dqc_r2_t1"], c),
        "TPA_scalar": (lambda: sos.TPA(E, dip, 2.1, g, e, f, gamma), ["sos_tpa"], r),
        "TPA_array": (lambda: sos.TPA(E, dip, v("tpa_wp"), g, e, f, gamma), ["sos_tpa"], r),
        "TPA2D": (lambda: sos.TPA2D(E, dip, v("tpa_wp"), v("tpa_w1"), g, e, f, gamma), ["sos_tpa"], r),
        "TPA2D_time_order": (lambda: sos.TPA2D_time_order(E, dip, v("tpa_wp"), v("tpa_w1"), g, e, f, gamma),
                             ["sos_tpa"], r),
        "cars": (lambda: sos.cars(E, dip, v("cars_shift"), v("cars_w1"), gamma=float(v("cars_gamma"))),
                 ["sos_cars", "sos_polesum_ifast"], c),
        "Mol_cars": (lambda: mol.cars(v("cars_shift"), v("cars_w1"), plt_signal=True, fname="x"), ["sos_cars"], c),
        "absorption_lw": (lambda: mol.absorption(v("abs_w"), linewidth=lw), ["sos_polesum"], r),
        "absorption_default": (lambda: mol.absorption(v("abs_w"), plt_signal=False), ["sos_polesum"], r),
        "absorption_norm": (lambda: mol.absorption(v("abs_w"), linewidth=lw, normalize=True), ["sos_polesum"], r),
        "linear_absorption": (lambda: sos.linear_absorption(v("abs_w"), v("la_e"), v("la_d"), gamma=lg),
                              ["sos_polesum"], r),
        "linear_absorption_norm": (lambda: sos.linear_absorption(v("abs_w"), v("la_e"), v("la_d"), gamma=lg,
                                                                 normalize=True), ["sos_polesum"], r),
    }


FIXTURE_NAMES = ["GSB", "SE", "ESA", "SE_t3", "ESA_t3", "SE_t3_default", "PE2", "PE2_se", "PE2_esa", "PE2_se_lists",
                 "PE2_esa_lists", "DQC_R1_t3", "DQC_R1_t1", "DQC_R2_t3", "DQC_R2_t1", "TPA_scalar", "TPA_array", "TPA2D",
                 "TPA2D_time_order", "cars", "Mol_cars", "absorption_lw", "absorption_default", "absorption_norm",
                 "linear_absorption", "linear_absorption_norm"]


@pytest.mark.parametrize("name", FIXTURE_NAMES)
@pytest.mark.parametrize("tag", ["a", "b"])
def test_matches_the_reference_fixture(fx, tag, name, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)   # photon_echo_t3 writes its .npz into the working directory
    calls = _fixture_calls(fx, tag)
    assert sorted(calls) == sorted(FIXTURE_NAMES)
    call, paths, dtype = calls[name]
    fresh_path()
    got = call()
    from pyqed_amd import _lib
    taken = _lib.take_path().split()
    for p in paths:
        assert any(t.startswith(p) for t in taken), (p, taken)
    assert np.asarray(got).dtype == dtype, name
    check(got, fx[f"{tag}_{name}"], f"{tag} {name}")


@pytest.mark.parametrize("tag", ["a", "b"])
def test_photon_echo_t3_writes_the_reference_files(fx, tag, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    mol = _mol(fx, tag)
    w1, w2, t3 = fx[f"{tag}_pe_w1"], fx[f"{tag}_w2"], float(fx[f"{tag}_t3"])
    S = mol.PE2(w1, w2, t3=t3)
    z = np.load(tmp_path / "2DES.npz")
    assert z.files == ["arr_0", "arr_1", "arr_2"]
    assert np.array_equal(z["arr_0"], w1) and np.array_equal(z["arr_1"], w2) and np.array_equal(z["arr_2"], S)
    se, esa = mol.PE2(w1, w2, t3=t3, separate=True, fname="sep")
    z = np.load(tmp_path / "sep.npz")
    assert z.files == ["arr_0", "arr_1", "arr_2", "arr_3"]
    assert np.array_equal(z["arr_2"], se) and np.array_equal(z["arr_3"], esa)
    check(se + esa, S, "se + esa against the accumulated call")


def test_mol_pe_is_photon_echo(tmp_path, monkeypatch):
    from pyqed_amd.mol import Mol
    monkeypatch.chdir(tmp_path)
    g = load_golden("photon_echo")
    mol = Mol(g["r4_H"], g["r4_dip"])
    mol.edip_rms = g["r4_dip"]
    mol.gamma = g["r4_gamma"]
    S = mol.PE(g["r4_pump"], g["r4_probe"], t2=float(g["r4_t2"]))
    check(S, g["r4_S"], "Mol.PE r4")


def test_factorised_echo_matches_the_photon_echo_kernel():
    """GSB + SE + ESA from qd_sos_pathway against the existing qd_photon_echo on the r4 case of photon_echo.npz."""
    from pyqed_amd import sos
    g = load_golden("photon_echo")
    E = np.diagonal(g["r4_H"]).astype(complex)
    dip, gamma, t2 = g["r4_dip"], g["r4_gamma"], float(g["r4_t2"])
    w1, w3 = -g["r4_pump"], g["r4_probe"]
    idx = range(len(E))
    old = sos._photon_echo(E, dip, w1, w3, t2, [0], idx, idx, gamma)
    new = (sos.GSB(E, dip, w1, w3, t2, [0], idx, gamma) + sos.SE(E, dip, w1, w3, t2, [0], idx, gamma) +
           sos.ESA(E, dip, w1, w3, t2, [0], idx, idx, gamma))
    check(new, old, "GSB + SE + ESA against qd_photon_echo")
    check(new, g["r4_S"], "GSB + SE + ESA against the reference")


# ------------------------------------------------------------------------------------------------ edge shapes
def rand_model(N, seed):
    """E_0 = 0 below a band of N - 1 levels, complex Hermitian dipoles, gamma in [0.02, 0.2]."""
    rng = np.random.default_rng(seed)
    E = np.concatenate([[0.0], np.sort(rng.uniform(0.8, 2.6, N - 1))])
    d = rng.standard_normal((N, N)) + 1j * rng.standard_normal((N, N))
    return E, (d + d.conj().T) / 2, rng.uniform(0.02, 0.2, N)


def grids(na, nb, seed=0):
    rng = np.random.default_rng(100 + seed)
    return np.sort(rng.uniform(-2.8, 2.8, na)), np.sort(rng.uniform(-2.8, 2.8, nb))


def lists(ng, ne, nf):
    return list(range(ng)), list(range(ng, ng + ne)), list(range(ng + ne, ng + ne + nf))


T, DEPH = 1.3, 0.03


def pathway_pair(name, E, dip, gamma, g, e, f, wa, wb):
    """(the port's value, the restatement's) of one pathway on grids wa, wb in the reference's argument order."""
    from pyqed_amd import sos
    kw = dict(g_idx=g, e_idx=e, f_idx=f, gamma=gamma)
    if name == "GSB":
        return sos.GSB(E, dip, wa, wb, T, g, e, gamma), sm.GSB(E, dip, wa, wb, T, g, e, gamma)
    if name == "SE":
        return sos.SE(E, dip, wa, wb, T, g, e, gamma), sm.SE(E, dip, wa, wb, T, g, e, gamma)
    if name == "ESA":
        return sos.ESA(E, dip, wa, wb, T, g, e, f, gamma), sm.ESA(E, dip, wa, wb, T, g, e, f, gamma)
    if name == "SE_T3":
        return sos._SE(E, dip, wa, wb, T, g, e, gamma, dephasing=DEPH), sm.SE_t3(E, dip, wa, wb, T, g, e, gamma, DEPH)
    if name == "ESA_T3":
        return (sos._ESA(E, dip, wa, wb, T, g, e, f, gamma, dephasing=DEPH),
                sm.ESA_t3(E, dip, wa, wb, T, g, e, f, gamma, DEPH))
    if name == "DQC_R1_T3":
        return sos.DQC_R1(E, dip, omega1=wa, omega2=wb, tau3=T, **kw), sm.DQC_R1(E, dip, omega1=wa, omega2=wb, tau3=T, **kw)
    if name == "DQC_R1_T1":
        return sos.DQC_R1(E, dip, omega2=wa, omega3=wb, tau1=T, **kw), sm.DQC_R1(E, dip, omega2=wa, omega3=wb, tau1=T, **kw)
    if name == "DQC_R2_T3":
        return sos.DQC_R2(E, dip, omega1=wa, omega2=wb, tau3=T, **kw), sm.DQC_R2(E, dip, omega1=wa, omega2=wb, tau3=T, **kw)
    if name == "DQC_R2_T1":
        return sos.DQC_R2(E, dip, omega2=wa, omega3=wb, tau1=T, **kw), sm.DQC_R2(E, dip, omega2=wa, omega3=wb, tau1=T, **kw)
    if name == "CARS":
        return sos.cars(E, dip, wa, wb, gamma=0.05), sm.cars(E, dip, wa, wb, gamma=0.05)
    if name == "TPA2D":
        return sos.TPA2D(E, dip, wa, wb, g, e, f, gamma), sm.TPA2D(E, dip, wa, wb, g, e, f, gamma)
    if name == "TPA2D_time_order":
        return (sos.TPA2D_time_order(E, dip, wa, wb, g, e, f, gamma),
                sm.TPA2D_time_order(E, dip, wa, wb, g, e, f, gamma))
    raise KeyError(name)


PATHWAYS = ["GSB", "SE", "ESA", "SE_T3", "ESA_T3", "DQC_R1_T3", "DQC_R1_T1", "DQC_R2_T3", "DQC_R2_T1", "CARS"]
ALL2D = PATHWAYS + ["TPA2D", "TPA2D_time_order"]


@pytest.mark.parametrize("shape", [(1, 1), (1, 5), (5, 1), (2, 3)])
@pytest.mark.parametrize("name", ALL2D)
def test_small_grids(name, shape):
    E, dip, gamma = rand_model(9, 1)
    g, e, f = lists(2, 3, 4)
    wa, wb = grids(*shape)
    got, ref = pathway_pair(name, E, dip, gamma, g, e, f, wa, wb)
    check(got, ref, f"{name} {shape}")


# x is the axis paired with the outer sum, y the one of the inner sums.  ESA: x = the first grid, output x-fastest (the
# i-fast outer kernel); DQC_R2_T3: x = the first grid, output y-fastest (j-fast); DQC_R1_T3: the diagonal x factor;
# CARS: x = the second grid.  SOS_TILE bounds the outer tile along x and along y, SOS_THREADS the inner pass along y.
GRID_EDGES = ([(n, 3) for n in around(SOS_TILE)] + [(3, n) for n in around(SOS_TILE)] +      # SOS_TILE, x and y
              [(n, 3) for n in around(SOS_THREADS)] + [(3, n) for n in around(SOS_THREADS)])  # SOS_THREADS, y (and x)


@pytest.mark.parametrize("shape", GRID_EDGES)
@pytest.mark.parametrize("name", ["ESA", "DQC_R2_T3", "DQC_R1_T3", "CARS"])
def test_grid_sizes_at_the_tile_and_workgroup_edges(name, shape):
    E, dip, gamma = rand_model(9, 2)
    g, e, f = lists(1, 4, 4)
    wa, wb = grids(*shape, seed=1)
    got, ref = pathway_pair(name, E, dip, gamma, g, e, f, wa, wb)
    check(got, ref, f"{name} {shape}")


@pytest.mark.parametrize("shape", [(n, 1) for n in around(SOS_THREADS)] + [(3, 85), (16, 16), (1, 257)])
def test_tpa_points_at_the_workgroup_edge(shape):
    """SOS_THREADS: grid points per workgroup of the TPA kernel (255, 256, 257 points; also as 3 x 85, 16 x 16)."""
    E, dip, gamma = rand_model(9, 3)
    g, e, f = lists(1, 4, 4)
    wa, wb = grids(*shape, seed=2)
    for name in ("TPA2D", "TPA2D_time_order"):
        got, ref = pathway_pair(name, E, dip, gamma, g, e, f, wa, wb)
        check(got, ref, f"{name} {shape}")
    from pyqed_amd import sos
    check(sos.TPA(E, dip, wa, g, e, f, gamma), sm.TPA(E, dip, wa, g, e, f, gamma), f"TPA {shape[0]}")


# P = ne and Q = nf for ESA and DQC_R2_T3; P = nf, Q = ne for DQC_R1_T1; Q = ne * ng for SE.
@pytest.mark.parametrize("name,ng,ne,nf", (
    [("ESA", 1, n, 3) for n in around(SOS_PCHUNK)] +            # SOS_PCHUNK: poles per round of the outer pass (i-fast)
    [("DQC_R2_T3", 1, n, 3) for n in around(SOS_PCHUNK)] +      # SOS_PCHUNK (j-fast)
    [("DQC_R1_T1", 1, 3, n) for n in around(2 * SOS_PCHUNK)] +  # two rounds, P from the f list
    [("ESA", 1, 2, n) for n in around(SOS_QCHUNK)] +            # SOS_QCHUNK: (zy, W) pairs per round of the inner pass
    [("SE", 2, n, 0) for n in (127, 128, 129)] +                # SOS_QCHUNK through Q = ne * ng = 254, 256, 258
    [("ESA", 1, 15, 17), ("ESA", 1, 16, 16), ("ESA", 1, 1, 257),  # SOS_THREADS: P * Q = 255, 256, 257 in the build pass
     ("DQC_R1_T3", 1, 1, 257)]))
def test_index_list_lengths_at_the_chunk_edges(name, ng, ne, nf):
    E, dip, gamma = rand_model(ng + ne + nf, 4)
    g, e, f = lists(ng, ne, nf)
    wa, wb = grids(5, 4, seed=3)
    got, ref = pathway_pair(name, E, dip, gamma, g, e, f, wa, wb)
    check(got, ref, f"{name} ng={ng} ne={ne} nf={nf}")


@pytest.mark.parametrize("ng,ne,nf", [(1, 0, 3), (1, 3, 0), (0, 3, 3), (1, 1, 1), (2, 2, 2), (3, 37, 21)])
@pytest.mark.parametrize("name", PATHWAYS[:-1] + ["TPA2D"])
def test_index_list_lengths(name, ng, ne, nf):
    """Lists of length 0, 1, 2 and 37 / 21 (no multiple of any tile constant); an empty list that a pathway sums over
    gives zeros of the right shape and dtype."""
    E, dip, gamma = rand_model(max(ng + ne + nf, 2), 5)
    g, e, f = lists(ng, ne, nf)
    wa, wb = grids(6, 5, seed=4)
    got, ref = pathway_pair(name, E, dip, gamma, g, e, f, wa, wb)
    assert got.dtype == (np.float64 if name == "TPA2D" else np.complex128)
    if not np.any(ref):
        assert got.shape == ref.shape and not np.any(got), name
    else:
        check(got, ref, f"{name} ng={ng} ne={ne} nf={nf}")


def test_one_dimensional_signals_at_the_tile_edges():
    """absorption / linear_absorption: the pole sum on a one-column grid.  SOS_TILE bounds the tile along the
    frequency axis, SOS_PCHUNK the round of poles (two poles per transition: 31, 32, 33 transitions)."""
    from pyqed_amd import sos
    from pyqed_amd.mol import Mol
    for nw in around(SOS_TILE) + [1]:
        for N in (32, 33, 34, 2, 1):
            E, dip, _ = rand_model(max(N, 2), 6)
            E, dip = E[:N], dip[:N, :N]
            w = np.sort(np.random.default_rng(nw).uniform(0.5, 2.8, nw))
            got = Mol(np.diag(E), dip).absorption(w, linewidth=0.03)
            assert got.dtype == np.float64 and got.shape == (nw,)
            if N == 1:
                assert not got.any()
                continue
            check(got, sm.absorption(E, dip, w, linewidth=0.03), f"absorption nw={nw} N={N}")
            check(sos.linear_absorption(w, E[1:], dip[1:, 0].real, gamma=0.04),
                  sm.linear_absorption(w, E[1:], dip[1:, 0].real, gamma=0.04), f"linear_absorption nw={nw} N={N}")


# ------------------------------------------------------------------------------------------------ the primitive
POLE, UNITY, DIAG = 0, 1, 2


def polesum_ref(zx, zy, W, x, y, xkind, ykind):
    fy = 1.0 / (y[None, None, :] - zy[:, :, None]) if ykind == POLE else np.ones(W.shape + (len(y),))
    inner = np.einsum("pq,pqj->pj", W, fy)
    if xkind == DIAG:
        return np.tile((inner / (y[None, :] - zx[:, None])).sum(0), (len(x), 1))
    Gx = 1.0 / (x[:, None] - zx[None, :]) if xkind == POLE else np.ones((len(x), len(zx)))
    return Gx @ inner


def polesum_call(zx, zy, W, x, y, xkind, ykind, S, si, sj, accumulate):
    """S: device tensor, written through the strides."""
    from pyqed_amd import _lib
    dev = S.device
    _lib.ensure_device(dev)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    P, Q = W.shape
    t = [up(a) for a in (zx, zy, W, x, y)]
    p = [a.data_ptr() if a.numel() else None for a in t]
    with torch.cuda.device(dev):
        rc = _lib.load().qd_sos_polesum(p[0], p[1], p[2], P, Q, p[3], len(x), p[4], len(y), xkind, ykind, S.data_ptr(),
                                        si, sj, int(accumulate), _lib.stream_ptr(dev))
    _lib.check(rc, "qd_sos_polesum")
    torch.cuda.synchronize()


def polesum_inputs(P, Q, n0, n1, seed):
    rng = np.random.default_rng(seed)
    cpx = lambda *s: rng.standard_normal(s) + 1j * rng.standard_normal(s)
    zx = rng.uniform(-2, 2, P) - 1j * rng.uniform(0.02, 0.2, P)
    zy = rng.uniform(-2, 2, (P, Q)) - 1j * rng.uniform(0.02, 0.2, (P, Q))
    # real grids, so |x - z| >= |Im z| >= 0.02
    return zx, zy, cpx(P, Q), np.sort(rng.uniform(-2.5, 2.5, n0)), np.sort(rng.uniform(-2.5, 2.5, n1))


@pytest.mark.parametrize("P,Q", [(150, 600),   # P crosses SOS_PCHUNK twice, Q crosses SOS_QCHUNK twice
                                 (0, 5), (5, 0), (0, 0), (1, 7), (1, 1)] +
                         [(p, 3) for p in around(SOS_PCHUNK)] + [(3, q) for q in around(SOS_QCHUNK)])
@pytest.mark.parametrize("layout", ["ij", "ji", "ij_pitched", "ji_pitched"])
def test_polesum_primitive(P, Q, layout):
    """qd_sos_polesum against Gx @ (W o 1 / (y - zy)) summed over q: both output orientations, with and without a row
    pitch, accumulate on and off, NaN-prefilled output (no NaN survives, nothing outside the strides is touched), and two
    identical calls bit for bit."""
    dev = torch.device("cuda", 0)
    n0, n1 = 37, 45
    zx, zy, W, x, y = polesum_inputs(P, Q, n0, n1, seed=P * 1000 + Q)
    ref = polesum_ref(zx, zy, W, x, y, POLE, POLE)
    pitch = 3 if layout.endswith("pitched") else 0
    if layout.startswith("ij"):
        rows, cols, si, sj = n0, n1 + pitch, n1 + pitch, 1
        view = lambda buf: buf[:, :n1]
    else:
        rows, cols, si, sj = n1, n0 + pitch, 1, n0 + pitch
        view = lambda buf: buf[:, :n0].T
    nan = complex(np.nan, np.nan)
    buf = torch.full((rows, cols), nan, dtype=torch.complex128, device=dev)
    fresh_path()
    polesum_call(zx, zy, W, x, y, POLE, POLE, buf, si, sj, False)
    ok, got_paths = took("sos_polesum_ifast" if si == 1 else "sos_polesum_jfast")
    assert ok, got_paths
    host = buf.cpu().numpy()
    got = view(host)
    assert not np.isnan(got).any()
    if pitch:
        assert np.isnan(host[:, -pitch:]).all()
    if P and Q:
        check(got, ref, f"polesum {layout} P={P} Q={Q}")
    else:
        assert not got.any()
    buf2 = torch.full((rows, cols), nan, dtype=torch.complex128, device=dev)
    polesum_call(zx, zy, W, x, y, POLE, POLE, buf2, si, sj, False)
    assert np.array_equal(view(buf2.cpu().numpy()), got)
    # accumulate onto a known array
    base = np.random.default_rng(7).standard_normal((rows, cols)) + 0j
    buf3 = torch.from_numpy(base.copy()).to(dev)
    polesum_call(zx, zy, W, x, y, POLE, POLE, buf3, si, sj, True)
    host3 = buf3.cpu().numpy()
    if P and Q:
        check(view(host3) - view(base), ref, f"polesum accumulate {layout} P={P} Q={Q}")
    else:
        assert np.array_equal(host3, base)
    if pitch:
        assert np.array_equal(host3[:, -pitch:], base[:, -pitch:])


@pytest.mark.parametrize("xkind,ykind", [(UNITY, POLE), (DIAG, POLE), (POLE, UNITY), (UNITY, UNITY), (DIAG, UNITY)])
@pytest.mark.parametrize("P,Q,n0,n1", [(70, 300, 19, 33), (5, 4, 1, 6), (5, 4, 6, 1), (1, 1, 1, 1)])
def test_polesum_factor_kinds(xkind, ykind, P, Q, n0, n1):
    dev = torch.device("cuda", 0)
    zx, zy, W, x, y = polesum_inputs(P, Q, n0, n1, seed=11)
    ref = polesum_ref(zx, zy, W, x, y, xkind, ykind)
    nan = complex(np.nan, np.nan)
    for si, sj, shape, view in ((n1, 1, (n0, n1), lambda a: a), (1, n0, (n1, n0), lambda a: a.T)):
        buf = torch.full(shape, nan, dtype=torch.complex128, device=dev)
        polesum_call(zx, zy, W, x, y, xkind, ykind, buf, si, sj, False)
        got = view(buf.cpu().numpy())
        check(got, ref, f"kinds ({xkind}, {ykind}) strides ({si}, {sj})")
        if xkind == DIAG:
            assert np.array_equal(got, np.tile(got[0], (n0, 1)))


# ------------------------------------------------------------------------------------------------ graph capture
def test_pathway_call_replays_from_a_graph():
    """One qd_sos_pathway call (build, inner and outer kernels on capture-owned scratch) captured into a graph and
    replayed twice equals the direct call bit for bit."""
    from pyqed_amd import _lib
    dev = torch.device("cuda", 0)
    _lib.ensure_device(dev)
    lib = _lib.load()
    E, dip, gamma = rand_model(40, 8)
    g, e, f = lists(1, 20, 19)
    wa, wb = grids(50, 70, seed=5)
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=dt))).to(dev)
    Et, Dt, Gt = up(E, complex), up(dip, complex), up(gamma, float)
    gi, ei, fi = (up(v, np.int32) for v in (g, e, f))
    xa, xb = up(wa, float), up(wb, float)
    s = torch.cuda.Stream(dev)

    def run(S):
        _lib.check(lib.qd_sos_pathway(2, Et.data_ptr(), Dt.data_ptr(), Gt.data_ptr(), len(E), 0.0, gi.data_ptr(), 1,
                                      ei.data_ptr(), 20, fi.data_ptr(), 19, T, xa.data_ptr(), 50, xb.data_ptr(), 70,
                                      S.data_ptr(), 0, s.cuda_stream), "qd_sos_pathway")
    ref = torch.zeros((70, 50), dtype=torch.complex128, device=dev)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        run(ref)
    torch.cuda.synchronize()
    check(ref.cpu().numpy(), sm.ESA(E, dip, wa, wb, T, g, e, f, gamma), "eager ESA")
    out = torch.zeros_like(ref)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        run(out)
    out.zero_()
    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, ref)
