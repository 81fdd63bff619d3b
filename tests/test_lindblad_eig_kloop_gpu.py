"""The eigenbasis Lindblad kernel's K loops (lindblad_eig_kernel; cg_dma_block_gemm_stream_h and cg_dma_herm_d_gemm_h of
cgemm_dma128.hpp): a K-tile's eight LDS-DMA pieces per thread are issued from inside the k-steps of the tile before it
(the hook of cg_dma_ksteps), not ahead of them.  A piece that is never issued, or issued into the wrong slot, leaves
stale rows in one K-tile; a wait that no longer covers a piece shows as a race between two identical calls.  Every case
is forced onto the path with glf_path "eig" and holds the oracle's RK4 at the project's bound, exact Hermiticity, an
exactly real diagonal and bit equality of two identical calls (_check)."""
import numpy as np
import pytest

from conftest import relerr
from test_lindblad_eig_gpu import DT, TOL, _check, _exactly_hermitian, _run
from test_lindblad_kreg_gpu import inputs

pytestmark = pytest.mark.gpu

# the edges of the 4-row B pieces, the 32-row A rounds, the 16-row K-tiles and the last wave's pieces
PIECE_EDGES = [0, 3, 4, 7, 8, 15, 16, 31, 32, 63, 64, 95, 96, 124, 127]


def test_per_piece_coverage():
    """rho0 = |i><i| for i at every piece edge, one member each: a piece that misses its slot zeroes or keeps stale
    the rows it carries, and the one member whose population sits there is wrong.  Error per member."""
    from oracle import lindblad as olb
    H, cs, _ = inputs(128, 1, 1)
    rho0 = np.zeros((len(PIECE_EDGES), 128, 128), complex)
    for m, i in enumerate(PIECE_EDGES):
        rho0[m, i, i] = 1.0
    r = _check(H, cs, rho0, 2, "unit populations at the piece edges")
    ref = olb.lindblad_batch(H, cs, rho0, DT, 2)
    errs = [relerr(r[m], ref[m]) for m in range(len(PIECE_EDGES))]
    for i, e in zip(PIECE_EDGES, errs):
        print(f"  rho0 = |{i}><{i}|: rel err {e:.3e}")
    assert max(errs) < TOL, dict(zip(PIECE_EDGES, errs))


@pytest.mark.parametrize("steps", [1, 3])
def test_handover_branch(steps):
    """N = 128, n_c = 1, B = 8: the second GEMM starts with `two` = true (tile 0 issues nothing, tile 2 is first issued
    inside tile 1) and the Y GEMM's last tile stages the B half alone; three steps cross step boundaries."""
    _check(*inputs(128, 1, 8), steps, f"hand-over branch, {steps} step(s)")


@pytest.mark.parametrize("nc", [2, 3])
def test_lookahead_branch(nc):
    """N = 113, n_c = 2 and 3, B = 2, 3 steps: 16 and 24 K-tiles in the second GEMM (both tile parities of a segment
    change) and every Y GEMM's last tile stages a whole tile 0 for its follower."""
    _check(*inputs(113, nc, 2), 3, f"lookahead branch, n_c = {nc}")


def test_padding_from_tile_4():
    """N = 65, n_c = 1, B = 2: the padding begins inside K-tile 4, so tiles 5 to 7 stage zeros only and the padded
    parts of every operand must stay exactly zero for the unpadded result to hold the oracle."""
    _check(*inputs(65, 1, 2), 2, "padding from tile 4 on")


def test_full_occupancy():
    """B = 256, N = 128, n_c = 1, 2 steps, twice from the same input: one workgroup on every CU is the only setting in
    which the issue timing of a real run occurs.  Bit equality of the two results; members 0, 85, 170 and 255 hold the
    oracle."""
    from oracle import lindblad as olb
    H, cs, rho0 = inputs(128, 1, 256)
    r = _run(H, cs, rho0, 2)
    r2 = _run(H, cs, rho0, 2)
    assert np.array_equal(r, r2)
    assert _exactly_hermitian(r)
    assert np.all(np.diagonal(r, axis1=-2, axis2=-1).imag == 0.0)
    members = [0, 85, 170, 255]
    ref = olb.lindblad_batch(H, cs, rho0[members], DT, 2)
    errs = [relerr(r[m], ref[k]) for k, m in enumerate(members)]
    for m, e in zip(members, errs):
        print(f"  full occupancy, member {m}: rel err {e:.3e}")
    assert max(errs) < TOL, dict(zip(members, errs))


def test_observables_between_phases():
    """Two observables with t0: the observable pass sits between stage 3 and the next stage 0, between the last issue
    of one phase's K loop and the first of the next."""
    from oracle import lindblad as olb
    H, cs, rho0 = inputs(113, 1, 2)
    rng = np.random.default_rng(13)
    a = rng.standard_normal((113, 113)) + 1j * rng.standard_normal((113, 113))
    es = [np.diag(np.arange(113.0)).astype(complex), a + a.conj().T]
    steps = 3
    r, obs = _run(H, cs, rho0, steps, es=es)
    r2, obs2 = _run(H, cs, rho0, steps, es=es)
    assert obs.shape == (2, steps + 1, 2)
    for b in range(2):
        ref_obs, _, ref_rho = olb.lindblad(H, rho0[b], cs, es, steps, DT, keep_states=False)
        ref_obs = np.asarray(ref_obs).reshape(steps + 1, 2)
        eo, er = relerr(obs[b], ref_obs), relerr(r[b], ref_rho)
        print(f"observables, member {b}: obs rel err {eo:.3e}, rho rel err {er:.3e}")
        assert eo < TOL and er < TOL
    assert _exactly_hermitian(r)
    assert np.all(np.diagonal(r, axis1=-2, axis2=-1).imag == 0.0)
    assert np.array_equal(r, r2) and np.array_equal(obs, obs2)
    assert np.array_equal(r, _run(H, cs, rho0, steps))
