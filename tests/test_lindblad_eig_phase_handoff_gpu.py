"""The eigenbasis Lindblad kernel's hand-over from one phase to the next (lindblad_eig_kernel, glf_eig_kernel.hpp): rows
0 .. 31 of a phase's result go from eig_tail's registers into L.b[0] and L.b[1] as the B halves of K-tiles 0 and 1 of the
next phase's Y GEMM (rows 16 .. 31 of column tile 0 as wave 0's conjugate transpose, the lower triangles of the diagonal
tiles as conjugates), the A halves arrive by DMA under the second GEMM's last K-tile and under the Y GEMM's tile 0, the
barrier between the phases drains nothing and the Y GEMM starts without a prologue.  A wrong slot, tile owner, sign or
wait shows in the members and entries chosen here.  Every case is forced onto the path with glf_path "eig" and holds the
oracle's RK4 at the project's bound, exact Hermiticity, an exactly real diagonal and bit equality of two identical calls
(_check)."""
import numpy as np
import pytest

from conftest import qd_option, relerr
from test_lindblad_eig_gpu import DT, TOL, TOL_SELF, _check, _dev, _exactly_hermitian, _run
from test_lindblad_kreg_gpu import BLOCK_PERM, block_permutation, inputs, permuted

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("steps", [1, 3])
def test_every_boundary(steps):
    """N = 128, n_c = 1, B = 2.  One step has all four kinds of boundary (basis change -> stage, stage -> stage, stage
    -> basis change, and Y GEMM -> second GEMM within a phase); three steps add stage 3 -> stage 0."""
    _check(*inputs(128, 1, 2), steps, f"phase hand-over, {steps} step(s)")


# (i, j) at the edges of what travels through LDS
ENTRIES = [(16, 0), (31, 15), (16, 15),   # the transposed tile (1, 0), written by wave 0 from its tile (0, 1)
           (17, 16), (1, 0),              # the lower triangles of the diagonal tiles (1, 1) and (0, 0)
           (31, 127), (32, 16)]           # the last row that travels, and the first that does not


def test_per_entry_edges():
    """rho0 = a E_ij + conj(a) E_ji with a = 1 + 2i, one matrix per entry: the complex a makes a wrong sign in a
    conjugated tile show up.  Error per member against the oracle."""
    from oracle import lindblad as olb
    H, cs, _ = inputs(128, 1, 1)
    a = 1.0 + 2.0j
    rho0 = np.zeros((len(ENTRIES), 128, 128), complex)
    for m, (i, j) in enumerate(ENTRIES):
        rho0[m, i, j] = a
        rho0[m, j, i] = np.conj(a)
    r = _check(H, cs, rho0, 2, "single entries")
    ref = olb.lindblad_batch(H, cs, rho0, DT, 2)
    errs = [relerr(r[m], ref[m]) for m in range(len(ENTRIES))]
    for ij, e in zip(ENTRIES, errs):
        print(f"  rho0 = a E_{ij} + h.c.: rel err {e:.3e}")
    assert max(errs) < TOL, dict(zip(ENTRIES, errs))


def test_block_permutation():
    """P rho P^T under P H P^T, P C P^T for a permutation of the 16-blocks, un-permuted, against the plain run, 5 steps:
    other blocks then lie in rows 0 .. 31, so a wrong tile owner or transposed address moves with the permutation."""
    assert len(BLOCK_PERM) == 8
    H, cs, rho0 = inputs(128, 1, 2)
    r = _check(H, cs, rho0, 5, "block permutation, plain")
    perm = block_permutation()
    rp = _run(*permuted(H, cs, rho0, perm), 5)
    assert _exactly_hermitian(rp)
    inv = np.argsort(perm)
    err = relerr(rp[:, inv][:, :, inv], r)
    print(f"block permutation: un-permuted against plain run, rel err {err:.3e}")
    assert err < TOL_SELF


@pytest.mark.parametrize("N", [65, 113])
def test_padding(N):
    """The padding begins beyond rows 0 .. 31 (inside tile 4 and inside tile 7); the padded parts of the rows that travel
    stay exactly zero: the un-padded result would otherwise miss the oracle or Hermiticity."""
    _check(*inputs(N, 1, 2), 2, f"padding, N = {N}")


@pytest.mark.parametrize("nc", [2, 3])
def test_more_collapse_operators(nc):
    """n_c = 2, 3 at N = 113: the hand-over feeds the Y GEMM of c = 0; the GEMM-to-GEMM lookaheads stay as they are."""
    _check(*inputs(113, nc, 2), 3, f"n_c = {nc}")


def test_observables_between_phases():
    """Two observables with t0, 3 steps: the observable pass stands between a phase and the one it handed its tiles
    to (behind the first basis change and behind every step) and reads the state from memory.  Against the oracle,
    and the state with and without observables is bit-equal."""
    from oracle import lindblad as olb
    H, cs, rho0 = inputs(113, 1, 2)
    rng = np.random.default_rng(14)
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


def test_graph_capture_warm_plan():
    """A captured call with a warm plan, replayed twice, equals two direct calls bit for bit."""
    import torch
    from pyqed_amd import _lib, lindblad_rk4
    H, cs, rho0 = inputs(128, 1, 2)
    Ht, Ct, r0, _ = _dev(H, cs, rho0)
    s = torch.cuda.Stream(torch.device("cuda", 0))
    with qd_option("glf_path", "eig"):
        ref = r0.clone()
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            for _ in range(2):
                lindblad_rk4(Ht, Ct, ref, DT, 3, hermitian=True, stream=s.cuda_stream)   # builds and caches the plan
        torch.cuda.synchronize()
        x = r0.clone()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        _lib.take_path()
        with torch.cuda.graph(g, stream=s):
            lindblad_rk4(Ht, Ct, x, DT, 3, hermitian=True, stream=s.cuda_stream)
        assert "glf_eig" in _lib.take_path().split()
        x.copy_(r0)
        g.replay()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(x, ref)
