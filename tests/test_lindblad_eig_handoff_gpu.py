"""The eigenbasis Lindblad kernel's hand-over through LDS (lindblad_eig_kernel, glf_eig_kernel.hpp): at n_c = 1 the
first two K-tiles of the second GEMM's A operand (columns 0 .. 31 of Y) go from the accumulators into the staging
buffers and never to memory, their B halves arrive by DMA around a raw barrier, and at n_c >= 2 the last Y GEMM stages
the second GEMM's first K-tile as its lookahead.  A wrong slot, tile owner or wait shows in the members and entries
chosen here, which also cover the rows 0 .. 15 that a pre-staged first K-tile of the next phase would carry.  Every
case is forced onto the path with glf_path "eig" and holds the oracle's RK4 at the project's bound, exact Hermiticity,
an exactly real diagonal and bit equality of two identical calls (_check)."""
import numpy as np
import pytest

from conftest import qd_option, relerr
from test_lindblad_eig_gpu import DT, TOL, TOL_SELF, _check, _dev, _exactly_hermitian, _run
from test_lindblad_kreg_gpu import inputs

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("steps", [1, 3])
def test_basic_handover(steps):
    """N = 128, n_c = 1, B = 8.  One step is six phases (two basis changes, four stages), each through the
    hand-over; three steps also run stage 3 -> stage 0 across a step boundary."""
    _check(*inputs(128, 1, 8), steps, f"hand-over, {steps} step(s)")


def test_per_entry_edges():
    """rho0 = |i><i| for i at the edges of the K-tiles that travel through LDS (columns 15|16 and 31|32 of Y, rows
    15|16 of the state) and at the far corner: one matrix each, error per member."""
    from oracle import lindblad as olb
    H, cs, _ = inputs(128, 1, 1)
    idx = [0, 15, 16, 31, 32, 127]
    rho0 = np.zeros((len(idx), 128, 128), complex)
    for m, i in enumerate(idx):
        rho0[m, i, i] = 1.0
    r = _check(H, cs, rho0, 2, "unit populations")
    ref = olb.lindblad_batch(H, cs, rho0, DT, 2)
    errs = [relerr(r[m], ref[m]) for m in range(len(idx))]
    for i, e in zip(idx, errs):
        print(f"  rho0 = |{i}><{i}|: rel err {e:.3e}")
    assert max(errs) < TOL, dict(zip(idx, errs))


@pytest.mark.parametrize("N", [65, 113])
def test_padding(N):
    """n_c = 1 with the padding beginning inside tile 4 (N = 65) and inside tile 7 (N = 113): beyond the handed-over
    columns and rows, whose padded parts must stay exactly zero."""
    _check(*inputs(N, 1, 2), 2, f"padding, N = {N}")


@pytest.mark.parametrize("nc", [2, 3])
def test_lookahead_branch(nc):
    """n_c >= 2: no register hand-over; the last Y GEMM stages (Y_0, C~_0^+) tile 0 as an ordinary lookahead."""
    _check(*inputs(113, nc, 2), 3, f"lookahead branch, n_c = {nc}")


def test_observables_between_phases():
    """Two observables with t0: the observable pass runs between stage 3 and the next stage 0 (and behind the change
    of basis) and must leave the staging buffers and the state as they are."""
    from oracle import lindblad as olb
    H, cs, rho0 = inputs(113, 1, 2)
    rng = np.random.default_rng(12)
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
    # the same states without observables: the pass in between changes nothing
    assert np.array_equal(r, _run(H, cs, rho0, steps))


def test_step_count():
    """One 8-step call against its first and last four steps as two calls (each call changes basis twice, so not bit
    for bit): what the basis changes and the first and last stage hand over does not depend on the step count."""
    import torch
    from pyqed_amd import lindblad_rk4
    H, cs, rho0 = inputs(128, 1, 2)
    whole = _check(H, cs, rho0, 8, "8 steps")
    Ht, Ct, b, _ = _dev(H, cs, rho0)
    with qd_option("glf_path", "eig"):
        for _ in range(2):
            lindblad_rk4(Ht, Ct, b, DT, 4, hermitian=True)
        torch.cuda.synchronize()
    err = relerr(b.cpu().numpy(), whole)
    print(f"2 x 4 steps against 8 steps: rel err {err:.3e}")
    assert err < TOL_SELF
