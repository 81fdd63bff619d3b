"""lindblad_eig_jump_kernel with k = X + X^+ formed inside the GEMM on the tiles on and above the diagonal
(glf_eig_jump_kernel.hpp; the schedule in NumPy: test_lindblad_eig_jump_fused_cpu.py): the two sums alone, the
elementwise term alone, every wave's tile roles one block pair at a time, the hand-over of rn through L.b[0] / L.b[1]
and the lookahead across passes and calls, and the observables at every batch size below four.  Helpers and bounds
are test_lindblad_eig_jump_gpu.py's."""
import numpy as np
import pytest

from conftest import qd_option, relerr
from test_lindblad_eig_jump_gpu import DT, PATH, TOL, TOL_SELF, _check, _dev, _exactly_hermitian, _paths, _run
from test_lindblad_kreg_gpu import inputs

pytestmark = pytest.mark.gpu


def _hermitian_full(N, seed):
    """A complex Hermitian H, every 16-block dense, scaled like the synthetic one."""
    rng = np.random.default_rng(seed)
    a = rng.standard_normal((N, N)) + 1j * rng.standard_normal((N, N))
    return (a + a.conj().T) / np.sqrt(8 * N)


@pytest.mark.parametrize("steps", [1, 2])
@pytest.mark.parametrize("N", [128, 65])
def test_two_sums_alone(N, steps):
    """C = 0: W = I and mu = 0, so a stage is the first and the swapped sums alone; N = 65 pads from inside tile 4."""
    _, _, rho0 = inputs(N, 1, 2)
    H = _hermitian_full(N, 21)
    assert np.abs(H[:16, -16:]).min() > 0 and np.abs(H.imag).max() > 0.01
    _check(H, [np.zeros((N, N), complex)], rho0, steps, f"C = 0, N = {N}")


def test_elementwise_term_alone():
    """H = 0 and a real diagonal C: A~ is diagonal and the stage is M o r and a diagonal product; bitwise Hermitian, the
    diagonal exactly real."""
    N = 128
    _, _, rho0 = inputs(N, 1, 3)
    C = np.diag(np.linspace(-0.3, 0.4, N)).astype(complex)
    r = _check(np.zeros((N, N), complex), [C], rho0, 3, "H = 0, diagonal C")
    assert _exactly_hermitian(r)
    assert np.all(np.diagonal(r, axis1=-2, axis2=-1).imag == 0.0)


def _block_state(N, R, C, rng):
    """Hermitian, supported on the 16-block pair (R, C), (C, R) and on the diagonal block (R, R)."""
    rho = np.zeros((N, N), complex)
    rs, cs = slice(16 * R, 16 * R + 16), slice(16 * C, 16 * C + 16)
    g = rng.standard_normal((16, 16)) + 1j * rng.standard_normal((16, 16))
    d = rng.standard_normal((16, 16)) + 1j * rng.standard_normal((16, 16))
    rho[rs, cs] = g
    rho[cs, rs] = g.conj().T
    rho[rs, rs] = d + d.conj().T
    return rho / 16


def test_every_block_pair():
    """A state on one block pair (R, C) and one diagonal block, for every R <= C, three pairs to a call: each wave's
    role, the diagonal dagger and the mirror stores, two steps against the oracle."""
    import torch
    from oracle import lindblad as olb
    from pyqed_amd import lindblad_rk4
    N, steps = 128, 2
    H, cs, _ = inputs(N, 1, 1)
    Ht, Ct, _, _ = _dev(H, cs, np.zeros((1, N, N), complex))
    rng = np.random.default_rng(17)
    pairs = [(R, C) for R in range(8) for C in range(R, 8)]
    assert len(pairs) == 36
    worst = 0.0
    with qd_option("glf_path", "eig_jump"):
        for i in range(0, 36, 3):
            rho0 = np.array([_block_state(N, R, C, rng) for R, C in pairs[i:i + 3]])
            rho = torch.from_numpy(rho0.copy()).to(Ht.device)
            _paths()
            lindblad_rk4(Ht, Ct, rho, DT, steps, hermitian=True)
            torch.cuda.synchronize()
            assert PATH in _paths()
            got = rho.cpu().numpy()
            ref = olb.lindblad_batch(H, cs, rho0, DT, steps)
            for b in range(3):
                err = relerr(got[b], ref[b])
                worst = max(worst, err)
                assert err < TOL, (pairs[i + b], err)
            assert _exactly_hermitian(got)
            assert np.all(np.diagonal(got, axis1=-2, axis2=-1).imag == 0.0)
    print(f"36 block pairs, {steps} steps: worst rel err {worst:.3e}")


def _calls(H, cs, rho0, plan):
    """rho0 through the calls of `plan` (steps per call), one after the other on one tensor."""
    import torch
    from pyqed_amd import lindblad_rk4
    Ht, Ct, rho, _ = _dev(H, cs, rho0)
    _paths()
    with qd_option("glf_path", "eig_jump"):
        for n in plan:
            lindblad_rk4(Ht, Ct, rho, DT, n, hermitian=True)
        torch.cuda.synchronize()
    assert _paths() == [PATH] * len(plan)
    return rho.cpu().numpy()


@pytest.mark.parametrize("split,whole", [((1, 1), 2), ((5, 5, 5, 5), 20)])
def test_calls_against_one_call(split, whole):
    """1 + 1 steps against 2 and 4 x 5 against 20: what a stage hands the next one through L.b[0], L.b[1] and the
    lookahead is what a call's first stage reads cold; each call changes basis twice, so not bit for bit."""
    H, cs, rho0 = inputs(128, 1, 2)
    err = relerr(_calls(H, cs, rho0, split), _calls(H, cs, rho0, (whole,)))
    print(f"{split} against {whole} steps: rel err {err:.3e}")
    assert err < TOL_SELF


@pytest.mark.parametrize("B", [1, 2, 3])
def test_batch_sizes_with_observables(B):
    """B = 1, 2, 3 with two e_ops at t0 and behind every step: a pass whose result the observables read ends in a
    full barrier and still hands its rows on."""
    from oracle import lindblad as olb
    N, steps = 128, 3
    H, cs, rho0 = inputs(N, 1, B)
    rng = np.random.default_rng(11)
    a = rng.standard_normal((N, N)) + 1j * rng.standard_normal((N, N))
    es = [np.eye(N, dtype=complex), a + a.conj().T]
    r, obs = _run(H, cs, rho0, steps, es=es)
    assert obs.shape == (B, steps + 1, 2)
    for b in range(B):
        ref_obs, _, ref_rho = olb.lindblad(H, rho0[b], cs, es, steps, DT, keep_states=False)
        assert relerr(obs[b], np.asarray(ref_obs).reshape(steps + 1, 2)) < TOL, b
        assert relerr(r[b], ref_rho) < TOL, b
    assert _exactly_hermitian(r)


def test_last_stage_leaves_zero_elementwise_term():
    """A stage's elementwise term M o r is what the tail of the pass before left in the accumulators; the k pass of a
    basis change must start from zero (the last stage leaves zero, and a Y pass zeroes behind its stores).  One step,
    whose last stage is the call's last, with a collapse operator four times the usual, where a carried term would be
    far outside the bound; and two such calls in a row against the oracle's two steps."""
    from oracle import lindblad as olb
    H, cs, rho0 = inputs(128, 1, 2)
    cs = [4.0 * cs[0]]
    _check(H, cs, rho0, 1, "strong C, 1 step")
    err = relerr(_calls(H, cs, rho0, (1, 1)), olb.lindblad_batch(H, cs, rho0, DT, 2))
    print(f"strong C, 1 + 1 steps against the oracle: rel err {err:.3e}")
    assert err < TOL
