"""The jump-basis Lindblad path (qd_lindblad_rk4_eig_jump, lindblad_eig_jump_kernel in glf_eig_jump_kernel.hpp): ONE
collapse operator C = W diag(mu) W^-1, rho~ = W^-1 rho W^-+ propagated with d rho~/dt = X + X^+ + M o rho~,
X = A~ rho~, M_ij = mu_i conj(mu_j), and transformed back.  Small batches forced onto the path with glf_path
"eig_jump"; every case asserts the path note and is held to the oracle's RK4 at the project's bound, to exact
Hermiticity, to an exactly real diagonal and to bit equality of two identical calls.  The host plan is tested without
a GPU in test_lindblad_eig_jump_plan_cpu.py."""
import numpy as np
import pytest

from conftest import qd_option, relerr
from test_lindblad_kreg_gpu import BLOCK_PERM, block_permutation, inputs, inputs_complex_diagonal, permuted

pytestmark = pytest.mark.gpu

TOL = 1e-10        # the project's bound against the oracle
TOL_SELF = 1e-12   # one run of the path against another in a different order of the same sums
DT = 1e-3
PATH = "glf_eig_jump"


def _dev(H, cs, rho0, es=None):
    import torch
    dev = torch.device("cuda", 0)
    Ht = torch.from_numpy(np.ascontiguousarray(H)).to(dev)
    Ct = torch.from_numpy(np.ascontiguousarray(np.array(cs))).to(dev)
    rho = torch.from_numpy(np.ascontiguousarray(rho0).copy()).to(dev)
    Et = torch.from_numpy(np.ascontiguousarray(np.array(es))).to(dev) if es is not None else None
    return Ht, Ct, rho, Et


def _paths():
    from pyqed_amd import _lib
    return _lib.take_path().split()


def _run(H, cs, rho0, steps, want=PATH, es=None, path="eig_jump", **kw):
    """rho0 [B,N,N] through lindblad_rk4 under glf_path `path`; asserts that the kernel path `want` was taken, by its
    whole name ("glf_eig" is not "glf_eig_jump").  Returns rho (and the observables when es is given)."""
    import torch
    from pyqed_amd import lindblad_rk4
    Ht, Ct, rho, Et = _dev(H, cs, rho0, es)
    _paths()   # clear the path record
    with qd_option("glf_path", path):
        obs, _ = lindblad_rk4(Ht, Ct, rho, DT, steps, e_ops=Et, hermitian=True, **kw)
        torch.cuda.synchronize()
    got = _paths()
    assert want in got, got
    return (rho.cpu().numpy(), obs.cpu().numpy()) if es is not None else rho.cpu().numpy()


def _exactly_hermitian(r):
    return np.array_equal(r, r.conj().swapaxes(-1, -2))


def _check(H, cs, rho0, steps, name):
    """What every case asserts: oracle, exact Hermiticity, exactly real diagonal, two identical calls bit for bit."""
    from oracle import lindblad as olb
    r = _run(H, cs, rho0, steps)
    r2 = _run(H, cs, rho0, steps)
    err = relerr(r, olb.lindblad_batch(H, cs, rho0, DT, steps))
    print(f"{name}: N={H.shape[0]} B={len(rho0)} steps={steps}: rel err {err:.3e}")
    assert err < TOL
    assert _exactly_hermitian(r)
    assert np.all(np.diagonal(r, axis1=-2, axis2=-1).imag == 0.0)
    assert np.array_equal(r, r2)
    return r


@pytest.mark.parametrize("steps", [1, 2])
def test_headline_shape(steps):
    """N = 128: one step, and two steps (step 2 reads what step 1's mirror stores wrote)."""
    _check(*inputs(128, 1, 2), steps, f"headline {steps} step(s)")


def test_padded():
    """N = 113: the padding starts inside diagonal tile 7."""
    _check(*inputs(113, 1, 3), 3, "padded")


def test_almost_all_padding():
    _check(*inputs(65, 1, 2), 2, "N = 65")


def test_hermitian_degenerate_collapse_operator():
    """A Hermitian C with a +-1 spectrum: the plan goes through eigh (W unitary) and mu is real."""
    H, _, rho0 = inputs(128, 1, 2)
    rng = np.random.default_rng(3)
    Q = np.linalg.qr(rng.standard_normal((128, 128)) + 1j * rng.standard_normal((128, 128)))[0]
    C = (Q * np.where(np.arange(128) % 2, 1.0, -1.0)) @ Q.conj().T * 0.1
    C = (C + C.conj().T) / 2
    _check(H, [C], rho0, 3, "Hermitian degenerate C")


def test_diagonal_exactly_real():
    """Mixed states under an H with a complex off-diagonal part and a non-zero diagonal: the diagonal of the result is
    exactly real and non-zero."""
    H, cs, rho0 = inputs_complex_diagonal(128, 2)
    r = _check(H, cs, rho0, 3, "complex diagonal")
    assert np.abs(H.imag).max() > 0.01 and np.abs(np.diagonal(H)).min() > 0.0
    assert np.all(np.diagonal(r, axis1=-2, axis2=-1).real != 0.0)


def test_block_permutation():
    """P rho P^T under P H P^T, P C P^T for a permutation of the 16-blocks, un-permuted, against the plain run: the
    same sums on other waves' tiles, so a wrong mirror address in one wave's tile role moves with the permutation."""
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


def test_observables_with_t0():
    """Two e_ops at N = 113, taken on rho~ with E~ = W^+ E W: every row, t0 included, against the oracle."""
    from oracle import lindblad as olb
    H, cs, rho0 = inputs(113, 1, 2)
    rng = np.random.default_rng(11)
    es = [np.eye(113, dtype=complex), (lambda a: a + a.conj().T)(rng.standard_normal((113, 113)) + 1j *
                                                                  rng.standard_normal((113, 113)))]
    steps = 3
    r, obs = _run(H, cs, rho0, steps, es=es)
    assert obs.shape == (2, steps + 1, 2)
    for b in range(2):
        ref_obs, _, ref_rho = olb.lindblad(H, rho0[b], cs, es, steps, DT, keep_states=False)
        ref_obs = np.asarray(ref_obs).reshape(steps + 1, 2)
        assert relerr(obs[b], ref_obs) < TOL, (b, obs[b], ref_obs)
        assert relerr(r[b], ref_rho) < TOL


def test_one_call_against_four():
    """One 20-step call against four 5-step calls: each call changes basis twice, so not bit for bit."""
    import torch
    from pyqed_amd import lindblad_rk4
    H, cs, rho0 = inputs(128, 1, 2)
    Ht, Ct, a, _ = _dev(H, cs, rho0)
    b = a.clone()
    _paths()
    with qd_option("glf_path", "eig_jump"):
        lindblad_rk4(Ht, Ct, a, DT, 20, hermitian=True)
        for _ in range(4):
            lindblad_rk4(Ht, Ct, b, DT, 5, hermitian=True)
        torch.cuda.synchronize()
    assert _paths() == [PATH] * 5
    err = relerr(b.cpu().numpy(), a.cpu().numpy())
    print(f"4 x 5 steps against 20 steps: rel err {err:.3e}")
    assert err < TOL_SELF


def _lowering(N):
    return [np.diag(np.sqrt(np.arange(1.0, N)), 1).astype(complex) * 0.05]


@pytest.mark.parametrize("B,nc,want", [(208, 1, PATH), (207, 1, "glf_split_pairs"), (208, 2, "glf_eig")])
def test_auto_dispatch(B, nc, want):
    """Under auto the jump basis is taken where the eigenbasis gate holds and there is one collapse operator; two
    collapse operators stay on the A basis, and below 208 matrices the pair-block split path runs."""
    from oracle import lindblad as olb
    H, cs, rho0 = inputs(128, nc, B)
    r = _run(H, cs, rho0, 2, want=want, path="auto")
    sel = [0, B - 1]
    assert relerr(r[sel], olb.lindblad_batch(H, cs, rho0[sel], DT, 2)) < TOL
    assert _exactly_hermitian(r)


def test_auto_dispatch_lowering_operator():
    """A lowering operator is defective: the jump plan is refused and the call runs elsewhere, within the bound."""
    import torch
    from oracle import lindblad as olb
    from pyqed_amd import lindblad_rk4
    B = 208
    H, _, rho0 = inputs(128, 1, B)
    cs = _lowering(128)
    Ht, Ct, rho, _ = _dev(H, cs, rho0)
    _paths()
    lindblad_rk4(Ht, Ct, rho, DT, 2, hermitian=True)
    torch.cuda.synchronize()
    got = _paths()
    assert got and PATH not in got, got
    sel = [0, B - 1]
    assert relerr(rho.cpu().numpy()[sel], olb.lindblad_batch(H, cs, rho0[sel], DT, 2)) < TOL


def test_forced_but_ineligible_raises():
    import torch
    from pyqed_amd import lindblad_rk4
    H, cs, rho0 = inputs(128, 2, 2)
    Ht, Ct, rho, _ = _dev(H, cs, rho0)
    with qd_option("glf_path", "eig_jump"):
        with pytest.raises(ValueError):
            lindblad_rk4(Ht, Ct, rho, DT, 1, hermitian=True)
    torch.cuda.synchronize()


def test_graph_capture_warm_and_cold_plan():
    """Captured with a cached plan, two replays equal two direct calls bit for bit; captured with a plan not yet
    built (capture allows no host work) the call completes on another path within the bound."""
    import torch
    from oracle import lindblad as olb
    from pyqed_amd import lindblad_rk4
    H, cs, rho0 = inputs(128, 1, 2)
    Ht, Ct, r0, _ = _dev(H, cs, rho0)
    s = torch.cuda.Stream(torch.device("cuda", 0))
    with qd_option("glf_path", "eig_jump"):
        ref = r0.clone()
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            for _ in range(2):
                lindblad_rk4(Ht, Ct, ref, DT, 3, hermitian=True, stream=s.cuda_stream)   # builds and caches the plan
        torch.cuda.synchronize()
        x = r0.clone()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        _paths()
        with torch.cuda.graph(g, stream=s):
            lindblad_rk4(Ht, Ct, x, DT, 3, hermitian=True, stream=s.cuda_stream)
        assert PATH in _paths()
        x.copy_(r0)
        g.replay()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(x, ref)
        # cold: the same collapse operator in a new tensor, first seen while capturing (H keeps its cached
        # Hermiticity check, which is host work as well)
        Cc = Ct.clone()
        y = r0.clone()
        torch.cuda.synchronize()
        g2 = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g2, stream=s):
            lindblad_rk4(Ht, Cc, y, DT, 3, hermitian=True, stream=s.cuda_stream)
        taken = _paths()
        assert taken and PATH not in taken and "glf_eig" not in taken, taken
        y.copy_(r0)
        g2.replay()
        torch.cuda.synchronize()
    assert relerr(y.cpu().numpy(), olb.lindblad_batch(H, cs, rho0, DT, 3)) < TOL
