"""The Lindblad batch kernel's stage boundaries (lindblad_rk4_kernel<128, true, true>): one K-tile stream per stage
(each GEMM's last K-tile stages the next GEMM's tile 0, no barrier behind the Y stores) and the Horner update's rho
loads issued ahead of the barrier that publishes k.  Small batches forced onto the persistent path; every case is held
to the oracle's RK4, to exact Hermiticity and to run-to-run bit equality."""
import numpy as np
import pytest

from conftest import qd_option, relerr, took

pytestmark = pytest.mark.gpu

TOL = 1e-10   # the project's bound against the oracle (test_lindblad_gpu.py)


def _run(H, cs, rho0, dt, steps, e_ops=None, save_every=0):
    """rho0 [B,N,N] through the persistent Hermitian kernel; returns (rho, obs, snap) as NumPy arrays."""
    import torch
    from pyqed_amd import lindblad_rk4
    dev = torch.device("cuda", 0)
    Ht = torch.from_numpy(np.ascontiguousarray(H)).to(dev)
    Ct = torch.from_numpy(np.array(cs)).to(dev) if len(cs) else None
    Et = torch.from_numpy(np.array(e_ops)).to(dev) if e_ops is not None else None
    rho = torch.from_numpy(np.ascontiguousarray(rho0).copy()).to(dev)
    took("")   # clear the path record
    with qd_option("glf_path", "persistent"):
        obs, snap = lindblad_rk4(Ht, Ct, rho, dt, steps, e_ops=Et, save_every=save_every, hermitian=True)
        torch.cuda.synchronize()
    ok, got = took("glf_persistent")
    assert ok, got
    return (rho.cpu().numpy(), None if obs is None else obs.cpu().numpy(),
            None if snap is None else snap.cpu().numpy())


def _exactly_hermitian(r):
    return np.array_equal(r, r.conj().swapaxes(-1, -2))


def _check(N, nc, B, steps, dt=1e-3):
    """The three properties every case asserts: oracle, exact Hermiticity, two identical calls bit for bit."""
    from oracle import lindblad as olb
    H, cs = olb.synthetic_lindblad(N, nc=max(nc, 1))
    cs = cs[:nc]
    rho0 = olb.random_pure_states(B, N)
    r, _, _ = _run(H, cs, rho0, dt, steps)
    r2, _, _ = _run(H, cs, rho0, dt, steps)
    err = relerr(r, olb.lindblad_batch(H, cs, rho0, dt, steps))
    print(f"N={N} nc={nc} B={B} steps={steps}: rel err {err:.3e}")
    assert err < TOL
    assert _exactly_hermitian(r)
    assert np.array_equal(r, r2)


def test_headline_shape():
    """N = 128, one collapse operator: Y -> X lookahead, no barrier behind the Y store."""
    _check(128, 1, 2, 5)


def test_no_collapse_operators_keeps_the_x_prologue():
    """n_c = 0: no Y GEMM to stage the X GEMM's tile 0 under."""
    _check(128, 0, 2, 5)


def test_padded_three_collapse_operators():
    """N = 100 padded to 128, three collapse operators, three matrices: the Y_c -> Y_{c+1} -> X lookahead chain, and
    zero padding through the prefetched Horner update."""
    _check(100, 3, 3, 5)


def test_single_step():
    """nsteps = 1: one pass through the four stages, nothing carried over."""
    _check(128, 1, 2, 1)


def test_two_launches_equal_one():
    """3 + 4 steps as two launches against one 7-step launch, with observables and a snapshot per step: states,
    observables and snapshots agree bit for bit (no lookahead state may leak across a step or a launch boundary: a
    stage's stream starts cold and ends with the X GEMM), and all of them agree with the oracle."""
    from oracle import lindblad as olb
    N, B, dt = 128, 2, 1e-3
    H, cs = olb.synthetic_lindblad(N, nc=1)
    rho0 = olb.random_pure_states(B, N)
    e_ops = [np.eye(N, dtype=complex), H.astype(complex)]
    r7, obs7, snap7 = _run(H, cs, rho0, dt, 7, e_ops=e_ops, save_every=1)
    r3, obs3, snap3 = _run(H, cs, rho0, dt, 3, e_ops=e_ops, save_every=1)
    r4, obs4, snap4 = _run(H, cs, r3, dt, 4, e_ops=e_ops, save_every=1)
    r7b, obs7b, snap7b = _run(H, cs, rho0, dt, 7, e_ops=e_ops, save_every=1)
    assert snap7.shape == (B, 7, N, N) and obs7.shape == (B, 8, 2)
    assert np.array_equal(r4, r7)
    assert np.array_equal(np.concatenate([obs3, obs4[:, 1:]], axis=1), obs7)
    assert np.array_equal(obs3[:, -1], obs4[:, 0])
    assert np.array_equal(np.concatenate([snap3, snap4], axis=1), snap7)
    assert np.array_equal(snap7[:, -1], r7)
    assert np.array_equal(r7, r7b) and np.array_equal(obs7, obs7b) and np.array_equal(snap7, snap7b)
    assert _exactly_hermitian(r7) and _exactly_hermitian(snap7)
    errs = []
    for b in range(B):
        ref_obs, ref_list, ref_rho = olb.lindblad(H, rho0[b], cs, e_ops, 7, dt)
        errs += [relerr(r7[b], ref_rho), relerr(obs7[b], ref_obs)]
        errs += [relerr(snap7[b, s], ref_list[s]) for s in range(7)]
    print("3 + 4 steps: rel errs", " ".join(f"{e:.3e}" for e in errs))
    assert max(errs) < TOL
