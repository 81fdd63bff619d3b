"""The Lindblad batch kernel (lindblad_rk4_kernel<128, true, true>: direct global -> LDS operand staging, optional
3-product complex MACs) against the oracle's RK4, on small batches forced onto the persistent path."""
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
    rho = torch.from_numpy(rho0.copy()).to(dev)
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


def test_headline_instantiation_matches_oracle():
    """N = 128 (no padding), one collapse operator: segment 0 and one Hermitian segment."""
    from oracle import lindblad as olb
    N, B, steps, dt = 128, 2, 5, 1e-3
    H, cs = olb.synthetic_lindblad(N, nc=1)
    rho0 = olb.random_pure_states(B, N)
    r, _, _ = _run(H, cs, rho0, dt, steps)
    err = relerr(r, olb.lindblad_batch(H, cs, rho0, dt, steps))
    print(f"N=128 nc=1 B=2: rel err {err:.3e}")
    assert err < TOL
    assert _exactly_hermitian(r)


def test_padded_three_collapse_operators_matches_oracle():
    """N = 100 padded to 128 (zero rows and columns through the swizzled staging), three Hermitian segments, a batch
    that is no power of two.  The library hands back the N x N part only, so the padding itself is not visible."""
    from oracle import lindblad as olb
    N, B, steps, dt = 100, 3, 5, 1e-3
    H, cs = olb.synthetic_lindblad(N, nc=3)
    rho0 = olb.random_pure_states(B, N)
    r, _, _ = _run(H, cs, rho0, dt, steps)
    err = relerr(r, olb.lindblad_batch(H, cs, rho0, dt, steps))
    print(f"N=100 nc=3 B=3: rel err {err:.3e}")
    assert err < TOL
    assert _exactly_hermitian(r)


def test_long_run_observables_and_snapshots():
    """200 steps at dt = 1e-2 with observables and snapshots: both agree with the oracle, and the last snapshot is the
    final state bit for bit."""
    from oracle import lindblad as olb
    N, steps, dt, every = 128, 200, 1e-2, 50
    H, cs = olb.synthetic_lindblad(N, nc=1)
    rho0 = olb.random_pure_states(1, N)
    e_ops = [np.eye(N, dtype=complex), H.astype(complex)]
    r, obs, snap = _run(H, cs, rho0, dt, steps, e_ops=e_ops, save_every=every)
    ref_obs, ref_list, ref_rho = olb.lindblad(H, rho0[0], cs, e_ops, steps, dt)
    errs = [relerr(r[0], ref_rho), relerr(obs[0], ref_obs)]
    assert snap.shape == (1, steps // every, N, N)
    for s in range(steps // every):
        errs.append(relerr(snap[0, s], ref_list[every * (s + 1) - 1]))
    print("long run: rel errs", " ".join(f"{e:.3e}" for e in errs))
    assert max(errs) < TOL
    assert np.max(np.abs(obs[0, :, 0] - 1.0)) < 1e-12   # trace
    assert np.array_equal(snap[0, -1], r[0])
    assert _exactly_hermitian(r)
    assert _exactly_hermitian(snap)


def test_no_collapse_operators_matches_oracle():
    """n_c = 0: the X GEMM is segment 0 alone (no Y GEMM, no Hermitian segment)."""
    from oracle import lindblad as olb
    N, B, steps, dt = 128, 2, 5, 1e-3
    H, _ = olb.synthetic_lindblad(N, nc=1)
    rho0 = olb.random_pure_states(B, N)
    r, _, _ = _run(H, [], rho0, dt, steps)
    err = relerr(r, olb.lindblad_batch(H, [], rho0, dt, steps))
    print(f"N=128 nc=0 B=2: rel err {err:.3e}")
    assert err < TOL
    assert _exactly_hermitian(r)
