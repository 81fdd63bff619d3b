"""The Lindblad batch kernel's stage epilogue (lindblad_rk4_kernel<128, true, true>): k = X + X^+ formed in the
registers of the wave that owns the upper tile (the waves publish their elements below the diagonal, conjugated, at
the mirror slot of one packed LDS image; one barrier; each upper element's owner adds the mirror and runs the Horner
update on it and on its mirror).  Small batches forced onto the persistent path; every case is held to the oracle's
RK4, to exact Hermiticity and to run-to-run bit equality.  tests/test_lindblad_kreg_inputs.py holds the same inputs
to a higher-accuracy reference on the CPU."""
import numpy as np
import pytest

from conftest import qd_option, relerr, took

pytestmark = pytest.mark.gpu

TOL = 1e-10        # the project's bound against the oracle (test_lindblad_gpu.py)
TOL_PERM = 1e-12   # permuted against unpermuted run (case 5)
DT = 1e-3

# case 5: the 16-blocks of the 128 rows and columns, permuted (no fixed block, not an involution)
BLOCK_PERM = (3, 6, 0, 5, 7, 1, 4, 2)


def inputs(N, nc, B):
    """H (GUE, complex Hermitian, non-zero diagonal), nc dense collapse operators, B pure states."""
    from oracle import lindblad as olb
    H, cs = olb.synthetic_lindblad(N, nc=max(nc, 1))
    return H, cs[:nc], olb.random_pure_states(B, N)


def inputs_complex_diagonal(N, B):
    """Case 4: H with a non-real off-diagonal part and a diagonal well away from zero; mixed states with every
    diagonal element non-zero."""
    H, cs, rho0 = inputs(N, 1, B)
    H = H + np.diag(np.linspace(-1.0, 1.0, N))
    rho0 = 0.5 * rho0 + 0.5 * np.eye(N) / N
    rho0 = (rho0 + rho0.conj().swapaxes(-1, -2)) / 2   # exactly Hermitian
    return H, cs, rho0


def block_permutation(N=128):
    return np.concatenate([np.arange(16 * b, 16 * b + 16) for b in BLOCK_PERM])


def permuted(H, cs, rho0, perm):
    """P H P^T, P C P^T, P rho P^T for the permutation matrix P of perm."""
    ix = np.ix_(perm, perm)
    return H[ix], [c[ix] for c in cs], np.ascontiguousarray(rho0[:, perm][:, :, perm])


# (name, builder, steps): the cases of this file and of the CPU check of their inputs
CASES = {
    "headline_1step": (lambda: inputs(128, 1, 2), 1),
    "headline_2steps": (lambda: inputs(128, 1, 2), 2),
    "padded_two_collapse": (lambda: inputs(113, 2, 3), 3),
    "no_collapse": (lambda: inputs(128, 0, 2), 3),
    "complex_diagonal": (lambda: inputs_complex_diagonal(128, 2), 3),
    "block_permutation": (lambda: inputs(128, 1, 2), 5),
}


def _run(H, cs, rho0, steps):
    """rho0 [B,N,N] through the persistent Hermitian kernel; returns rho as a NumPy array."""
    import torch
    from pyqed_amd import lindblad_rk4
    dev = torch.device("cuda", 0)
    Ht = torch.from_numpy(np.ascontiguousarray(H)).to(dev)
    Ct = torch.from_numpy(np.array(cs)).to(dev) if len(cs) else None
    rho = torch.from_numpy(np.ascontiguousarray(rho0).copy()).to(dev)
    took("")   # clear the path record
    with qd_option("glf_path", "persistent"):
        lindblad_rk4(Ht, Ct, rho, DT, steps, hermitian=True)
        torch.cuda.synchronize()
    ok, got = took("glf_persistent")
    assert ok, got
    return rho.cpu().numpy()


def _exactly_hermitian(r):
    return np.array_equal(r, r.conj().swapaxes(-1, -2))


def _check(name):
    """The three properties every case asserts: oracle, exact Hermiticity, two identical calls bit for bit."""
    from oracle import lindblad as olb
    build, steps = CASES[name]
    H, cs, rho0 = build()
    r = _run(H, cs, rho0, steps)
    r2 = _run(H, cs, rho0, steps)
    err = relerr(r, olb.lindblad_batch(H, cs, rho0, DT, steps))
    print(f"{name}: N={H.shape[0]} nc={len(cs)} B={len(rho0)} steps={steps}: rel err {err:.3e}")
    assert err < TOL
    assert _exactly_hermitian(r)
    assert np.array_equal(r, r2)
    return H, cs, rho0, r


def test_headline_one_step():
    """Case 1, one step: the four stages once; stage 3 updates rho in place from loads issued before its stores."""
    _check("headline_1step")


def test_headline_two_steps():
    """Case 1, two steps: step 2 reads what step 1's mirror stores wrote."""
    _check("headline_2steps")


def test_padded_two_collapse_operators():
    """Case 2, N = 113 padded to 128: the padding starts inside diagonal tile 7 and inside the last row and column
    tiles; two collapse operators, so two Y stores ahead of the X GEMM."""
    _check("padded_two_collapse")


def test_no_collapse_operators():
    """Case 3, n_c = 0: no Y GEMM, the X GEMM's own prologue."""
    _check("no_collapse")


def test_diagonal_exactly_real():
    """Case 4: k on the diagonal is v + conj(v), so a Hermitian rho keeps an exactly real diagonal."""
    H, cs, rho0, r = _check("complex_diagonal")
    assert np.abs(H.imag).max() > 0.01 and np.abs(np.diagonal(H)).min() > 0.0
    d = np.diagonal(r, axis1=-2, axis2=-1)
    assert np.all(d.imag == 0.0)
    assert np.all(d.real != 0.0)


def test_block_permutation():
    """Case 5: P rho P^T under P H P^T, P C P^T for a permutation of the 16-blocks, un-permuted, against the plain
    run.  The same sums in another K order and on other waves' tiles: a wrong mirror slot in one wave's tile role
    moves with the permutation."""
    H, cs, rho0, r = _check("block_permutation")
    steps = CASES["block_permutation"][1]
    perm = block_permutation()
    Hp, csp, rho0p = permuted(H, cs, rho0, perm)
    rp = _run(Hp, csp, rho0p, steps)
    assert _exactly_hermitian(rp)
    inv = np.argsort(perm)
    back = rp[:, inv][:, :, inv]
    err = relerr(back, r)
    print(f"block permutation: un-permuted against plain run, rel err {err:.3e}")
    assert err < TOL_PERM
