"""The inputs of tests/test_lindblad_kreg_gpu.py on the CPU: the oracle's double-precision RK4 must itself stay well
inside the 1e-10 bound those tests hold the kernel to, against the same RK4 step in extended precision
(np.longdouble, 64-bit mantissa on x86) written in the generator form A r + r A^+ + sum_c C r C^+.  One batch member
per case: the members share every operator."""
import numpy as np
import pytest

from conftest import relerr
from test_lindblad_kreg_gpu import CASES, DT, TOL, block_permutation, permuted

LD = np.clongdouble


def _rk4_extended(H, cs, rho, dt, steps):
    H = np.asarray(H, LD)
    cs = [np.asarray(c, LD) for c in cs]
    A = -1j * H
    for c in cs:
        A = A - (c.conj().T @ c) / 2
    Ad = A.conj().T

    def rhs(r):
        out = A @ r + r @ Ad
        for c in cs:
            out = out + c @ r @ c.conj().T
        return out

    rho = np.asarray(rho, LD)
    dt = np.longdouble(dt)
    for _ in range(steps):
        k1 = rhs(rho)
        k2 = rhs(rho + k1 * (dt / 2))
        k3 = rhs(rho + k2 * (dt / 2))
        k4 = rhs(rho + k3 * dt)
        rho = rho + (k1 + 2 * k2 + 2 * k3 + k4) * (dt / 6)
    return rho


@pytest.mark.skipif(np.finfo(np.longdouble).nmant <= 52, reason="no extended precision on this platform")
@pytest.mark.parametrize("name", sorted(CASES))
def test_oracle_inside_bound(name):
    from oracle import lindblad as olb
    build, steps = CASES[name]
    H, cs, rho0 = build()
    if name == "block_permutation":
        H, cs, rho0 = permuted(H, cs, rho0, block_permutation())
    rho0 = rho0[:1]
    assert np.array_equal(rho0, rho0.conj().swapaxes(-1, -2))   # the Hermitian kernel's precondition
    ref = _rk4_extended(H, cs, rho0[0], DT, steps)
    got = olb.lindblad_batch(H, cs, rho0, DT, steps)[0]
    err = float(relerr(got.astype(LD), ref))
    print(f"{name}: oracle against extended precision, rel err {err:.3e}")
    assert err < TOL / 100
