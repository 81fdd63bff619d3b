"""The curvilinear test model and a numpy restatement of the reference's curvilinear propagation, shared by the host
and GPU tests of the G-matrix kinetic operator (test_gmat_host.py, test_gmat_gpu.py) and by the fixture generator
(golden/make_golden_gmat.py).

The restatement is written the way the reference computes (pyqed/wpd.py:1861-1940 KEO / PEO / hpsi, phys.py:1051-1064
rk4): two-dimensional transforms for every derivative and the classical four-slope RK4.  It is deliberately NOT the
arithmetic under test, which takes one-dimensional transforms along each axis and RK4 in Horner form; the two agree
to rounding (a few 1e-16 relative on these models)."""
import numpy as np
from scipy.fftpack import fftfreq


def model(nx, ny):
    """x in [-6, 6), y in [-5, 5); a smooth metric with Gxy != Gyx (so a swap of the two shows), a real potential,
    a Gaussian packet with momentum along both axes, and dt = 1 / lam with
        lam = 1/2 (max Gxx kx_max^2 + max Gyy ky_max^2 + max(|Gxy| + |Gyx|) kx_max ky_max) + max |v|,
    a bound on ||H||: dt ||H|| <= 1 keeps every shape inside RK4's stability region."""
    dx, dy = 12.0 / nx, 10.0 / ny
    x = -6.0 + dx * np.arange(nx)
    y = -5.0 + dy * np.arange(ny)
    X, Y = np.meshgrid(x, y, indexing="ij")
    G = np.empty((nx, ny, 2, 2))
    G[..., 0, 0] = 1.0 + 0.3 * np.exp(-X ** 2 / 8.0)
    G[..., 1, 1] = 0.8 + 0.2 * np.cos(2 * np.pi * Y / 10.0)
    G[..., 0, 1] = 0.15 * np.sin(2 * np.pi * X / 12.0) * np.cos(2 * np.pi * Y / 10.0)
    G[..., 1, 0] = 0.05 - 0.1 * np.cos(2 * np.pi * X / 12.0)
    v = 0.15 * X ** 2 + 0.1 * Y ** 2 + 0.05 * X * Y
    psi0 = np.exp(-((X + 1.0) ** 2 + (Y - 0.5) ** 2) / 2.0 + 0.6j * X - 0.4j * Y).astype(complex)
    psi0 /= np.linalg.norm(psi0)
    kx = 2.0 * np.pi * fftfreq(nx, dx)
    ky = 2.0 * np.pi * fftfreq(ny, dy)
    kxm, kym = np.abs(kx).max(), np.abs(ky).max()
    lam = 0.5 * (G[..., 0, 0].max() * kxm ** 2 + G[..., 1, 1].max() * kym ** 2
                 + (np.abs(G[..., 0, 1]) + np.abs(G[..., 1, 0])).max() * kxm * kym) + np.abs(v).max()
    return dict(x=x, y=y, G=G, v=v, psi0=psi0, kx=kx, ky=ky, dt=1.0 / lam)


def _momentum(f, k, axis):
    """ifft2(k fft2 f) with k along `axis`, as the reference forms every derivative."""
    kk = k[:, None] if axis == 0 else k[None, :]
    return np.fft.ifft2(kk * np.fft.fft2(f))


def keo_ref(psi, kx, ky, G):
    grad = np.stack([_momentum(psi, kx, 0), _momentum(psi, ky, 1)], axis=-1)
    phi = np.einsum("ijrs,ijs->ijr", G, grad)
    return 0.5 * (_momentum(phi[..., 0], kx, 0) + _momentum(phi[..., 1], ky, 1))


def hpsi_ref(psi, kx, ky, v, G):
    return -1j * (keo_ref(psi, kx, ky, G) + v * psi)


def rk4_ref(psi, dt, kx, ky, v, G):
    """One classical RK4 step in the reference's stage order (four slopes, then the weighted sum)."""
    k1 = hpsi_ref(psi, kx, ky, v, G)
    k2 = hpsi_ref(psi + k1 * (dt / 2.0), kx, ky, v, G)
    k3 = hpsi_ref(psi + k2 * (dt / 2.0), kx, ky, v, G)
    k4 = hpsi_ref(psi + k3 * dt, kx, ky, v, G)
    return psi + (k1 + 2 * k2 + 2 * k3 + k4) / 6.0 * dt


def run_ref(psi0, dt, nt, kx, ky, v, G):
    """The states after steps 1 .. nt, [nt, nx, ny]."""
    out, psi = [], np.array(psi0, dtype=complex)
    for _ in range(nt):
        psi = rk4_ref(psi, dt, kx, ky, v, G)
        out.append(psi)
    return np.array(out)
