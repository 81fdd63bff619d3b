"""The three-dimensional curvilinear test model and a numpy restatement of its propagation, shared by the host and GPU
tests of the 3 x 3 G-matrix propagator (test_gmat3_host.py, test_gmat3_gpu.py) and by tools/wp_gmat3_bench.py.

    i d psi_a / dt = 1/2 sum_rs p_r G_rs(x, y, z) p_s psi_a + sum_b V_ab(x, y, z) psi_b

The restatement is written the way the reference computes in two dimensions (gmat_models.py): n-dimensional transforms
for every derivative, an einsum for the metric and the potential, and the classical four-slope RK4.  It is
deliberately NOT the arithmetic under test, which takes one-dimensional transforms along each axis with 1/n folded
into the k tables, holds the states as planes and runs RK4 in Horner form; emulate_* below is that arithmetic in numpy
(the host tests hold it against the restatement)."""
import numpy as np
from scipy.fftpack import fftfreq

SPAN = (12.0, 10.0, 8.0)   # x in [-6, 6), y in [-5, 5), z in [-4, 4)


def model3(nx, ny, nz, ns=1):
    """A smooth metric whose nine entries all differ, with G_rs != G_sr, so a swap of any two shows; a real potential
    v [nx, ny, nz] and the coupled V [nx, ny, nz, ns, ns] (complex Hermitian; V[..., 0, 0] = v); a Gaussian packet with
    momentum along all three axes, psi0 [nx, ny, nz] for ns = 1, else [nx, ny, nz, ns] spread over the states; and
    dt = 1 / lam with
        lam = 1/2 sum_rs max |G_rs| k_r,max k_s,max + max_p ||V(p)||_2,
    a bound on ||H||: dt ||H|| <= 1 keeps every shape inside RK4's stability region.  k = 2 pi fftfreq(n, d), which is
    zeros(1) for an axis of length 1."""
    n = (nx, ny, nz)
    d = [s / m for s, m in zip(SPAN, n)]
    x, y, z = (-s / 2.0 + h * np.arange(m) for s, h, m in zip(SPAN, d, n))
    X, Y, Z = np.meshgrid(x, y, z, indexing="ij")
    cx, cy, cz = (2 * np.pi * A / s for A, s in zip((X, Y, Z), SPAN))
    G = np.empty(n + (3, 3))
    G[..., 0, 0] = 1.0 + 0.3 * np.exp(-X ** 2 / 8.0)
    G[..., 1, 1] = 0.8 + 0.2 * np.cos(cy)
    G[..., 2, 2] = 0.9 + 0.15 * np.cos(cz) * np.cos(cx)
    G[..., 0, 1] = 0.15 * np.sin(cx) * np.cos(cy)
    G[..., 1, 0] = 0.05 - 0.1 * np.cos(cx)
    G[..., 0, 2] = 0.12 * np.cos(cz) + 0.02
    G[..., 2, 0] = -0.07 * np.sin(cy) * np.sin(cz) + 0.03
    G[..., 1, 2] = 0.09 * np.sin(cz) * np.cos(cx) - 0.04
    G[..., 2, 1] = 0.06 + 0.05 * np.cos(cy) * np.cos(cz)
    v = 0.15 * X ** 2 + 0.1 * Y ** 2 + 0.12 * Z ** 2 + 0.05 * X * Y - 0.03 * Y * Z
    psi0 = np.exp(-((X + 1.0) ** 2 + (Y - 0.5) ** 2 + (Z + 0.3) ** 2) / 2.0 + 0.6j * X - 0.4j * Y + 0.5j * Z)
    psi0 = psi0.astype(complex) / np.linalg.norm(psi0)
    V = np.zeros(n + (ns, ns), dtype=complex)
    for a in range(ns):
        V[..., a, a] = (1.0 + 0.2 * (-1) ** a * a / ns) * v + 0.3 * a
        for b in range(a + 1, ns):
            V[..., a, b] = 0.1 * (1.0 + 0.5j) / (b - a) * np.exp(-X ** 2 - Y ** 2 - Z ** 2)
            V[..., b, a] = np.conj(V[..., a, b])
    if ns > 1:
        amp = np.array([1.0 / (1.0 + a) for a in range(ns)]) * np.exp(0.7j * np.arange(ns))
        psi0 = psi0[..., None] * (amp / np.linalg.norm(amp))
    ks = [2.0 * np.pi * fftfreq(m, h) for m, h in zip(n, d)]
    km = [np.abs(k).max() for k in ks]
    lam = 0.5 * sum(np.abs(G[..., r, s]).max() * km[r] * km[s] for r in range(3) for s in range(3)) \
        + np.linalg.norm(V, ord=2, axis=(-2, -1)).max()
    return dict(x=x, y=y, z=z, G=G, v=v, V=V, psi0=psi0, kx=ks[0], ky=ks[1], kz=ks[2], ks=ks, dt=1.0 / lam, lam=lam)


def block_diagonal(V):
    """V with the couplings removed."""
    return V * np.eye(V.shape[-1])


def _momentum(f, k, axis):
    """ifftn(k fftn f) with k along `axis`, as the reference forms every derivative."""
    kk = k.reshape([-1 if a == axis else 1 for a in range(3)])
    return np.fft.ifftn(kk * np.fft.fftn(f))


def keo3_ref(psi, ks, G):
    """K psi of one state [nx, ny, nz]."""
    grad = np.stack([_momentum(psi, ks[a], a) for a in range(3)], axis=-1)
    phi = np.einsum("ijkrs,ijks->ijkr", G, grad)
    return 0.5 * sum(_momentum(phi[..., a], ks[a], a) for a in range(3))


def hpsi3_ref(psi, ks, v, G):
    """-i (K + v) psi: psi [nx, ny, nz] with v [nx, ny, nz] (or None), or psi [nx, ny, nz, ns] with
    v [nx, ny, nz, ns, ns]."""
    if v is not None and np.ndim(v) == 5:
        K = np.stack([keo3_ref(psi[..., a], ks, G) for a in range(psi.shape[-1])], axis=-1)
        return -1j * (K + np.einsum("ijkab,ijkb->ijka", v, psi))
    return -1j * (keo3_ref(psi, ks, G) + (0.0 if v is None else v * psi))


def rk4_ref(psi, dt, ks, v, G):
    """One classical RK4 step in the reference's stage order (four slopes, then the weighted sum)."""
    k1 = hpsi3_ref(psi, ks, v, G)
    k2 = hpsi3_ref(psi + k1 * (dt / 2.0), ks, v, G)
    k3 = hpsi3_ref(psi + k2 * (dt / 2.0), ks, v, G)
    k4 = hpsi3_ref(psi + k3 * dt, ks, v, G)
    return psi + (k1 + 2 * k2 + 2 * k3 + k4) / 6.0 * dt


def run_ref(psi0, dt, nt, ks, v, G):
    """The states after steps 1 .. nt."""
    out, psi = [], np.array(psi0, dtype=complex)
    for _ in range(nt):
        psi = rk4_ref(psi, dt, ks, v, G)
        out.append(psi)
    return np.array(out)


# ---------------------------------------------------------------- the kernels' arithmetic in numpy
def _deriv(f, k, axis):
    """IFFT_a((k / n) FFT_a f) with unnormalised one-dimensional transforms."""
    n = f.shape[axis]
    kk = (k / n).reshape([-1 if a == axis else 1 for a in range(3)])
    return np.fft.ifft(kk * np.fft.fft(f, axis=axis), axis=axis) * n


def emulate_h(y, ks, v, G):
    """(K + v) y of planes y [ns, nx, ny, nz] with v [ns, ns, nx, ny, nz] or None: phi_r summed with s ascending,
    the kinetic half as (D_x phi_x + D_y phi_y) + D_z phi_z, sum_b V_ab y_b with b ascending and added last."""
    out = np.empty_like(y)
    for a in range(len(y)):
        d = [_deriv(y[a], ks[s], s) for s in range(3)]
        phi = [(G[..., r, 0] * d[0] + G[..., r, 1] * d[1]) + G[..., r, 2] * d[2] for r in range(3)]
        h = 0.5 * ((_deriv(phi[0], ks[0], 0) + _deriv(phi[1], ks[1], 1)) + _deriv(phi[2], ks[2], 2))
        if v is not None:
            vy = v[a, 0] * y[0]
            for b in range(1, len(y)):
                vy = vy + v[a, b] * y[b]
            h = h + vy
        out[a] = h
    return out


def emulate_run(psi0, dt, nt, ks, v, G):
    """Horner-form RK4, y_{s+1} = psi - i c_s H y_s with c = dt/4, dt/3, dt/2, dt: the states after steps 1 .. nt,
    planes [nt, ns, nx, ny, nz]."""
    out, psi = [], np.array(psi0, dtype=complex)
    for _ in range(nt):
        y = psi
        for c in (dt * 0.25, dt / 3.0, dt * 0.5, dt):
            y = psi - 1j * c * emulate_h(y, ks, v, G)
        psi = y
        out.append(psi)
    return np.array(out)


def taylor_run(psi0, dt, nt, ks, G0):
    """nt RK4 steps under a constant metric G0 [3, 3] and v = 0 in closed form: ifftn(R(-i dt E_k)^nt fftn psi0),
    E_k = 1/2 sum_rs G0_rs k_r k_s, R the degree-4 Taylor polynomial of exp."""
    K = np.meshgrid(*ks, indexing="ij")
    E = 0.5 * sum(G0[r, s] * K[r] * K[s] for r in range(3) for s in range(3))
    zz = -1j * dt * E
    R = 1.0 + zz * (1.0 + zz / 2.0 * (1.0 + zz / 3.0 * (1.0 + zz / 4.0)))
    return np.fft.ifftn(R ** nt * np.fft.fftn(psi0))
