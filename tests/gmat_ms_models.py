"""The coupled-surface curvilinear test model and a numpy restatement of its propagation, shared by the host and GPU
tests of the multi-state G-matrix propagator (test_gmat_ms_host.py, test_gmat_ms_gpu.py).

    i d psi_a / dt = K psi_a + sum_b V_ab(x, y) psi_b,    psi [nx, ny, ns], V [nx, ny, ns, ns]

Built on gmat_models: the same grid, metric and packet, gmat_models.keo_ref (fft2 form) per state, an einsum for the
potential and the classical four-slope RK4.  Like gmat_models it is deliberately NOT the arithmetic under test, which
holds the states as planes, takes one-dimensional transforms and sums V_ab y_b in a loop inside Horner-form RK4."""
import numpy as np

import gmat_models as gm


def model_ms(nx, ny, ns):
    """gmat_models.model with a complex Hermitian V [nx, ny, ns, ns]: distinct smooth diagonals (v, 0.8 v + 0.3,
    1.2 v - 0.2, then a_k v + b_k), Gaussian couplings with a phase between every pair of states, psi0 [nx, ny, ns]
    with the packet spread over the states (norm 1), and dt = 1 / lam with gmat_models' lam taking
    max_x ||V(x)||_2 in place of max |v|."""
    m = gm.model(nx, ny)
    X, Y = np.meshgrid(m["x"], m["y"], indexing="ij")
    v = m["v"]
    V = np.zeros((nx, ny, ns, ns), dtype=complex)
    scale = [1.0, 0.8, 1.2] + [1.0 + 0.1 * k for k in range(3, ns)]
    shift = [0.0, 0.3, -0.2] + [0.05 * k for k in range(3, ns)]
    for a in range(ns):
        V[..., a, a] = scale[a] * v + shift[a]
        for b in range(a + 1, ns):
            V[..., a, b] = 0.1 * (1.0 + 0.5j) / (b - a) * np.exp(-X ** 2 - Y ** 2)
            V[..., b, a] = np.conj(V[..., a, b])
    amp = np.array([1.0 / (1.0 + a) for a in range(ns)]) * np.exp(0.7j * np.arange(ns))
    psi0 = m["psi0"][..., None] * (amp / np.linalg.norm(amp))
    vmax = np.linalg.norm(V, ord=2, axis=(-2, -1)).max()
    lam = 1.0 / m["dt"] - np.abs(v).max() + vmax
    return dict(x=m["x"], y=m["y"], G=m["G"], V=V, v=v, psi0=psi0, kx=m["kx"], ky=m["ky"], dt=1.0 / lam, lam=lam)


def block_diagonal(V):
    """V with the couplings removed."""
    ns = V.shape[-1]
    return V * np.eye(ns)[None, None]


def hpsi_ms_ref(psi, kx, ky, V, G):
    """-i (K psi_a + sum_b V_ab psi_b), psi [nx, ny, ns]."""
    K = np.stack([gm.keo_ref(psi[..., a], kx, ky, G) for a in range(psi.shape[-1])], axis=-1)
    return -1j * (K + np.einsum("ijab,ijb->ija", V, psi))


def rk4_ms_ref(psi, dt, kx, ky, V, G):
    """One classical RK4 step, in gmat_models.rk4_ref's stage order."""
    k1 = hpsi_ms_ref(psi, kx, ky, V, G)
    k2 = hpsi_ms_ref(psi + k1 * (dt / 2.0), kx, ky, V, G)
    k3 = hpsi_ms_ref(psi + k2 * (dt / 2.0), kx, ky, V, G)
    k4 = hpsi_ms_ref(psi + k3 * dt, kx, ky, V, G)
    return psi + (k1 + 2 * k2 + 2 * k3 + k4) / 6.0 * dt


def run_ms_ref(psi0, dt, nt, kx, ky, V, G):
    """The states after steps 1 .. nt, [nt, nx, ny, ns]."""
    out, psi = [], np.array(psi0, dtype=complex)
    for _ in range(nt):
        psi = rk4_ms_ref(psi, dt, kx, ky, V, G)
        out.append(psi)
    return np.array(out)
