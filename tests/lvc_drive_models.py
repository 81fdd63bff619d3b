"""Helpers of the driven LVC tests (no test here): qd_lvc_driven_rk4 of include/qdyn.h restated in numpy on top of
lvc_models.apply, with the working precision as a parameter.

    H(t) = H0 - sum_d f_d(t) mu_d,  mu_d = A_d (x) 1 (mode -1) or A_d (x) x_j (mode j)

is the LVC Hamiltonian with the tables Hel - sum_{d: -1} f_d A_d and W[j] - sum_{d: j} f_d A_d (eff_tables, the drives
subtracted in the order d = 0, 1, ..).  sample "hold": step s takes row s // hold of fvals and is the Horner step of
lvc_models.rk4; "stage": classical RK4, the stages of step s take rows 2s, 2s + 1, 2s + 1, 2s + 2 and
psi' = ((psi + dt/6 k1) + dt/3 k2 + dt/3 k3) + dt/6 k4.  dense_mu assembles mu_d from explicit Kronecker products, for
the dense propagation tests/test_lvc_drive_host.py checks the restatement against."""
from __future__ import annotations

import numpy as np

import lvc_models as lm


def random_drives(nel, dims, modes, nf, seed=2):
    """A [nd, nel, nel] and fvals [nf, nd], dense random complex (nothing Hermitian, no real field)."""
    rng = np.random.default_rng([seed, nel, len(modes), nf] + [int(d) for d in dims])
    c = lambda *sh: rng.standard_normal(sh) + 1j * rng.standard_normal(sh)   # noqa: E731
    return 0.5 * c(len(modes), nel, nel), 0.5 * c(nf, len(modes))


def row_of(sample, hold, s, stage):
    return 2 * s + (stage + 1) // 2 if sample == "stage" else s // hold


def mu_bound(dims, A, modes):
    """An upper bound of ||mu_d||_1 for every drive: ||A_d||_1 times 1 or ||x_j||_1 <= 2 sqrt(N_j / 2)."""
    return np.array([np.abs(A[d]).sum(axis=0).max() * (1.0 if k < 0 else 2 * np.sqrt(dims[k] / 2))
                     for d, k in enumerate(modes)])


def drive_bound(dims, omega, Hel, W, A, modes, fvals):
    """lm.h_bound plus sum_d max|f_d| ||mu_d||_1: a bound of ||H(t)||_1 over the whole run."""
    extra = float((np.abs(fvals).max(axis=0) * mu_bound(dims, A, modes)).sum()) if len(modes) else 0.0
    return lm.h_bound(dims, omega, Hel, W) + extra


def eff_tables(Hel, W, A, modes, f, dtype=np.complex128):
    """(Hel(t), W(t)) for the field values f [nd], in `dtype`."""
    He = np.array(Hel, dtype=dtype)
    We = np.array(W, dtype=dtype)
    for d, k in enumerate(modes):
        term = dtype(f[d]) * np.asarray(A[d], dtype=dtype)
        if k < 0:
            He = He - term
        else:
            We[k] = We[k] - term
    return He, We


def driven_rk4(psi0, nel, dims, omega, Hel, W, A, modes, fvals, dt, nsteps, hold=1, sample="hold", save_every=0,
               dtype=np.complex128):
    """qd_lvc_driven_rk4 restated.  Returns (psi [B, D], snap [B, nsave, D] | None, obs [B, nsave + 1, nobs]) rounded
    to complex128 once."""
    real = lm.real_of(dtype)
    psi = np.asarray(psi0, dtype=dtype)
    dt = real(dt)
    mi = dtype(-1j)

    def L(v, s, stage):
        f = fvals[row_of(sample, hold, s, stage)] if len(modes) else ()
        He, We = eff_tables(Hel, W, A, modes, f, dtype)
        return mi * lm.apply(v, nel, dims, omega, He, We, dtype)

    saves, recs = [], [lm.record(psi, nel, dims, dtype)]
    for s in range(nsteps):
        if sample == "stage":
            k1 = L(psi, s, 0)
            k2 = L(psi + dt / real(2) * k1, s, 1)
            k3 = L(psi + dt / real(2) * k2, s, 2)
            k4 = L(psi + dt * k3, s, 3)
            psi = ((psi + dt / real(6) * k1) + dt / real(3) * k2 + dt / real(3) * k3) + dt / real(6) * k4
        else:
            v = psi
            for stage, c in enumerate((dt / real(4), dt / real(3), dt / real(2), dt)):
                v = psi + c * L(v, s, stage)
            psi = v
        if save_every > 0 and (s + 1) % save_every == 0:
            saves.append(psi.copy())
            recs.append(lm.record(psi, nel, dims, dtype))
    snap = np.stack(saves, axis=1).astype(np.complex128) if saves else None
    return psi.astype(np.complex128), snap, np.stack(recs, axis=1).astype(np.complex128)


def dense_mu(nel, dims, A_d, mode):
    """mu = A (x) 1 or A (x) x_mode as a dense [D, D] matrix from explicit Kronecker products."""
    fac = [lm.x_matrix(int(N)) if j == mode else np.eye(int(N)) for j, N in enumerate(dims)]
    return lm._kron(np.asarray(A_d, dtype=complex), *fac)


def dense_driven_rk4(psi0, H0, mus, fvals, dt, nsteps, hold=1, sample="hold"):
    """The same two rules on dense matrices: H_row = H0 - sum_d fvals[row, d] mus[d]; classical RK4 in both modes (with a
    generator constant within the step the Horner form is the same polynomial)."""
    psi = np.asarray(psi0, dtype=complex)

    def L(v, s, stage):
        H = H0 - sum(fvals[row_of(sample, hold, s, stage), d] * mu for d, mu in enumerate(mus)) if mus else H0
        return -1j * (v @ H.T)

    for s in range(nsteps):
        k1 = L(psi, s, 0)
        k2 = L(psi + dt / 2 * k1, s, 1)
        k3 = L(psi + dt / 2 * k2, s, 2)
        k4 = L(psi + dt * k3, s, 3)
        psi = psi + dt / 6 * (k1 + 2 * k2 + 2 * k3 + k4)
    return psi


# ---------------------------------------------------------------- the cases of tests/test_lvc_driven_kernels_gpu.py
NSTEPS, SE = 5, 2
# (sample, hold): hold 1, 2 (a partial last block), 3 (no multiple of the save interval), 6 (one row for the whole
# call), and stage mode
SETTINGS = [("hold", 1), ("hold", 2), ("hold", 3), ("hold", 6), ("stage", 1)]
FIXED = [(1, (1,)), (1, (2,)), (3, (70,)), (3, (3, 5, 7)), (8, (4, 3)), (3, (2, 2, 2, 2, 2, 2)), (3, (5, 67)),
         (3, (65, 3)), (2, (1, 9, 1)), (3, (37, 37))]
EIGHT = {(1, (1,)), (8, (4, 3)), (3, (3, 5, 7))}


def drive_modes(name, dims):
    """The drive_mode list of a named drive set: "el" one electronic drive; "ends" one drive on the fastest and one on
    the slowest mode; "inert" one drive on an axis of extent 1; "eight" eight drives, three of them on the table Hel."""
    M = len(dims)
    if name == "el":
        return [-1]
    if name == "ends":
        return [M - 1, 0]
    if name == "inert":
        return [list(dims).index(1)]
    if name == "eight":
        return [-1, 0, -1, M - 1, min(1, M - 1), -1, M - 1, 0]
    raise KeyError(name)


def gpu_cases(T, L, L6):
    """(nel, dims, drive set) of the GPU kernel test for the plan's tile extent T and its resident limits, L in one to
    five modes and L6 in six."""
    shapes = list(FIXED) + [(3, (T - 1,)), (3, (T,)), (3, (T + 1,)), (2, (2, T // 2))]
    shapes += [(1, (L,)), (1, (L + 1,)), (3, (L // 3,)), (3, (L // 3 + 1,)), (8, (L // 8,)), (2, (L // 2 // 64, 64))]
    shapes += [(3, (2, 2, 2, 2, 2, L6 // 96)), (3, (1, 1, 1, 1, 1, L6 // 3 + 1))]     # six modes: at and past their limit
    eight = EIGHT | {(8, (L // 8,))}
    out = []
    for nel, dims in shapes:
        out.append((nel, dims, "el"))
        if len(dims) >= 2:
            out.append((nel, dims, "ends"))
        if 1 in dims and len(dims) >= 2:
            out.append((nel, dims, "inert"))
        if (nel, dims) in eight:
            out.append((nel, dims, "eight"))
    return out


def gpu_inputs(nel, dims, name, B):
    """(omega, Hel, W, A, modes, fvals, psi0, dt) of one case: fvals has the 2 NSTEPS + 1 rows stage mode needs, hold
    mode reads its first ceil(NSTEPS / hold)."""
    omega, Hel, W = lm.random_model(nel, dims)
    modes = drive_modes(name, dims)
    A, fvals = random_drives(nel, dims, modes, 2 * NSTEPS + 1)
    psi0 = lm.random_states(B, nel, dims)
    dt = 0.5 / drive_bound(dims, omega, Hel, W, A, modes, fvals)
    return omega, Hel, W, A, modes, fvals, psi0, dt


# ---------------------------------------------------------------- the order check's model (one fixed case)
ORDER = dict(nel=2, dims=(8,), omega=(0.2,), E=(0.0, 1.0), W=np.array([[[0, 0.1], [0.1, 0.15]]], dtype=complex),
             A=np.array([[[0, 1], [1, 0]]], dtype=complex), modes=[-1], amplitude=0.3, omegac=1.0, tau=3.0, tc=10.0,
             T=20.0, nref=6400)


def order_field(t):
    o = ORDER
    return o["amplitude"] * np.exp(-(t - o["tc"]) ** 2 / 2 / o["tau"] ** 2) * np.cos(o["omegac"] * (t - o["tc"]))


def order_fvals(sample, nsteps):
    dt = ORDER["T"] / nsteps
    n = 2 * nsteps + 1 if sample == "stage" else nsteps
    return order_field((0.5 * dt if sample == "stage" else dt) * np.arange(n)).astype(complex).reshape(n, 1)


def order_run(sample, nsteps, dtype=np.complex128):
    """The final state of the order model from |0, 0> over T in nsteps steps, on the host."""
    o = ORDER
    psi0 = np.zeros((1, 16), dtype=complex)
    psi0[0, 0] = 1.0
    return driven_rk4(psi0, 2, o["dims"], o["omega"], np.diag(o["E"]).astype(complex), o["W"], o["A"], o["modes"],
                      order_fvals(sample, nsteps), o["T"] / nsteps, nsteps, 1, sample, dtype=dtype)[0]
