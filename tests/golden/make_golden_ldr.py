"""Generate tests/golden/ldr.npz by running the REAL reference's local-diabatic-representation solvers
(pyqed/ldr/ldr.py: LDR2, LDRN, ResultLDR) and its sine DVR (pyqed/dvr/dvr_1d.py SineDVR).

Run in the build container only (the reference does not exist on the GPU box):
    python tests/golden/make_golden_ldr.py
The reference is imported read-only through ref_shim, as in make_golden.py.  Fixtures are data; no reference source
is copied.

Stored:
  dvr{n}_*      SineDVR(-1.5, 2.5, n, mass=1.3): x, t(), expT(0.05), fbr2dvr() at n = 5 and 16
  a_*           LDR2 15 x 11, M = ns = 2, real states from the reference's build_apes, a Gaussian on the upper state
  b_*           LDR2 17 x 13, M = 3 kept ns = 2 (truncated: the step is a non-unitary projection), white noise
  c_*           as b with complex states, A from build_ovlp(dtype=complex)
  d_*           LDR2 9 x 8, sol.v = v and nothing else (the build path)
  s_*           LDR2 6 x 5, M = ns = 2: the whole short_time_propagator
  n_*           LDRN levels (3, 2, 2) = 7 x 3 x 3, M = 3, ns = 2, A formed here from the states
  m_*           LDRN levels (3, 2) = 7 x 3, M = 3, ns = 2, with ResultLDR.get_population(plot=False): the reference's
                get_population reads psi[:, :, n] and raises on a 3-D state, so its fixture is two-dimensional
Each LDR2 case holds x, y, v, apes, U (adiabatic_states), psi0, expKx, expKy, states (every psilist entry) and rdm
(rdm_el of the last).  Case a also holds columns of its short_time_propagator (the whole of it is 1.7 MB): a_stp_cols
names the flat (k, l, b) indices, a_stp [nx, ny, ns, ncols].
"""
from __future__ import annotations

import contextlib
import io
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_shim  # noqa: E402

ref_shim.install()

DT, NT, NOUT = 0.05, 5, 2


def diabatic(x, y, M, cplx=False):
    """A conical intersection at the origin, tuning along x and coupling along y; minimum shifted to zero."""
    X, Y = np.meshgrid(x, y, indexing="ij")
    v = np.zeros(X.shape + (M, M), dtype=complex if cplx else float)
    v[..., 0, 0] = 0.5 * ((X + 1.0) ** 2 + Y ** 2)
    v[..., 1, 1] = 0.5 * ((X - 1.0) ** 2 + Y ** 2) + 0.2
    v[..., 0, 1] = 0.4 * Y + (0.15j * X if cplx else 0.0)
    v[..., 1, 0] = v[..., 0, 1].conj()
    if M > 2:
        v[..., 2, 2] = 0.4 * (X ** 2 + (Y - 0.5) ** 2) + 1.5
        v[..., 0, 2] = 0.1 * X + (0.05j if cplx else 0.0)
        v[..., 2, 0] = v[..., 0, 2].conj()
        v[..., 1, 2] = 0.07 * Y
        v[..., 2, 1] = v[..., 1, 2].conj()
    return v


def gaussian(x, y, ns, state):
    X, Y = np.meshgrid(x, y, indexing="ij")
    psi = np.zeros(X.shape + (ns,), dtype=complex)
    psi[..., state] = np.exp(-0.5 * ((X - 0.4) ** 2 + (Y + 0.2) ** 2) / 0.5 ** 2 + 0.3j * X)
    return psi / np.sqrt(np.sum(np.abs(psi) ** 2) * (x[1] - x[0]) * (y[1] - y[0]))


def noise(rng, shape):
    psi = rng.standard_normal(shape) + 1j * rng.standard_normal(shape)
    return psi / np.linalg.norm(psi)


def quiet():
    return contextlib.redirect_stdout(io.StringIO())


def ldr2_case(out, tag, sol, psi0, x, y, v):
    with quiet():
        r = sol.run(psi0.copy(), dt=DT, nt=NT, nout=NOUT)
        rdm = sol.rdm_el(r.psilist[-1])
    assert len(r.psilist) == NT // NOUT + 1
    out.update({f"{tag}_x": x, f"{tag}_y": y, f"{tag}_v": v, f"{tag}_apes": np.asarray(sol.apes),
                f"{tag}_U": np.asarray(sol.adiabatic_states), f"{tag}_psi0": psi0,
                f"{tag}_expKx": sol.exp_K[0], f"{tag}_expKy": sol.exp_K[1],
                f"{tag}_states": np.array(r.psilist), f"{tag}_rdm": np.asarray(rdm)})


def main():
    from pyqed.dvr.dvr_1d import SineDVR
    from pyqed.ldr.ldr import LDR2, LDRN
    rng = np.random.default_rng(2024)
    out = {"dt": DT, "nt": NT, "nout": NOUT}

    for n in (5, 16):
        d = SineDVR(-1.5, 2.5, n, mass=1.3)
        out.update({f"dvr{n}_x": d.x, f"dvr{n}_t": d.t(), f"dvr{n}_expT": d.expT(0.05), f"dvr{n}_U": d.fbr2dvr()})
    out["dvr_args"] = np.array([-1.5, 2.5, 1.3, 0.05])

    # (a) M = ns = 2, the reference's own states
    x, y = np.linspace(-3, 3, 15), np.linspace(-2.5, 2.5, 11)
    v = diabatic(x, y, 2)
    sol = LDR2(x, y, nstates=2, mass=[1.0, 1.7])
    sol.v = v
    with quiet():
        sol.build_apes()
    ldr2_case(out, "a", sol, gaussian(x, y, 2, 1), x, y, v)
    with quiet():
        stp = sol.short_time_propagator(DT)
    D = 15 * 11 * 2
    cols = np.array([0, 1, 7, 164, 165, 211, D - 2, D - 1])
    out["a_stp_cols"] = cols
    out["a_stp"] = stp.reshape(15, 11, 2, D)[..., cols]

    # (b), (c) three diabatic states, the lowest two adiabatic ones kept
    x, y = np.linspace(-3, 3, 17), np.linspace(-2.5, 2.5, 13)
    for tag, cplx in (("b", False), ("c", True)):
        v = diabatic(x, y, 3, cplx)
        w, u = np.linalg.eigh(v)
        sol = LDR2(x, y, nstates=2, mass=[1.0, 1.7])
        sol.apes = w[..., :2].copy()
        sol.adiabatic_states = u[..., :, :2].copy()
        if cplx:
            sol.build_ovlp(dtype=complex)
        ldr2_case(out, tag, sol, noise(rng, (17, 13, 2)), x, y, v)

    # (d) the build path
    x, y = np.linspace(-2, 2, 9), np.linspace(-1.5, 1.5, 8)
    v = diabatic(x, y, 2)
    sol = LDR2(x, y, nstates=2)
    sol.v = v
    ldr2_case(out, "d", sol, gaussian(x, y, 2, 0), x, y, v)

    # (s) the whole short-time propagator on a small grid
    x, y = np.linspace(-2, 2, 6), np.linspace(-1.5, 1.5, 5)
    v = diabatic(x, y, 2)
    sol = LDR2(x, y, nstates=2, mass=[0.8, 1.1])
    sol.v = v
    with quiet():
        sol.build_apes()
        stp = sol.short_time_propagator(DT)
    out.update({"s_x": x, "s_y": y, "s_v": v, "s_apes": sol.apes, "s_U": sol.adiabatic_states, "s_stp": stp})

    # LDRN in three dimensions
    domains, levels = [(-3.0, 3.0), (-2.0, 2.0), (-2.0, 2.5)], (3, 2, 2)
    sol = LDRN(domains, levels, ndim=3, nstates=2, mass=[1.0, 1.7, 0.9])
    X = np.meshgrid(*sol.x, indexing="ij")
    v3 = np.zeros(X[0].shape + (3, 3), dtype=complex)
    v3[..., 0, 0] = 0.5 * ((X[0] + 1) ** 2 + X[1] ** 2 + 0.8 * X[2] ** 2)
    v3[..., 1, 1] = 0.5 * ((X[0] - 1) ** 2 + X[1] ** 2 + 1.2 * X[2] ** 2) + 0.2
    v3[..., 2, 2] = 0.4 * (X[0] ** 2 + X[1] ** 2 + X[2] ** 2) + 1.5
    v3[..., 0, 1] = 0.4 * X[1] + 0.1j * X[2]
    v3[..., 0, 2] = 0.1 * X[0]
    v3[..., 1, 2] = 0.07 * X[2]
    for a in range(3):
        for b in range(a):
            v3[..., a, b] = v3[..., b, a].conj()
    w, u = np.linalg.eigh(v3)
    U = u[..., :, :2].copy()
    sol.apes = w[..., :2].copy()
    sol.A = np.einsum("ijkma,lnomb->ijkalnob", U.conj(), U)
    psi0 = noise(rng, (7, 3, 3, 2))
    with quiet():
        r = sol.run(psi0.copy(), dt=DT, nt=NT, nout=NOUT)
        rdm = sol.rdm_el(r.psilist[-1])
    out.update({"n_domains": np.array(domains), "n_levels": np.array(levels), "n_mass": np.array(sol.mass),
                "n_v": v3, "n_apes": sol.apes, "n_U": U, "n_psi0": psi0, "n_states": np.array(r.psilist),
                "n_rdm": np.asarray(rdm), "n_dx": np.array(sol.dx),
                **{f"n_expK{d}": sol.exp_K[d] for d in range(3)}})

    # LDRN in two dimensions: the reference's ResultLDR.get_population takes psi[:, :, n] and runs in 2-D only
    domains, levels = [(-3.0, 3.0), (-2.0, 2.0)], (3, 2)
    sol = LDRN(domains, levels, ndim=2, nstates=2, mass=[1.0, 1.7])
    v2 = diabatic(sol.x[0], sol.x[1], 3, True)
    w, u = np.linalg.eigh(v2)
    U = u[..., :, :2].copy()
    sol.apes = w[..., :2].copy()
    sol.A = np.einsum("ijma,lnmb->ijalnb", U.conj(), U)
    psi0 = noise(rng, (7, 3, 2))
    with quiet():
        r = sol.run(psi0.copy(), dt=DT, nt=NT, nout=NOUT)
        pop = r.get_population(plot=False)
    out.update({"m_domains": np.array(domains), "m_levels": np.array(levels), "m_mass": np.array(sol.mass),
                "m_v": v2, "m_apes": sol.apes, "m_U": U, "m_psi0": psi0, "m_states": np.array(r.psilist),
                "m_pop": np.asarray(pop)})

    out["lib_versions"] = np.array(str(ref_shim.lib_versions()))
    path = os.path.join(HERE, "ldr.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, f"{os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
