"""Generate tests/golden/ldr_jacobi.npz by running the REAL reference's LDR2_Jacobi (pyqed/ldr/ldr.py:1779-1987).

Run in the build container only (the reference does not exist on the GPU box):
    python tests/golden/make_golden_ldr_jacobi.py
The reference is imported read-only through ref_shim, as in make_golden_ldr.py.  Fixtures are data; no reference source
is copied.

The reference's class does not run as it stands; three attributes its constructor never sets are set by hand here, and
nothing else of it is touched:
  sol.nbasis = nx * ny     build_ovlp reads it (ldr.py:1479-1527)
  sol.dx, sol.dy           rdm_el reads them (ldr.py:1706); the constructor's own line is commented out (ldr.py:1833)
  sol.adiabatic_states     case b: build_ovlp is not called there (A is given), the attribute only feeds the fixture

Cases, all nt = 5, nout = 2, run dt 0.05, white-noise psi0 of norm one, domains (0.5, 3.5) x (0, pi),
mass = [1.3, lambda r: 2.0 * r ** 2]:
  a_*   levels (3, 3) = 7 x 7, M = ns = 2, sol.v = v, states from the reference's build_apes, constructor dt 0.05
  b_*   levels (4, 3) = 15 x 7, three diabatic states of which two are kept (M = 3, ns = 2), complex coupling; apes and
        adiabatic_states set, A formed here from the states by an einsum
  q_*   as a with constructor dt 0.03: buildK takes the constructor's dt, buildV run's
Each case holds x, y, v, apes, U, I (the moment of inertia on x), psi0, expKx (exp_K[0]), expKy (exp_K[1] [nx, ny, ny]),
states (every psilist entry), rdm (rdm_el of the last), dt_ctor.
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
DOMAINS = [(0.5, 3.5), (0.0, np.pi)]
MX = 1.3


def inertia(r):
    return 2.0 * r ** 2


def diabatic(x, y, M, cplx=False):
    """Two bound stretch surfaces crossing near r = 2, coupled through the angle; minimum shifted to zero."""
    X, Y = np.meshgrid(x, y, indexing="ij")
    v = np.zeros(X.shape + (M, M), dtype=complex if cplx else float)
    v[..., 0, 0] = 0.5 * (X - 1.6) ** 2 + 0.3 * (1.0 - np.cos(Y))
    v[..., 1, 1] = 0.4 * (X - 2.4) ** 2 + 0.2 * (1.0 + np.cos(Y)) + 0.1
    v[..., 0, 1] = 0.25 * np.sin(Y) + (0.1j * (X - 2.0) if cplx else 0.0)
    v[..., 1, 0] = v[..., 0, 1].conj()
    if M > 2:
        v[..., 2, 2] = 0.3 * (X - 2.0) ** 2 + 1.2
        v[..., 0, 2] = 0.1 * np.cos(Y) + (0.05j if cplx else 0.0)
        v[..., 2, 0] = v[..., 0, 2].conj()
        v[..., 1, 2] = 0.07 * (X - 2.0)
        v[..., 2, 1] = v[..., 1, 2].conj()
    return v


def noise(rng, shape):
    psi = rng.standard_normal(shape) + 1j * rng.standard_normal(shape)
    return psi / np.linalg.norm(psi)


def quiet():
    return contextlib.redirect_stdout(io.StringIO())


def by_hand(sol):
    sol.nbasis = sol.nx * sol.ny
    sol.dx, sol.dy = sol.x[1] - sol.x[0], sol.y[1] - sol.y[0]


def store(out, tag, sol, psi0, v, U, dt_ctor):
    with quiet():
        r = sol.run(psi0.copy(), dt=DT, nt=NT, nout=NOUT)
        rdm = sol.rdm_el(r.psilist[-1])
    assert len(r.psilist) == NT // NOUT + 1
    out.update({f"{tag}_x": sol.x, f"{tag}_y": sol.y, f"{tag}_v": v, f"{tag}_apes": np.asarray(sol.apes),
                f"{tag}_U": np.asarray(U), f"{tag}_I": inertia(sol.x), f"{tag}_psi0": psi0,
                f"{tag}_expKx": sol.exp_K[0], f"{tag}_expKy": sol.exp_K[1], f"{tag}_states": np.array(r.psilist),
                f"{tag}_rdm": np.asarray(rdm), f"{tag}_dt_ctor": dt_ctor})


def main():
    from pyqed.ldr.ldr import LDR2_Jacobi
    rng = np.random.default_rng(2025)
    out = {"dt": DT, "nt": NT, "nout": NOUT, "domains": np.array(DOMAINS), "mx": MX}

    for tag, dt_ctor in (("a", 0.05), ("q", 0.03)):
        sol = LDR2_Jacobi(DOMAINS, (3, 3), ['sine', 'sine'], mass=[MX, inertia], nstates=2, dt=dt_ctor)
        by_hand(sol)
        v = diabatic(sol.x, sol.y, 2)
        sol.v = v
        with quiet():
            sol.build_apes()
        store(out, tag, sol, noise(rng, (sol.nx, sol.ny, 2)), v, sol.adiabatic_states, dt_ctor)

    sol = LDR2_Jacobi(DOMAINS, (4, 3), ['sine', 'sine'], mass=[MX, inertia], nstates=2, dt=DT)
    by_hand(sol)
    v = diabatic(sol.x, sol.y, 3, True)
    w, u = np.linalg.eigh(v)
    U = u[..., :, :2].copy()
    sol.apes = w[..., :2].copy()
    sol.adiabatic_states = U
    sol.A = np.einsum("ijma,klmb->ijaklb", U.conj(), U)
    store(out, "b", sol, noise(rng, (sol.nx, sol.ny, 2)), v, U, DT)

    out["levels_a"], out["levels_b"] = np.array((3, 3)), np.array((4, 3))
    out["lib_versions"] = np.array(str(ref_shim.lib_versions()))
    path = os.path.join(HERE, "ldr_jacobi.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, f"{os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
