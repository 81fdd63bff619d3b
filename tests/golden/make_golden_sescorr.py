"""Generate tests/golden/sesolver_corr.npz by running the REAL reference's SESolver correlation functions.

Run in the build container only (the reference does not exist on the GPU box):
    python tests/golden/make_golden_sescorr.py
The reference is imported read-only through ref_shim, as in make_golden.py.  Fixtures are data; no reference
source is copied.

SESolver.propagator, correlation_3op_1t / _2t, correlation_4op_1t / _2t (pyqed/mol.py:1468-1566): H random
Hermitian scaled by 1/sqrt(N) (case b: H - (i/2) diag(gamma), non-Hermitian), four Ginibre operators, normalised
psi0.  The 1t functions are stored with Nt = Ntau, the length of the tau axis of the 2t ones.
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

#        tag  N  Nt Ntau  dt   non-Hermitian
CASES = [("a", 37, 5, 7, 0.02, False),
         ("b", 12, 6, 4, 0.05, True),
         ("c", 5, 1, 1, 0.1, False)]


def _herm(rng, n, scale=1.0):
    a = rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))
    return scale * (a + a.conj().T) / 2


def _ginibre(rng, n):
    return rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))


def main():
    from pyqed.mol import SESolver
    rng = np.random.default_rng(61)
    out = {}
    for tag, N, Nt, Ntau, dt, nonherm in CASES:
        H = _herm(rng, N, 1 / np.sqrt(N))
        if nonherm:
            H = H - 0.5j * np.diag(rng.uniform(0.0, 0.3, N))
        ops = [_ginibre(rng, N) for _ in range(4)]
        psi0 = rng.standard_normal(N) + 1j * rng.standard_normal(N)
        psi0 /= np.linalg.norm(psi0)
        sol = SESolver(H)
        out.update({f"{tag}_H": H, f"{tag}_ops": np.array(ops), f"{tag}_psi0": psi0, f"{tag}_dt": dt,
                    f"{tag}_Nt": Nt, f"{tag}_Ntau": Ntau,
                    f"{tag}_c3_1t": sol.correlation_3op_1t(psi0, ops[:3], dt, Ntau),
                    f"{tag}_c3_2t": sol.correlation_3op_2t(psi0, ops[:3], dt, Nt, Ntau),
                    f"{tag}_c4_1t": sol.correlation_4op_1t(psi0, ops, dt, Ntau),
                    f"{tag}_c4_2t": sol.correlation_4op_2t(psi0, ops, dt, Nt, Ntau)})
        if tag == "b":
            with contextlib.redirect_stdout(io.StringIO()):
                U = sol.propagator(dt, 4)
            out["b_prop"] = np.array([np.asarray(u.toarray() if hasattr(u, "toarray") else u) for u in U])
            out["b_prop_Nt"] = 4
    out["lib_versions"] = np.array(str(ref_shim.lib_versions()))
    path = os.path.join(HERE, "sesolver_corr.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, f"{os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
