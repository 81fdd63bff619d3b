"""Generate tests/golden/lvc.npz by running the REAL reference's LVC class (pyqed/mol.py:959-1293).

Run in the build container only (the reference does not exist on the GPU box):
    python tests/golden/make_golden_lvc.py
The reference is imported read-only through ref_shim, as in make_golden.py.  Fixtures are data; no reference source
is copied.

Two models of 3 electronic states, on 2 modes of 4 levels and on 3 modes of 3 levels (the reference's buildH needs at
least two modes and one truncation for all of them), with tuning (a == b) and coupling (a != b) terms and one
add_coupling after buildH.  Stored per model: the parameters, H as COO triplets, vertical(1), APES at two points,
rdm_el of a random state, and run(vertical(1), dt, Nt=10, nout=3, e_ops=[buildop(1), coordinate(0)]): the reference
returns 3 states and observables of shape (3, 2) for that run.
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

E = [0.0, 0.8, 1.1]
#        tag  truncations  (omega, couplings) per mode                                    add_coupling   APES points
CASES = [("a", (4, 4),
          [(0.10, [[[1, 1], 0.06], [[2, 2], -0.05]]), (0.13, [[[1, 2], 0.04]])],
          [[0, 1], 0.02], [[0.3, -0.7], [1.5, 0.4]]),
         ("b", (3, 3, 3),
          [(0.09, [[[1, 1], 0.05], [[0, 0], 0.01]]), (0.12, [[[1, 2], 0.03], [[0, 2], 0.02]]),
           (0.21, [[[2, 2], -0.07]])],
          [[1, 2], 0.015], [[0.2, 0.5, -1.0], [-0.8, 0.1, 0.6]])]
DT, NT, NOUT = 0.05, 10, 3


def main():
    from pyqed.mol import LVC, Mode
    rng = np.random.default_rng(97)
    out = {}
    for tag, trunc, modes, extra, pts in CASES:
        with contextlib.redirect_stdout(io.StringIO()):
            ms = [Mode(w, c, truncate=n) for (w, c), n in zip(modes, trunc)]
            mol = LVC(np.array(E), ms)
            mol.buildH()
            mol.add_coupling(extra)
            H = mol.H.tocoo()
            psi0 = mol.vertical(1)
            apes = np.array([mol.APES(np.array(p)) for p in pts])
            psi_r = rng.standard_normal(H.shape[0]) + 1j * rng.standard_normal(H.shape[0])
            psi_r /= np.linalg.norm(psi_r)
            rdm = mol.rdm_el(psi_r)
            sol = mol.wavepacket_dynamics()
            res = sol.run(psi0=psi0, dt=DT, Nt=NT, nout=NOUT, e_ops=[mol.buildop(1), mol.coordinate(0)])
        states = np.array([np.asarray(s).reshape(-1) for s in res.psilist])
        assert states.shape == (NT // NOUT, H.shape[0]) and res.observables.shape == (NT // NOUT, 2)
        out.update({f"{tag}_E": np.array(E), f"{tag}_trunc": np.array(trunc),
                    f"{tag}_omega": np.array([w for w, _ in modes]),
                    # couplings as rows (mode, a, b, strength)
                    f"{tag}_couplings": np.array([[j, c[0][0], c[0][1], c[1]] for j, (_, cs) in enumerate(modes)
                                                  for c in cs], dtype=float),
                    f"{tag}_extra": np.array([extra[0][0], extra[0][1], extra[1]], dtype=float),
                    f"{tag}_H_row": H.row.astype(np.int32), f"{tag}_H_col": H.col.astype(np.int32),
                    f"{tag}_H_val": np.asarray(H.data, dtype=complex),
                    f"{tag}_vertical1": np.asarray(psi0).reshape(-1),
                    f"{tag}_apes_x": np.array(pts), f"{tag}_apes": np.asarray(apes, dtype=complex),
                    f"{tag}_psi_r": psi_r, f"{tag}_rdm": np.asarray(rdm),
                    f"{tag}_states": states, f"{tag}_obs": np.asarray(res.observables)})
    out["dt"], out["Nt"], out["nout"] = DT, NT, NOUT
    out["lib_versions"] = np.array(str(ref_shim.lib_versions()))
    path = os.path.join(HERE, "lvc.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, f"{os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
