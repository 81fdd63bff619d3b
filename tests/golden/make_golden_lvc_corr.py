"""Generate tests/golden/lvc_corr.npz by running the REAL reference's SESolver correlation functions on its LVC model.

Run in the build container only (the reference does not exist on the GPU box):
    python tests/golden/make_golden_lvc_corr.py
The reference is imported read-only through ref_shim, as in make_golden_sescorr.py.  Fixtures are data; no reference
source is copied.

The reference's LVC with 3 electronic states on two modes of 3 levels each (equal truncations, D = 27), tuning and
coupling terms; SESolver(mol.H).correlation_3op_1t, correlation_3op_2t, correlation_4op_1t and correlation_4op_2t
(pyqed/mol.py:1475-1566) on the reference's own H, with the operators of mol.buildop and mol.coordinate, from a random
normalised state.  Stored: the model's parameters, the reference's operators as dense arrays next to their factors
(electronic matrix and mode, -1 for none), and the four results.  The 1t functions are stored with Nt = Ntau.
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
TRUNC = (3, 3)
MODES = [(0.10, [[[1, 1], 0.06], [[2, 2], -0.05]]), (0.13, [[[1, 2], 0.04], [[0, 1], 0.03]])]
DT, NT, NTAU = 0.05, 4, 6
# the operators by how they are made: ("buildop", i, f) or ("coordinate", n)
OPS3 = [("buildop", 0, 1), ("coordinate", 0), ("buildop", 0, 1)]
OPS4 = [("buildop", 0, 1), ("buildop", 1, 2), ("coordinate", 1), ("buildop", 0, 2)]


def _dense(a):
    return np.asarray(a.toarray() if hasattr(a, "toarray") else a, dtype=complex)


def main():
    from pyqed.mol import LVC, Mode, SESolver
    rng = np.random.default_rng(131)
    with contextlib.redirect_stdout(io.StringIO()):
        mol = LVC(np.array(E), [Mode(w, c, truncate=n) for (w, c), n in zip(MODES, TRUNC)])
        mol.buildH()
        make = lambda s: mol.buildop(s[1], s[2]) if s[0] == "buildop" else mol.coordinate(s[1])   # noqa: E731
        ops3, ops4 = [make(s) for s in OPS3], [make(s) for s in OPS4]
        H = mol.H
        D = H.shape[0]
        psi0 = rng.standard_normal(D) + 1j * rng.standard_normal(D)
        psi0 /= np.linalg.norm(psi0)
        sol = SESolver(H)
        c3_1t = sol.correlation_3op_1t(psi0, ops3, DT, NTAU)
        c3_2t = sol.correlation_3op_2t(psi0, ops3, DT, NT, NTAU)
        c4_1t = sol.correlation_4op_1t(psi0, ops4, DT, NTAU)
        c4_2t = sol.correlation_4op_2t(psi0, ops4, DT, NT, NTAU)
    assert D == 27 and c3_1t.shape == (NTAU,) and c3_2t.shape == (NT, NTAU) and c4_2t.shape == (NT, NTAU)
    Hc = H.tocoo()
    out = {"E": np.array(E), "trunc": np.array(TRUNC), "omega": np.array([w for w, _ in MODES]),
           # couplings as rows (mode, a, b, strength)
           "couplings": np.array([[j, c[0][0], c[0][1], c[1]] for j, (_, cs) in enumerate(MODES) for c in cs],
                                 dtype=float),
           "H_row": Hc.row.astype(np.int32), "H_col": Hc.col.astype(np.int32), "H_val": np.asarray(Hc.data, complex),
           # the operators as rows (kind, i, f): kind 0 buildop(i, f), kind 1 coordinate(i)
           "ops3_spec": np.array([[0 if s[0] == "buildop" else 1, s[1], s[2] if len(s) > 2 else -1] for s in OPS3]),
           "ops4_spec": np.array([[0 if s[0] == "buildop" else 1, s[1], s[2] if len(s) > 2 else -1] for s in OPS4]),
           "ops3": np.array([_dense(o) for o in ops3]), "ops4": np.array([_dense(o) for o in ops4]),
           "psi0": psi0, "dt": DT, "Nt": NT, "Ntau": NTAU,
           "c3_1t": np.asarray(c3_1t), "c3_2t": np.asarray(c3_2t), "c4_1t": np.asarray(c4_1t),
           "c4_2t": np.asarray(c4_2t), "lib_versions": np.array(str(ref_shim.lib_versions()))}
    path = os.path.join(HERE, "lvc_corr.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, f"{os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
