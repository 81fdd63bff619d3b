"""Generate tests/golden/spo_observables.npz by running the REAL reference's SPO2 observables.

Run in the build container only (the reference does not exist on the GPU box):
    python tests/golden/make_golden_spoobs.py
The reference is imported read-only through ref_shim, as in make_golden.py.  Fixtures are data; no reference
source is copied.

SPO2.population (diabatic and adiabatic, list branch), SPO2.rdm_el (list branch) and ResultSPO2.position
(pyqed/wpd.py:627-689, 760-794, 138-159):

  case a: SPO2 on a 24 x 20 grid with three surfaces (the potential of tests/spo_models.spo2_model_rect), a packet
          displaced in x AND y with momentum along both, spread over two surfaces, so that <y> is not rounding noise
          and the reduced density matrix has off-diagonal weight from the first row on; nt = 6, nout = 2.  The
          reference's psilist is stored with its observables and its d2a (the adiabatic numbers depend on the
          eigenvector gauge, so the test applies the stored matrices).
  case b: the same observables for the states already in spo2_32.npz (regenerated here from make_golden's model and
          checked against that file); no states are stored.
"""
from __future__ import annotations

import contextlib
import io
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import ref_shim  # noqa: E402

ref_shim.install()

from spo_models import spo2_model_rect  # noqa: E402


def _observables(sol, r):
    """The reference's own numbers for the states of r (position() writes xAve.npz into the CWD: a scratch one)."""
    states = list(r.psilist)
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)
        try:
            xAve, yAve = r.position()
        finally:
            os.chdir(cwd)
    return dict(pop=sol.population(states), pop_adiabatic=sol.population(states, 'adiabatic'),
                d2a=np.asarray(sol.d2a), rdm=np.array(sol.rdm_el(states)), xAve=np.asarray(xAve),
                yAve=np.asarray(yAve))


def case_a():
    from pyqed.wpd import SPO2
    nx, ny, ns, dt, nt, nout = 24, 20, 3, 0.05, 6, 2
    x, y, surfaces, couplings, _ = spo2_model_rect(nx, ny, ns)
    X, Y = np.meshgrid(x, y, indexing="ij")
    g = np.exp(-((X + 1.5) ** 2 + (Y - 0.8) ** 2) / 2 + 0.5j * X - 0.7j * Y) / np.sqrt(np.pi)
    psi0 = np.zeros((nx, ny, ns), dtype=complex)
    psi0[:, :, 0] = np.sqrt(0.7) * g
    psi0[:, :, 1] = np.sqrt(0.3) * g * np.exp(0.4j)
    sol = SPO2(x, y, mass=[1.0, 1.3], nstates=ns)
    sol.set_DPES(surfaces, couplings)
    with contextlib.redirect_stdout(io.StringIO()):
        r = sol.run(psi0, dt=dt, nt=nt, nout=nout)
    out = dict(nx=nx, ny=ny, ns=ns, dt=dt, nt=nt, nout=nout, masses=np.array([1.0, 1.3]), psi0=psi0,
               psilist=np.array(r.psilist))
    out.update(_observables(sol, r))
    return {f"a_{k}": v for k, v in out.items()}


def case_b():
    from pyqed.wpd import SPO2
    import make_golden
    g = np.load(os.path.join(HERE, "spo2_32.npz"))
    x, y, v0, v1, c, psi0 = make_golden.spo2_model(32)
    sol = SPO2(x, y, mass=[1.0, 1.0], nstates=2)
    sol.set_DPES([v0, v1], [[[0, 1], c]])
    with contextlib.redirect_stdout(io.StringIO()):
        r = sol.run(psi0, dt=float(g["dt"]), nt=int(g["nt"]), nout=int(g["nout"]))
    assert np.allclose(np.array(r.psilist), g["psilist"], rtol=0, atol=1e-13), "spo2_32.npz is another model"
    r.psilist = list(g["psilist"])   # the observables of exactly the stored states
    return {f"b_{k}": v for k, v in _observables(sol, r).items()}


def main():
    out = {}
    out.update(case_a())
    out.update(case_b())
    out["lib_versions"] = np.array(str(ref_shim.lib_versions()))
    path = os.path.join(HERE, "spo_observables.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, f"{os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
