"""Generate tests/golden/gmat2d.npz by running the REAL reference's curvilinear wavepacket propagation.

Run in the build container only (the reference does not exist on the GPU box):
    python tests/golden/make_golden_gmat.py
The reference is imported read-only through ref_shim, as in make_golden.py.  Fixtures are data; no reference
source is copied.

adiabatic_2d(coords='curvilinear'), hpsi and KEO (pyqed/wpd.py:1783-1940) on the model of tests/gmat_models.py:

  case a: 24 x 20 (the any-length path), Nt = 20; also hpsi and KEO of a stored white-noise input
  case b: 32 x 16 (the power-of-two path), Nt = 20
  case c: 16 x 16 with the absorbing potential v - 0.1j, Nt = 10
Each case stores x, y, G, v, dt, psi0 and the reference's final psi.
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import ref_shim  # noqa: E402

ref_shim.install()

from gmat_models import model  # noqa: E402


def case(tag, nx, ny, nt, absorb=0.0, noise_seed=None):
    from pyqed.wpd import KEO, adiabatic_2d, hpsi
    m = model(nx, ny)
    v = m["v"] - 1j * absorb if absorb else m["v"]
    psi0 = m["psi0"].copy()
    psi = adiabatic_2d(m["x"], m["y"], psi0, v, m["dt"], Nt=nt, coords="curvilinear", G=m["G"])
    assert np.array_equal(psi0, m["psi0"]), "the reference modified psi0"
    out = dict(x=m["x"], y=m["y"], G=m["G"], v=v, dt=m["dt"], nt=nt, psi0=psi0, psi=psi)
    if noise_seed is not None:
        rng = np.random.default_rng(noise_seed)
        w = rng.standard_normal((nx, ny)) + 1j * rng.standard_normal((nx, ny))
        w /= np.linalg.norm(w)
        out.update(noise=w, hpsi=hpsi(w, m["kx"], m["ky"], v, m["G"]), keo=KEO(w, m["kx"], m["ky"], m["G"]))
    return {f"{tag}_{k}": val for k, val in out.items()}


def main():
    out = {}
    out.update(case("a", 24, 20, 20, noise_seed=11))
    out.update(case("b", 32, 16, 20))
    out.update(case("c", 16, 16, 10, absorb=0.1))
    out["lib_versions"] = np.array(str(ref_shim.lib_versions()))
    path = os.path.join(HERE, "gmat2d.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, f"{os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
