"""Generate tests/golden/sos_signals.npz by running the REAL reference's sum-over-states signals.

Run in the build container only (the reference does not exist on the GPU box):
    python tests/golden/make_golden_sos.py
The reference is imported read-only through ref_shim, as in make_golden.py.  Fixtures are data; no reference
source is copied.

pyqed/signal/sos.py GSB, SE, ESA, _SE, _ESA, photon_echo_t3 (through Mol.PE2), DQC_R1, DQC_R2, TPA, TPA2D,
TPA2D_time_order, cars (also through Mol.cars), absorption (through Mol.absorption) and linear_absorption on two models:

  a: N = 6, g = [0], e = [1, 2, 3], f = [4, 5], real symmetric dipoles
  b: N = 8, complex Hermitian dipoles (they pin dip[b, a] against dip[a, b]), g = [0, 1], e = [2, 3, 4], f = [5, 6, 7]
gamma[0] = 0 in both.  Grids are rectangular (11 x 7) wherever the reference accepts them; its standalone GSB / SE / ESA
need a square one (9 x 9).  Each case stores its inputs beside the reference's output.
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
import ref_shim  # noqa: E402

ref_shim.install()


def model(tag):
    rng = np.random.default_rng({"a": 5, "b": 6}[tag])
    if tag == "a":
        N, g, e, f = 6, [0], [1, 2, 3], [4, 5]
        E = np.array([0.0, 1.00, 1.13, 1.31, 2.05, 2.42])
        d = rng.uniform(0.2, 1.0, (N, N))
        dip = (d + d.T) / 2
    else:
        N, g, e, f = 8, [0, 1], [2, 3, 4], [5, 6, 7]
        E = np.array([0.0, 0.06, 0.95, 1.08, 1.22, 1.96, 2.17, 2.31])
        d = rng.uniform(0.2, 1.0, (N, N)) * np.exp(1j * rng.uniform(-np.pi, np.pi, (N, N)))
        dip = (d + d.conj().T) / 2
    gamma = rng.uniform(0.01, 0.04, N)
    gamma[0] = 0.0
    return dict(E=E, dip=dip, gamma=gamma, g=np.array(g), e=np.array(e), f=np.array(f))


def case(tag):
    import pyqed.signal.sos as sos
    from pyqed.mol import Mol
    m = model(tag)
    E, dip, gamma, g, e, f = (m[k] for k in ("E", "dip", "gamma", "g", "e", "f"))
    N = len(E)
    out = dict(m)
    # square grids for the standalone pathways
    w1s, w3s = np.linspace(-1.5, -0.8, 9), np.linspace(0.7, 1.6, 9)
    out.update(w1s=w1s, w3s=w3s, tau2=3.0)
    out["GSB"] = sos.GSB(E, dip, w1s, w3s, 3.0, g, e, gamma)
    out["SE"] = sos.SE(E, dip, w1s, w3s, 3.0, g, e, gamma)
    out["ESA"] = sos.ESA(E, dip, w1s, w3s, 3.0, g, e, f, gamma)
    # rectangular grids
    w1, w2 = np.linspace(-1.5, -0.8, 11), np.linspace(-0.4, 0.4, 7)
    out.update(w1=w1, w2=w2, t3=2.5, deph=0.015)
    out["SE_t3"] = sos._SE(E, dip, w1, w2, 2.5, g, e, gamma, dephasing=0.015)
    out["ESA_t3"] = sos._ESA(E, dip, w1, w2, 2.5, g, e, f, gamma, dephasing=0.015)
    out["SE_t3_default"] = sos._SE(E, dip, w1, w2, 2.5, g, e, gamma)
    # Mol.PE2 -> photon_echo_t3 (omega1 negated, mol.dephasing, default e_idx = f_idx = range(1, N))
    mol = Mol(np.diag(E), dip)
    mol.edip_rms = dip
    mol.set_decay(gamma)
    mol.set_dephasing(0.02)
    pe_w1 = np.linspace(0.8, 1.5, 11)
    out.update(pe_w1=pe_w1, pe_deph=0.02)
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as td:
        os.chdir(td)
        try:
            S = mol.PE2(pe_w1, w2, t3=2.5)
            z = np.load("2DES.npz")
            assert len(z.files) == 3 and np.array_equal(z["arr_2"], S)
            se, esa = mol.PE2(pe_w1, w2, t3=2.5, separate=True, fname="sep")
            assert len(np.load("sep.npz").files) == 4
            se_l, esa_l = mol.PE2(pe_w1, w2, t3=2.5, separate=True, g_idx=g, e_idx=e, f_idx=f)
        finally:
            os.chdir(cwd)
    out.update(PE2=S, PE2_se=se, PE2_esa=esa, PE2_se_lists=se_l, PE2_esa_lists=esa_l)
    # double-quantum coherence, both modes
    o1, o2, o3 = np.linspace(0.8, 1.5, 11), np.linspace(1.8, 2.6, 7), np.linspace(0.6, 1.4, 5)
    out.update(dq_w1=o1, dq_w2=o2, dq_w3=o3, dq_tau=1.7)
    kw = dict(g_idx=g, e_idx=e, f_idx=f, gamma=gamma)
    out["DQC_R1_t3"] = sos.DQC_R1(E, dip, omega1=o1, omega2=o2, tau3=1.7, **kw)
    out["DQC_R1_t1"] = sos.DQC_R1(E, dip, omega2=o2, omega3=o3, tau1=1.7, **kw)
    out["DQC_R2_t3"] = sos.DQC_R2(E, dip, omega1=o1, omega2=o2, tau3=1.7, **kw)
    out["DQC_R2_t1"] = sos.DQC_R2(E, dip, omega2=o2, omega3=o3, tau1=1.7, **kw)
    # two-photon absorption
    wp, wt = np.linspace(1.8, 2.6, 11), np.linspace(0.8, 1.5, 7)
    out.update(tpa_wp=wp, tpa_w1=wt)
    out["TPA_scalar"] = np.array(sos.TPA(E, dip, 2.1, g, e, f, gamma))
    out["TPA_array"] = sos.TPA(E, dip, wp, g, e, f, gamma)
    out["TPA2D"] = sos.TPA2D(E, dip, wp, wt, g, e, f, gamma)
    out["TPA2D_time_order"] = sos.TPA2D_time_order(E, dip, wp, wt, g, e, f, gamma)
    # CARS: standalone with a linewidth, Mol.cars with the default
    shift = np.linspace(-0.5, 0.5, 11)
    out.update(cars_shift=shift, cars_w1=wt, cars_gamma=0.012)
    out["cars"] = sos.cars(E, dip, shift, wt, gamma=0.012)
    out["Mol_cars"] = mol.cars(shift, wt)
    # linear absorption
    wa = np.linspace(0.5, 2.8, 23)
    out.update(abs_w=wa, abs_linewidth=0.03)
    with contextlib.redirect_stdout(io.StringIO()):
        out["absorption_lw"] = mol.absorption(wa, linewidth=0.03, plt_signal=False)
        out["absorption_default"] = mol.absorption(wa, plt_signal=False)
        out["absorption_norm"] = mol.absorption(wa, linewidth=0.03, plt_signal=False, normalize=True)
    te, td_ = E[1:] - E[0], np.abs(dip[1:, 0])
    out.update(la_e=te, la_d=td_, la_gamma=0.025)
    out["linear_absorption"] = sos.linear_absorption(wa, te, td_, gamma=0.025)
    out["linear_absorption_norm"] = sos.linear_absorption(wa, te, td_, gamma=0.025, normalize=True)
    return {f"{tag}_{k}": np.asarray(v) for k, v in out.items()}


def main():
    out = {}
    out.update(case("a"))
    out.update(case("b"))
    out["lib_versions"] = np.array(str(ref_shim.lib_versions()))
    path = os.path.join(HERE, "sos_signals.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, f"{os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
