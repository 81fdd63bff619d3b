"""Sum-over-states nonlinear spectra (drop-in for pyqed/signal/sos.py photon_echo)."""
from __future__ import annotations

import numpy as np
import torch

from . import _lib
from ._util import default_device


def _photon_echo(evals, edip, omega1, omega3, t2, g_idx, e_idx, f_idx, gamma):
    """GSB + SE + ESA on the (omega3, omega1) grid (sos.py:845-879), computed on the GPU.
    Returns S [len(omega3), len(omega1)]."""
    dev = default_device()
    _lib.ensure_device(dev)
    E = torch.from_numpy(np.ascontiguousarray(np.asarray(evals, dtype=complex))).to(dev)
    D = torch.from_numpy(np.ascontiguousarray(np.asarray(edip, dtype=complex))).to(dev)
    G = torch.from_numpy(np.ascontiguousarray(np.asarray(gamma, dtype=float))).to(dev)
    idx = [torch.from_numpy(np.ascontiguousarray(np.asarray(list(x), dtype=np.int32).reshape(-1))).to(dev)
           for x in (g_idx, e_idx, f_idx)]
    pump = torch.from_numpy(np.ascontiguousarray(-np.asarray(omega1, dtype=float))).to(dev)
    probe = torch.from_numpy(np.ascontiguousarray(np.asarray(omega3, dtype=float))).to(dev)
    N = E.numel()
    S = torch.empty((probe.numel(), pump.numel()), dtype=torch.complex128, device=dev)
    with torch.cuda.device(dev):
        rc = _lib.load().qd_photon_echo(E.data_ptr(), D.data_ptr(), G.data_ptr(), N, idx[0].data_ptr(),
                                        idx[0].numel(), idx[1].data_ptr(), idx[1].numel(), idx[2].data_ptr(),
                                        idx[2].numel(), pump.data_ptr(), pump.numel(), probe.data_ptr(),
                                        probe.numel(), float(t2), S.data_ptr(), _lib.stream_ptr(dev))
    _lib.check(rc, "qd_photon_echo")
    return S.cpu().numpy()


def photon_echo(mol, pump, probe, t2=0., g_idx=[0], e_idx=None, f_idx=None, fname='signal', plt_signal=False,
                pol=None):
    """sos.py:962-1052: S = GSB + SE + ESA with omega1 = -pump; writes `fname`.npz as the reference."""
    E = mol.eigvals()
    dip = mol.edip_rms
    gamma = mol.gamma
    if gamma is None:
        raise ValueError('Please set the decay constants gamma first.')
    N = mol.nstates
    if e_idx is None:
        e_idx = range(N)
    if f_idx is None:
        f_idx = range(N)
    S = _photon_echo(E, dip, omega1=-np.asarray(pump), omega3=probe, t2=t2, g_idx=g_idx, e_idx=e_idx, f_idx=f_idx,
                     gamma=gamma)
    if fname is not None:
        np.savez(fname, pump, probe, S)
    return S


# ------------------------------------------------------------------ the other signals of pyqed/signal/sos.py
# Third-order pathways run through qd_sos_pathway (csrc/sos_signals.hip): the fixed-delay factor is summed first, which
# leaves S[i, j] = sum_p 1 / (x_i - zx[p]) sum_q W[p, q] / (y_j - zy[p, q]) (qd_sos_polesum).  The 1-D absorption
# signals are the same pole sum on a one-column grid, TPA has a kernel of its own (qd_sos_tpa).  Nothing plots:
# plt_signal is accepted and ignored.  Every argument check runs on the host, before any device call.
au2ev = 27.2116
au2mev = 27.2116e3

# include/qdyn.h QD_SOS_*
_PATHWAY = {"GSB": 0, "SE": 1, "ESA": 2, "SE_T3": 3, "ESA_T3": 4, "DQC_R1_T3": 5, "DQC_R1_T1": 6, "DQC_R2_T3": 7,
            "DQC_R2_T1": 8, "CARS": 9}
_SOS_POLE, _SOS_UNITY = 0, 1


def lorentzian(x, width=1.):
    """phys.py:1084-1103: width is the half width at half maximum."""
    return 1. / np.pi * width / (width ** 2 + (x) ** 2)


def issorted(a):
    """sos.py:38-53."""
    return np.all(np.diff(a) >= 0)


def _grid(w, name):
    g = np.ascontiguousarray(np.asarray(w, dtype=float).reshape(-1))
    if g.size < 1:
        raise ValueError(f"{name} must hold at least one frequency")
    return g


def _index_list(idx, N, name):
    a = np.ascontiguousarray(np.asarray(list(idx), dtype=np.int64).reshape(-1))
    if a.size and (a.min() < 0 or a.max() >= N):
        raise ValueError(f"{name} must index the {N} states, got {a.tolist()}")
    return a.astype(np.int32)


def _states(E, dip, gamma, who, real_E=False):
    """Host copies of E [N], dip [N, N] (complex) and gamma [N], with their shapes checked."""
    if gamma is None:
        raise ValueError(f"{who}: gamma (the decay rates of the states) must be given")
    E = np.asarray(E)
    if real_E:
        if np.iscomplexobj(E) and np.any(E.imag != 0):
            raise ValueError(f"{who}: complex eigenvalues are not supported, the signal is a real array")
        E = E.real
    E = np.ascontiguousarray(E.reshape(-1), dtype=float if real_E else complex)
    N = E.size
    D = np.ascontiguousarray(np.asarray(dip, dtype=complex))
    G = np.ascontiguousarray(np.asarray(gamma, dtype=float).reshape(-1))
    if N < 1 or D.shape != (N, N) or G.size != N:
        raise ValueError(f"{who}: E [N], dip [N, N] and gamma [N] do not agree: {E.shape}, {D.shape}, {G.shape}")
    return E, D, G


def _pathways(paths, E, dip, gamma, dephasing, g_idx, e_idx, f_idx, delay, wa, wb, who, accumulate=False):
    """One qd_sos_pathway call per entry of `paths` on one upload of the model; wa, wb in the reference's argument
    order.  Returns the list of host arrays (one array, their sum, when accumulate)."""
    E, D, G = _states(E, dip, gamma, who)
    N = E.size
    lists = [_index_list(x if x is not None else [], N, n) for x, n in
             ((g_idx, "g_idx"), (e_idx, "e_idx"), (f_idx, "f_idx"))]
    wa, wb = _grid(wa, "the first frequency grid"), _grid(wb, "the second frequency grid")
    dev = default_device()
    _lib.ensure_device(dev)
    up = lambda a: torch.from_numpy(a).to(dev)
    Et, Dt, Gt, gi, ei, fi, xa, xb = (up(a) for a in (E, D, G, *lists, wa, wb))
    outs = []
    lib = _lib.load()
    with torch.cuda.device(dev):
        for k, path in enumerate(paths):
            first = path in ("GSB", "SE", "ESA", "SE_T3", "ESA_T3")   # laid [len(wb), len(wa)]
            if not (accumulate and k):
                S = torch.empty((wb.size, wa.size) if first else (wa.size, wb.size), dtype=torch.complex128, device=dev)
                outs.append(S)
            rc = lib.qd_sos_pathway(_PATHWAY[path], Et.data_ptr(), Dt.data_ptr(), Gt.data_ptr(), N, float(dephasing),
                                    _lib.ptr(gi) if gi.numel() else None, gi.numel(),
                                    _lib.ptr(ei) if ei.numel() else None, ei.numel(),
                                    _lib.ptr(fi) if fi.numel() else None, fi.numel(), float(delay), xa.data_ptr(),
                                    xa.numel(), xb.data_ptr(), xb.numel(), S.data_ptr(), int(bool(accumulate and k)),
                                    _lib.stream_ptr(dev))
            _lib.check(rc, f"qd_sos_pathway({path})")
    return [S.cpu().numpy() for S in outs]


def GSB(evals, dip, omega1, omega3, tau2, g_idx, e_idx, gamma):
    """sos.py:624-678, gg -> ge -> gg -> e'g -> gg.  Returns [len(omega3), len(omega1)] (any grid; the reference
    needs a square one)."""
    return _pathways(["GSB"], evals, dip, gamma, 0., g_idx, e_idx, [], tau2, omega1, omega3, "GSB")[0]


def SE(evals, dip, omega1, omega3, tau2, g_idx, e_idx, gamma):
    """sos.py:731-785, stimulated emission at -k1 + k2 + k3.  Returns [len(omega3), len(omega1)]."""
    return _pathways(["SE"], evals, dip, gamma, 0., g_idx, e_idx, [], tau2, omega1, omega3, "SE")[0]


def ESA(evals, dip, omega1, omega3, tau2, g_idx, e_idx, f_idx, gamma):
    """sos.py:498-557, excited-state absorption (sign -1).  Returns [len(omega3), len(omega1)]."""
    return _pathways(["ESA"], evals, dip, gamma, 0., g_idx, e_idx, f_idx, tau2, omega1, omega3, "ESA")[0]


def _SE(E, dip, omega1, omega2, t3, g_idx, e_idx, gamma, dephasing=10 / au2mev):
    """sos.py:788-842: SE on (omega1, omega2) at detection time t3, with pure dephasing.
    Returns [len(omega2), len(omega1)]."""
    return _pathways(["SE_T3"], E, dip, gamma, dephasing, g_idx, e_idx, [], t3, omega1, omega2, "_SE")[0]


def _ESA(evals, dip, omega1, omega2, t3, g_idx, e_idx, f_idx, gamma, dephasing=10 / au2mev):
    """sos.py:560-622: ESA on (omega1, omega2) at detection time t3, with pure dephasing.
    Returns [len(omega2), len(omega1)]."""
    return _pathways(["ESA_T3"], evals, dip, gamma, dephasing, g_idx, e_idx, f_idx, t3, omega1, omega2, "_ESA")[0]


def photon_echo_t3(mol, omega1, omega2, t3, g_idx=[0], e_idx=None, f_idx=None, fname='2DES', plt_signal=False,
                   separate=False):
    """sos.py:882-960: _SE + _ESA with omega1 negated, mol.dephasing and e_idx = f_idx = range(1, N) by default;
    writes `fname`.npz (omega1, omega2, S) or, with separate, (omega1, omega2, se, esa) and returns (se, esa)."""
    E = mol.eigvals()
    edip = mol.edip_rms
    gamma = mol.gamma
    dephasing = mol.dephasing
    if gamma is None:
        raise ValueError('Please set the decay constants gamma first.')
    N = mol.nstates
    if e_idx is None:
        e_idx = range(1, N)
    if f_idx is None:
        f_idx = range(1, N)
    out = _pathways(["SE_T3", "ESA_T3"], E, edip, gamma, dephasing, g_idx, e_idx, f_idx, t3, -np.asarray(omega1),
                    omega2, "photon_echo_t3", accumulate=not separate)
    if separate:
        se, esa = out
        np.savez(fname, omega1, omega2, se, esa)
        return se, esa
    S = out[0]
    np.savez(fname, omega1, omega2, S)
    return S


def _dqc(which, evals, dip, omega1, omega2, omega3, tau1, tau3, g_idx, e_idx, f_idx, gamma):
    if omega3 is None and tau3 is not None and omega1 is not None:
        mode, wa, wb, tau = "T3", omega1, omega2, tau3
    elif omega1 is None and tau1 is not None and omega3 is not None:
        mode, wa, wb, tau = "T1", omega2, omega3, tau1
    else:
        raise Exception('Input Error! Please specify either omega1, tau3 or omega3, tau1.')
    if e_idx is None or f_idx is None:
        raise ValueError(f"{which}: e_idx and f_idx must be given")
    name = f"{which}_{mode}"
    return _pathways([name], evals, dip, gamma, 0., g_idx, e_idx, f_idx, tau, wa, wb, which)[0]


def DQC_R1(evals, dip, omega1=None, omega2=[], omega3=None, tau1=None, tau3=None, g_idx=[0], e_idx=None, f_idx=None,
           gamma=None):
    """sos.py:1054-1145, double-quantum coherence gg -> eg -> fg -> fe' -> e'e' (sign -1).  (omega1, omega2, tau3)
    -> [len(omega1), len(omega2)], both Green's functions at omega2 as the reference, so the values of omega1 do not
    enter; (omega2, omega3, tau1) -> [len(omega2), len(omega3)].  Anything else raises the Exception of DQC_R2."""
    return _dqc("DQC_R1", evals, dip, omega1, omega2, omega3, tau1, tau3, g_idx, e_idx, f_idx, gamma)


def DQC_R2(evals, dip, omega1=None, omega2=[], omega3=None, tau1=None, tau3=None, g_idx=[0], e_idx=None, f_idx=None,
           gamma=None):
    """sos.py:1147-1249, gg -> eg -> fg -> eg -> gg (sign +1); layouts as DQC_R1.  The (omega2, omega3, tau1) mode
    carries no -i on its delay factor, as the reference."""
    return _dqc("DQC_R2", evals, dip, omega1, omega2, omega3, tau1, tau3, g_idx, e_idx, f_idx, gamma)


def cars(E, edip, shift, omega1, t2=0, gamma=10 / au2mev):
    """sos.py:1392-1432: S[len(shift), len(omega1)] = sum_{a != b >= 1} mu_bg mu_ag L(shift - (E_b - E_a); gamma) /
    (omega1 - (E_a - E_g) + i gamma) with one scalar gamma; t2 is not used (as in the reference)."""
    E = np.asarray(E).reshape(-1)
    return _pathways(["CARS"], E, edip, np.zeros(E.size), float(gamma), [], [], [], 0., shift, omega1, "cars")[0]


def _tpa(E, dip, omegaps, omega1s, e_idx, f_idx, gamma, second, who):
    E, D, G = _states(E, dip, gamma, who, real_E=True)
    N = E.size
    ei, fi = _index_list(e_idx, N, "e_idx"), _index_list(f_idx, N, "f_idx")
    wp = _grid(omegaps, "omegap")
    w1 = None if omega1s is None else _grid(omega1s, "omega1")
    dev = default_device()
    _lib.ensure_device(dev)
    up = lambda a: torch.from_numpy(a).to(dev)
    Et, Dt, Gt, eit, fit, wpt = (up(a) for a in (E, D, G, ei, fi, wp))
    w1t = None if w1 is None else up(w1)
    n1 = 1 if w1 is None else w1.size
    out = torch.empty((wp.size, n1), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        rc = _lib.load().qd_sos_tpa(Et.data_ptr(), Dt.data_ptr(), Gt.data_ptr(), N,
                                    _lib.ptr(eit) if ei.size else None, ei.size, _lib.ptr(fit) if fi.size else None,
                                    fi.size, wpt.data_ptr(), wp.size, _lib.ptr(w1t), n1, int(second), out.data_ptr(),
                                    _lib.stream_ptr(dev))
    _lib.check(rc, "qd_sos_tpa")
    return out.cpu().numpy()


def TPA(E, dip, omegap, g_idx, e_idx, f_idx, gamma, degenerate=True):
    """sos.py:349-377: degenerate two-photon absorption, omega1 = omega2 = omegap / 2.  A scalar omegap gives a scalar,
    an array an array of its shape.  degenerate=False is refused (the reference leaves omega1 undefined)."""
    if not degenerate:
        raise ValueError('TPA: only the degenerate scan omega1 = omega2 = omegap / 2 is defined.')
    s = _tpa(E, dip, omegap, None, e_idx, f_idx, gamma, 1, "TPA")[:, 0]
    return s[0] if np.ndim(omegap) == 0 else s.reshape(np.shape(omegap))


def TPA2D(E, dip, omegaps, omega1s, g_idx, e_idx, f_idx, gamma):
    """sos.py:380-406: signal [len(omegaps), len(omega1s)] (float64), both time orders."""
    return _tpa(E, dip, omegaps, omega1s, e_idx, f_idx, gamma, 1, "TPA2D")


def TPA2D_time_order(E, dip, omegaps, omega1s, g_idx, e_idx, f_idx, gamma):
    """sos.py:408-433: as TPA2D with the omega1-first time order only."""
    return _tpa(E, dip, omegaps, omega1s, e_idx, f_idx, gamma, 0, "TPA2D_time_order")


def _lorentzian_sum(omegas, centres, weights, widths, who):
    """sum_k weights[k] L(omegas - centres[k]; widths[k]) on the device: each Lorentzian is the two poles
    centres[k] +- i widths[k] with weights -+ i weights[k] / 2 pi (qd_sos_polesum on a one-column grid)."""
    w = _grid(omegas, "omegas")
    c = np.asarray(centres, dtype=float).reshape(-1)
    g = np.broadcast_to(np.asarray(widths, dtype=float), c.shape)
    a = np.asarray(weights, dtype=complex).reshape(-1)
    if a.shape != c.shape:
        raise ValueError(f"{who}: {c.size} transition energies but {a.size} dipoles")
    zx = np.ascontiguousarray(np.concatenate([c + 1j * g, c - 1j * g]))
    W = np.ascontiguousarray(np.concatenate([a, -a]) * (-1j / (2 * np.pi))).reshape(-1, 1)
    dev = default_device()
    _lib.ensure_device(dev)
    zxt, Wt, wt = (torch.from_numpy(x).to(dev) for x in (zx, W, w))
    S = torch.empty(w.size, dtype=torch.complex128, device=dev)
    P = zx.size
    with torch.cuda.device(dev):
        rc = _lib.load().qd_sos_polesum(zxt.data_ptr() if P else None, None, Wt.data_ptr() if P else None, P, 1,
                                        wt.data_ptr(), w.size, None, 1, _SOS_POLE, _SOS_UNITY, S.data_ptr(), 1, 1, 0,
                                        _lib.stream_ptr(dev))
    _lib.check(rc, "qd_sos_polesum")
    return S.cpu().numpy()


def absorption(mol, omegas, linewidth=None, plt_signal=True, fname=None, normalize=False, scale=1., yscale=None):
    """sos.py:192-281: sum_{j >= 1} |edip[j, 0]|^2 L(omegas - (E_j - E_0); linewidth) from mol.edip (not edip_rms),
    linewidth 20 meV by default.  Returns the float64 signal alone (the reference's default also returns a figure)."""
    edip = np.asarray(mol.edip)
    if edip.ndim != 2:
        raise ValueError(f"absorption: mol.edip must be a matrix [N, N], got shape {edip.shape}")
    gamma = 20 / au2mev if linewidth is None else linewidth
    eigenergies = np.asarray(mol.eigvals())
    if np.iscomplexobj(eigenergies):
        if np.any(eigenergies.imag != 0):
            raise ValueError('absorption: complex eigenvalues are not supported, the signal is a real array')
        eigenergies = eigenergies.real
    if not issorted(eigenergies):
        raise ValueError('Eigenenergies are not sorted.')
    eigenergies = eigenergies - eigenergies[0]
    n = mol.nstates
    signal = _lorentzian_sum(omegas, eigenergies[1:n], np.abs(edip[1:n, 0]) ** 2, gamma, "absorption").real.copy()
    signal = signal.reshape(np.shape(omegas))
    if normalize:
        signal /= max(signal)
    return signal


def linear_absorption(omegas, transition_energies, dip, output=None, gamma=1. / au2ev, scale=1, normalize=False):
    """sos.py:283-347: sum_j dip[j]^2 L(omegas - transition_energies[j]; gamma).  Nothing is plotted for `output`."""
    e = np.asarray(transition_energies)
    if np.iscomplexobj(e):
        if np.any(e.imag != 0):
            raise ValueError('linear_absorption: complex transition energies are not supported')
        e = e.real
    d = np.asarray(dip).reshape(-1)
    signal = _lorentzian_sum(omegas, e, d ** 2, gamma, "linear_absorption").reshape(np.shape(omegas))
    if not np.iscomplexobj(d):
        signal = signal.real.copy()
    if normalize:
        signal /= max(signal)
    return signal
