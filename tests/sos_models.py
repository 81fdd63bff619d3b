"""NumPy restatement of the sum-over-states signals (pyqed_amd/sos.py), written from their formulas as einsums over the
index lists.  It is the oracle at shapes tests/golden/sos_signals.npz does not hold; tests/test_sos_signals_host.py
checks it against every entry of that fixture.

Conventions: the initial state is 0; Gamma_uv = (gamma_u + gamma_v) / 2 + dephasing (u != v); the Green's function of
the coherence |u><v| is G_uv(w) = 1 / (w - (E_u - E_v) + i Gamma_uv) and its propagator over a delay t is
U_uv(t) = -i exp(-i (E_u - E_v) t - Gamma_uv t).
"""
import numpy as np

au2ev = 27.2116
au2mev = 27.2116e3


def lorentzian(x, width):
    return width / (np.pi * (width ** 2 + x ** 2))


def _es(*a):
    return np.einsum(*a, optimize=True)


def _idx(x):
    return np.asarray(list(x), dtype=int).reshape(-1)


def _lw(gamma, dephasing, N):
    g = np.asarray(gamma, dtype=float)
    return 0.5 * (g[:, None] + g[None, :]) + dephasing * (1.0 - np.eye(N))


def _omega(E):
    E = np.asarray(E)
    return E[:, None] - E[None, :]


def green(w, E, gamma, rows, cols, dephasing=0.0):
    """G[k, u, v] = 1 / (w_k - (E_u - E_v) + i Gamma_uv) for u in rows, v in cols."""
    N = len(E)
    z = (_omega(E) - 1j * _lw(gamma, dephasing, N))[np.ix_(_idx(rows), _idx(cols))]
    return 1.0 / (np.asarray(w, dtype=float).reshape(-1, 1, 1) - z[None])


def prop(t, E, gamma, rows, cols, dephasing=0.0, retarded=True):
    """U[u, v] = (-i) exp(-i (E_u - E_v) t - Gamma_uv t); retarded=False drops the -i."""
    N = len(E)
    u = np.exp(-1j * _omega(E) * t - _lw(gamma, dephasing, N) * t)[np.ix_(_idx(rows), _idx(cols))]
    return -1j * u if retarded else u


def GSB(E, dip, omega1, omega3, tau2, g_idx, e_idx, gamma):
    D, e = np.asarray(dip), _idx(e_idx)
    Gx = green(omega1, E, gamma, [0], e)[:, 0, :]          # G_ab(omega1), a = 0
    Gy = green(omega3, E, gamma, e, [0])[:, :, 0]          # G_dc(omega3), c = 0
    return _es("b,b,d,d,jd,ib->ji", D[0, e], D[e, 0], D[0, e], D[e, 0], Gy, Gx)


def SE(E, dip, omega1, omega3, tau2, g_idx, e_idx, gamma):
    D, g, e = np.asarray(dip), _idx(g_idx), _idx(e_idx)
    Gx = green(omega1, E, gamma, [0], e)[:, 0, :]
    Gy = green(omega3, E, gamma, e, g)                     # G_cd(omega3)
    U = prop(tau2, E, gamma, e, e)                         # U_cb
    return _es("b,c,dc,bd,jcd,cb,ib->ji", D[0, e], D[e, 0], D[np.ix_(g, e)], D[np.ix_(e, g)], Gy, U, Gx)


def ESA(E, dip, omega1, omega3, tau2, g_idx, e_idx, f_idx, gamma):
    D, e, f = np.asarray(dip), _idx(e_idx), _idx(f_idx)
    Gx = green(omega1, E, gamma, [0], e)[:, 0, :]
    Gy = green(omega3, E, gamma, f, e)                     # G_db(omega3)
    U = prop(tau2, E, gamma, e, e)                         # U_cb
    return -_es("b,c,dc,bd,jdb,cb,ib->ji", D[e, 0], D[e, 0], D[np.ix_(f, e)], D[np.ix_(e, f)], Gy, U, Gx)


def SE_t3(E, dip, omega1, omega2, t3, g_idx, e_idx, gamma, dephasing):
    D, g, e = np.asarray(dip), _idx(g_idx), _idx(e_idx)
    Gx = green(omega1, E, gamma, [0], e, dephasing)[:, 0, :]
    Gy = green(omega2, E, gamma, e, e, dephasing)          # the (c, b) coherence along omega2
    U = prop(t3, E, gamma, e, g, dephasing)                # the (c, d) coherence over t3
    return _es("b,c,dc,bd,cd,jcb,ib->ji", D[0, e], D[e, 0], D[np.ix_(g, e)], D[np.ix_(e, g)], U, Gy, Gx)


def ESA_t3(E, dip, omega1, omega2, t3, g_idx, e_idx, f_idx, gamma, dephasing):
    D, e, f = np.asarray(dip), _idx(e_idx), _idx(f_idx)
    Gx = green(omega1, E, gamma, [0], e, dephasing)[:, 0, :]
    Gy = green(omega2, E, gamma, e, e, dephasing)          # (c, b)
    U = prop(t3, E, gamma, f, e, dephasing)                # (d, b)
    return -_es("b,c,dc,bd,db,jcb,ib->ji", D[e, 0], D[e, 0], D[np.ix_(f, e)], D[np.ix_(e, f)], U, Gy, Gx)


def photon_echo_t3(E, dip, omega1, omega2, t3, g_idx, e_idx, f_idx, gamma, dephasing):
    """(se, esa) of sos.photon_echo_t3: omega1 enters negated."""
    w1 = -np.asarray(omega1, dtype=float)
    return (SE_t3(E, dip, w1, omega2, t3, g_idx, e_idx, gamma, dephasing),
            ESA_t3(E, dip, w1, omega2, t3, g_idx, e_idx, f_idx, gamma, dephasing))


def DQC_R1(E, dip, omega1=None, omega2=(), omega3=None, tau1=None, tau3=None, g_idx=(0,), e_idx=None, f_idx=None,
           gamma=None):
    D, e, f = np.asarray(dip), _idx(e_idx), _idx(f_idx)
    amp = ("b,cb,d,dc", D[e, 0], D[np.ix_(f, e)], D[e, 0], D[np.ix_(e, f)])
    if omega3 is None and tau3 is not None:
        Gb = green(omega2, E, gamma, e, [0])[:, :, 0]      # G_ba at omega2 (not omega1)
        Gc = green(omega2, E, gamma, f, [0])[:, :, 0]
        row = _es(amp[0] + ",jb,jc,cd->j", *amp[1:], Gb, Gc, prop(tau3, E, gamma, f, e))
        return -np.tile(row, (len(omega1), 1))
    Gc = green(omega2, E, gamma, f, [0])[:, :, 0]
    Gcd = green(omega3, E, gamma, f, e)
    return -_es(amp[0] + ",b,ic,jcd->ij", *amp[1:], prop(tau1, E, gamma, e, [0])[:, 0], Gc, Gcd)


def DQC_R2(E, dip, omega1=None, omega2=(), omega3=None, tau1=None, tau3=None, g_idx=(0,), e_idx=None, f_idx=None,
           gamma=None):
    D, e, f = np.asarray(dip), _idx(e_idx), _idx(f_idx)
    amp = ("b,cb,dc,d", D[e, 0], D[np.ix_(f, e)], D[np.ix_(e, f)], D[0, e])
    if omega3 is None and tau3 is not None:
        Gb = green(omega1, E, gamma, e, [0])[:, :, 0]
        Gc = green(omega2, E, gamma, f, [0])[:, :, 0]
        return _es(amp[0] + ",ib,jc,d->ij", *amp[1:], Gb, Gc, prop(tau3, E, gamma, e, [0])[:, 0])
    Gc = green(omega2, E, gamma, f, [0])[:, :, 0]
    Gd = green(omega3, E, gamma, e, [0])[:, :, 0]
    U = prop(tau1, E, gamma, e, [0], retarded=False)[:, 0]  # no -i in this mode
    return _es(amp[0] + ",b,ic,jd->ij", *amp[1:], U, Gc, Gd)


def cars(E, edip, shift, omega1, t2=0, gamma=10 / au2mev):
    E, D = np.asarray(E), np.asarray(edip)
    s = np.arange(1, len(E))
    alpha = 1.0 - np.eye(len(s))
    w_ba = (E[s][:, None] - E[s][None, :])
    L = lorentzian(np.asarray(shift, dtype=float).reshape(-1, 1, 1) - w_ba[None], gamma)
    Ga = 1.0 / (np.asarray(omega1, dtype=float).reshape(-1, 1) - (E[s] - E[0])[None, :] + 1j * gamma)
    return _es("b,a,ba,iba,ja->ij", D[s, 0], D[s, 0], alpha, L, Ga)


def TPA2D(E, dip, omegaps, omega1s, g_idx, e_idx, f_idx, gamma, both=True):
    E, D, gam = np.asarray(E, dtype=float), np.asarray(dip), np.asarray(gamma, dtype=float)
    e, f = _idx(e_idx), _idx(f_idx)
    wp = np.asarray(omegaps, dtype=float).reshape(-1, 1, 1)
    w1 = np.asarray(omega1s, dtype=float).reshape(1, -1, 1)
    em, gm = (E[e] - E[0])[None, None, :], gam[e][None, None, :]
    r = 1.0 / (w1 - em + 1j * gm) + (1.0 / (wp - w1 - em + 1j * gm) if both else 0.0)
    amp = _es("fm,m,ijm->ijf", D[np.ix_(f, e)], D[e, 0], r + 0 * wp)
    L = lorentzian(wp - (E[f] - E[0])[None, None, :], gam[f][None, None, :])
    return _es("ijf,ijf->ij", np.abs(amp) ** 2, L + 0 * w1)


def TPA2D_time_order(E, dip, omegaps, omega1s, g_idx, e_idx, f_idx, gamma):
    return TPA2D(E, dip, omegaps, omega1s, g_idx, e_idx, f_idx, gamma, both=False)


def TPA(E, dip, omegap, g_idx, e_idx, f_idx, gamma):
    wp = np.asarray(omegap, dtype=float).reshape(-1)
    out = np.array([TPA2D(E, dip, [w], [0.5 * w], g_idx, e_idx, f_idx, gamma)[0, 0] for w in wp])
    return out[0] if np.ndim(omegap) == 0 else out.reshape(np.shape(omegap))


def linear_absorption(omegas, transition_energies, dip, gamma=1.0 / au2ev, normalize=False):
    w = np.asarray(omegas, dtype=float)
    e, d = np.asarray(transition_energies, dtype=float), np.asarray(dip)
    s = _es("k,wk->w", d ** 2, lorentzian(w[:, None] - e[None, :], gamma))
    return s / s.max() if normalize else s


def absorption(E, edip, omegas, linewidth=None, normalize=False):
    E, D = np.asarray(E, dtype=float), np.asarray(edip)
    width = 20 / au2mev if linewidth is None else linewidth
    return linear_absorption(omegas, E[1:] - E[0], np.abs(D[1:, 0]), gamma=width, normalize=normalize)
