"""Result container (mirror of pyqed/mol.py:98-171)."""
from __future__ import annotations

import pickle
from dataclasses import dataclass

import numpy as np


class Result:
    """Same fields and `times` convention as pyqed.mol.Result (mol.py:98-119):
    times = t0 + arange(Nt//nout + 1) * dt * nout."""

    def __init__(self, description=None, psi0=None, rho0=None, dt=None, Nt=None, times=None, t0=0, nout=1):
        self.description = description
        self.dt = dt
        self.timesteps = self.nt = Nt
        self.observables = None
        self.rholist = None
        self.psilist = []
        self.psi = None
        self.rho0 = rho0
        self.psi0 = psi0
        self.nout = nout
        self.times = t0 + np.arange(Nt // nout + 1) * dt * nout
        return

    def expect(self):
        return self.observables

    def dump(self, fname):
        """Pickle the result (mol.py:146-162)."""
        with open(fname, "wb") as f:
            pickle.dump(self, f)

    def save(self, fname):
        self.dump(fname)


def load_result(fname):
    """Counterpart of mol.load_result (mol.py:173-179); loads a file this package wrote."""
    with open(fname, "rb") as f:
        return pickle.load(f)


# --------------------------------------------------------------------------- TDSE
def tdse_rk4(H, psi, dt, nsteps, save_every=0, e_ops=None):
    """Batched RK4 of dpsi/dt = -iH psi on the GPU (qd_tdse_rk4).  H [N,N], psi [B,N] (in place),
    e_ops [ne,N,N] (torch complex128, one device).  Returns (snap [B,nsave,N] | None,
    obs [B,nsave+1,ne] | None)."""
    import torch
    from . import _lib
    dev = psi.device
    _lib.ensure_device(dev)
    B, N = psi.shape
    ne = 0 if e_ops is None else e_ops.shape[0]
    nsave = nsteps // save_every if save_every > 0 else 0
    snap = torch.empty((B, nsave, N), dtype=torch.complex128, device=dev) if nsave else None
    obs = torch.empty((B, nsave + 1, ne), dtype=torch.complex128, device=dev) if ne else None
    with torch.cuda.device(dev):
        rc = _lib.load().qd_tdse_rk4(_lib.ptr(H), _lib.ptr(psi), B, N, float(dt), int(nsteps), int(save_every),
                                     _lib.ptr(snap), _lib.ptr(e_ops), ne, _lib.ptr(obs), _lib.stream_ptr(dev))
    _lib.check(rc, "qd_tdse_rk4")
    return snap, obs


def tdse_pair_corr(H, A, Bop, C, psi, dt, ntau):
    """Batched cross correlations on the GPU (qd_tdse_pair_corr): for every row psi_b the ket C psi_b and the bra
    A^dagger psi_b are propagated by the RK4 of tdse_rk4 and corr[b, j] = <bra_b(j)| Bop |ket_b(j)> after j steps,
    j = 0 .. ntau-1.  H, A, Bop, C [N,N], psi [B,N] (read only) torch complex128 on one device.  Returns corr
    [B, ntau]."""
    import torch
    from . import _lib
    dev = psi.device
    _lib.ensure_device(dev)
    B, N = psi.shape
    corr = torch.empty((B, int(ntau)), dtype=torch.complex128, device=dev)
    with torch.cuda.device(dev):
        rc = _lib.load().qd_tdse_pair_corr(_lib.ptr(H), _lib.ptr(A), _lib.ptr(Bop), _lib.ptr(C), _lib.ptr(psi), B, N,
                                           float(dt), int(ntau), _lib.ptr(corr), _lib.stream_ptr(dev))
    _lib.check(rc, "qd_tdse_pair_corr")
    return corr


def tdse_driven_rk4(H0, Hd, fvals, psi, dt, nout, e_ops=None):
    """Laser-driven batched RK4 on the GPU (qd_tdse_driven_rk4): block k of `nout` steps uses
    H0 - sum_d fvals[k, d] Hd[d].  H0 [N,N], Hd [nd,N,N] | None, fvals host complex [nblocks, nd],
    psi [B,N] (in place), e_ops [ne,N,N] | None.  Returns (snap [B,nblocks,N], obs [B,nblocks+1,ne] | None)."""
    import torch
    from . import _lib
    dev = psi.device
    _lib.ensure_device(dev)
    B, N = psi.shape
    fv = np.ascontiguousarray(np.asarray(fvals, dtype=np.complex128))
    nblocks = fv.shape[0]
    nd = 0 if Hd is None else Hd.shape[0]
    ne = 0 if e_ops is None else e_ops.shape[0]
    snap = torch.empty((B, nblocks, N), dtype=torch.complex128, device=dev) if nblocks else None
    obs = torch.empty((B, nblocks + 1, ne), dtype=torch.complex128, device=dev) if ne else None
    with torch.cuda.device(dev):
        rc = _lib.load().qd_tdse_driven_rk4(_lib.ptr(H0), _lib.ptr(Hd), nd, fv.ctypes.data if fv.size else None,
                                            _lib.ptr(psi), B, N, float(dt), nblocks, int(nout), _lib.ptr(snap),
                                            _lib.ptr(e_ops), ne, _lib.ptr(obs), _lib.stream_ptr(dev))
        torch.cuda.current_stream(dev).synchronize()  # fvals is a host buffer read asynchronously
    _lib.check(rc, "qd_tdse_driven_rk4")
    return snap, obs


def driven_dynamics(H, psi0, dt=0.01, Nt=1, e_ops=None, nout=1, t0=0.0, return_result=True, use_sparse=True):
    """mol.py:1862-1958.  H = [H0, [Hd_1, f_1], [Hd_2, f_2], ...] with H(t) = H0 - sum_d f_d(t) Hd_d,
    evaluated once per block of nout steps at the block's start time (calcH(t), t advanced by
    dt*nout after each block).  return_result=True: Nt//nout - 1 blocks; psilist = [psi0] + the
    state after each block (csr columns when use_sparse, as the reference's sparse psi);
    observables (Nt//nout, n_e) including t0; result.psi = psit [nstates, Nt//nout].
    return_result=False: int(Nt/nout) blocks written to psi.dat / obs.dat (t after the block,
    then the values; dense formatting)."""
    import torch
    from scipy.sparse import csr_matrix
    from ._util import default_device, stack_ops, to_numpy
    if e_ops is None:
        e_ops = []
    dev = default_device()
    H0 = to_numpy(H[0], np.complex128)
    N = H0.shape[0]
    drives = H[1:]
    Hd = [to_numpy(h[0], np.complex128) for h in drives]
    p0 = to_numpy(psi0, np.complex128).reshape(N)
    nblocks = max(Nt // nout - 1, 0) if return_result else int(Nt / nout)
    fvals = np.array([[complex(f(t0 + k * dt * nout)) for (_, f) in drives] for k in range(nblocks)],
                     dtype=np.complex128).reshape(nblocks, len(drives))
    psi = torch.from_numpy(p0.copy()).to(dev).reshape(1, N)
    Hdt = torch.from_numpy(np.ascontiguousarray(np.array(Hd))).to(dev) if Hd else None
    Ed = stack_ops(e_ops, N, dev)
    snap, obs = tdse_driven_rk4(torch.from_numpy(np.ascontiguousarray(H0)).to(dev), Hdt, fvals, psi, dt, nout,
                                e_ops=Ed)
    states = snap[0].cpu().numpy() if snap is not None else np.zeros((0, N), complex)
    o = obs[0].cpu().numpy() if obs is not None else np.zeros((nblocks + 1, 0), complex)
    if not return_result:
        with open("psi.dat", "w") as f_dm, open("obs.dat", "w") as f_obs:
            fmt = "{} " * (len(e_ops) + 1) + "\n"
            fmt_dm = "{} " * (N + 1) + "\n"
            for k in range(nblocks):
                t = t0 + (k + 1) * dt * nout
                f_dm.write(fmt_dm.format(t, *states[k]))
                f_obs.write(fmt.format(t, *o[k + 1]))
        return None
    result = Result(dt=dt, Nt=Nt, psi0=psi0, t0=t0, nout=nout)
    nrec = Nt // nout
    observables = np.zeros((nrec, len(e_ops)), dtype=complex)
    observables[:nblocks + 1] = o[:nrec]
    psit = np.zeros((N, nrec), dtype=complex)
    psit[:, 0] = p0
    psilist = [np.array(psi0, copy=True)]
    for k in range(nblocks):
        psit[:, k + 1] = states[k]
        psilist.append(csr_matrix(states[k].reshape(N, 1)) if use_sparse else states[k].copy())
    result.psilist = psilist
    result.psi = psit
    result.observables = observables
    return result


def _driven_dynamics(H, psi0, edip, E, dt=0.001, Nt=1, e_ops=None, nout=1, t0=0.0, sparse=True):
    """mol.py:1772-1859: full vector dipole edip [N, N, 3] in a polarized field E(t) -> 3-vector,
    H(t) = H - einsum('ija, a -> ij', edip, E(t)), held for each block of nout RK4 steps at the block's start time
    (t advanced by dt*nout after a block); Nt//nout - 1 blocks.  On the GPU this is qd_tdse_driven_rk4 with the
    three dipole components as drives.  As the reference: result.psilist holds only the states after each block
    (csr columns), observables (Nt//nout, n_e) include t0, result.psi = psit [nstates, Nt//nout].  The reference's
    sparse=False branch never defines psi and raises; only the sparse (default) arithmetic exists."""
    import torch
    from scipy.sparse import csr_matrix
    from ._util import default_device, stack_ops, to_numpy
    if not sparse:
        raise NotImplementedError("_driven_dynamics(sparse=False): the reference's dense branch never sets psi")
    if e_ops is None:
        e_ops = []
    dev = default_device()
    H0 = to_numpy(H, np.complex128)
    N = H0.shape[0]
    ed = np.asarray(to_numpy(edip, np.complex128))
    if ed.shape[:2] != (N, N) or ed.ndim != 3:
        raise ValueError(f"edip must be [N, N, ncomp] with N = {N}, got {ed.shape}")
    nc = ed.shape[2]
    p0 = to_numpy(psi0, np.complex128).reshape(N)
    nblocks = max(Nt // nout - 1, 0)
    fvals = np.zeros((nblocks, nc), dtype=np.complex128)
    for k in range(nblocks):
        fvals[k] = np.asarray(E(t0 + k * dt * nout), dtype=np.complex128).reshape(nc)
    psi = torch.from_numpy(p0.copy()).to(dev).reshape(1, N)
    Hdt = torch.from_numpy(np.ascontiguousarray(np.moveaxis(ed, 2, 0))).to(dev)
    Ed = stack_ops(e_ops, N, dev)
    snap, obs = tdse_driven_rk4(torch.from_numpy(np.ascontiguousarray(H0)).to(dev), Hdt, fvals, psi, dt, nout,
                                e_ops=Ed)
    states = snap[0].cpu().numpy() if snap is not None else np.zeros((0, N), complex)
    nrec = Nt // nout
    result = Result(dt=dt, Nt=Nt, psi0=psi0, t0=t0, nout=nout)
    observables = np.zeros((nrec, len(e_ops)), dtype=complex)
    if obs is not None:
        o = obs[0].cpu().numpy()
        observables[:nblocks + 1] = o[:nrec]
    psit = np.zeros((N, nrec), dtype=complex)
    if nrec:
        psit[:, 0] = p0
    for k in range(nblocks):
        psit[:, k + 1] = states[k]
    result.psilist = [csr_matrix(states[k].reshape(N, 1)) for k in range(nblocks)]
    result.psi = psit
    result.observables = observables
    return result


def _quantum_dynamics(H, psi0, dt=0.001, Nt=1, e_ops=[], t0=0.0, nout=1, store_states=True, output='obs.dat'):
    """mol.py:1603-1691 (store_states=True): (Nt//nout - 1)*nout RK4 steps; psilist = [psi0] + the
    state after every nout steps; observables (Nt//nout, n_e) at those states."""
    import torch
    from ._util import default_device, stack_ops, to_numpy
    if e_ops is None:
        e_ops = []
    dev = default_device()
    Hn = to_numpy(H, np.complex128)
    N = Hn.shape[0]
    p0 = to_numpy(psi0, np.complex128).reshape(N)
    nblk = Nt // nout
    nsteps = max(nblk - 1, 0) * nout
    psi = torch.from_numpy(p0.copy()).to(dev).reshape(1, N)
    Ed = stack_ops(e_ops, N, dev)
    snap, obs = tdse_rk4(torch.from_numpy(np.ascontiguousarray(Hn)).to(dev), psi, dt, nsteps,
                         save_every=nout, e_ops=Ed)
    result = Result(dt=dt, Nt=Nt, psi0=psi0, t0=t0, nout=nout)
    result.psilist = [p0.copy()]
    if snap is not None:
        host = snap[0].cpu().numpy()
        result.psilist += [host[k] for k in range(host.shape[0])]
    observables = np.zeros((nblk, len(e_ops)), dtype=complex)
    if obs is not None:
        o = obs[0].cpu().numpy()
        observables[:o.shape[0]] = o[:nblk]
    result.observables = observables
    result.psi = psi[0].cpu().numpy()
    return result


def _check_corr_args(name, oplist, nops, **counts):
    """Argument checks of the SESolver correlation functions, before any device work."""
    if len(oplist) != nops:
        raise ValueError(f"{name}: oplist must hold {nops} operators, got {len(oplist)}")
    for k, v in counts.items():
        if int(v) < 1:
            raise ValueError(f"{name}: {k} must be >= 1, got {v}")


def _propagator(H, dt, Nt):
    """mol.py:1569-1600, rk4 branch: [I, I, R, R^2, ..., R^(Nt-1)] with R the one-step RK4 map (the reference appends
    U before it steps, so the identity comes twice).  The columns of U are one tdse_rk4 batch of N wavefunctions
    with a snapshot after every step."""
    import torch
    from ._util import default_device, to_numpy
    if int(Nt) < 0:
        raise ValueError(f"propagator: Nt must be >= 0, got {Nt}")
    Hn = to_numpy(H, np.complex128)
    N = Hn.shape[-1]
    Ulist = [np.eye(N, dtype=complex)]
    if Nt >= 1:
        Ulist.append(np.eye(N, dtype=complex))
    if Nt >= 2:
        dev = default_device()
        psi = torch.eye(N, dtype=torch.complex128, device=dev)
        snap, _ = tdse_rk4(torch.from_numpy(np.ascontiguousarray(Hn)).to(dev), psi, dt, Nt - 1, save_every=1)
        host = snap.cpu().numpy()   # [b, k, :] = R^(k+1) e_b: column b of R^(k+1)
        Ulist += [np.ascontiguousarray(host[:, k, :].T) for k in range(Nt - 1)]
    return Ulist


class SESolver:
    """Drop-in for pyqed.mol.SESolver (mol.py:1369-1566), time-independent H."""

    def __init__(self, H=None):
        self.H = H
        self.groundstate = None

    def propagator(self, dt, Nt):
        """mol.py:1468-1470: list of Nt + 1 dense N x N arrays [I, I, R, ..., R^(Nt-1)]."""
        return _propagator(self.H, dt, Nt)

    def _corr_3op(self, psi_t, oplist, dt, ntau):
        """corr [B, ntau] of the states psi_t [B, N] (device) for [a, b, c] = oplist: one qd_tdse_pair_corr."""
        import torch
        from ._util import to_numpy
        dev = psi_t.device
        N = psi_t.shape[1]
        ops = []
        for i, op in enumerate(oplist):
            a = to_numpy(op, np.complex128)
            if a.shape != (N, N):
                raise ValueError(f"operator {i} has shape {a.shape}, expected {(N, N)}")
            ops.append(torch.from_numpy(np.ascontiguousarray(a)).to(dev))
        H = torch.from_numpy(np.ascontiguousarray(to_numpy(self.H, np.complex128))).to(dev)
        return tdse_pair_corr(H, ops[0], ops[1], ops[2], psi_t, dt, ntau).cpu().numpy()

    def correlation_3op_1t(self, psi0, oplist, dt, Nt):
        """<A B(t) C> at t = 0 .. (Nt-1) dt (mol.py:1475-1501): complex ndarray (Nt,)."""
        import torch
        from ._util import default_device, to_numpy
        _check_corr_args("correlation_3op_1t", oplist, 3, Nt=Nt)
        p0 = to_numpy(psi0, np.complex128).reshape(1, -1)
        psi = torch.from_numpy(np.ascontiguousarray(p0)).to(default_device())
        return self._corr_3op(psi, oplist, dt, int(Nt))[0]

    def correlation_3op_2t(self, psi0, oplist, dt, Nt, Ntau):
        """<A(t) B(t+tau) C(t)> (mol.py:1503-1536): complex ndarray (Nt, Ntau), t_i = i dt, tau_j = j dt.  The Nt
        states psi(t_i) come from one tdse_rk4 run and stay on the device; their 2 Nt kets and bras are one batch."""
        import torch
        from ._util import default_device, to_numpy
        _check_corr_args("correlation_3op_2t", oplist, 3, Nt=Nt, Ntau=Ntau)
        dev = default_device()
        p0 = to_numpy(psi0, np.complex128).reshape(1, -1)
        psi = torch.from_numpy(p0.copy()).to(dev)
        psi_t = psi.clone()
        if Nt > 1:
            H = torch.from_numpy(np.ascontiguousarray(to_numpy(self.H, np.complex128))).to(dev)
            snap, _ = tdse_rk4(H, psi, dt, int(Nt) - 1, save_every=1)
            psi_t = torch.cat([psi_t, snap[0]], dim=0).contiguous()
        return self._corr_3op(psi_t, oplist, dt, int(Ntau))

    def correlation_4op_1t(self, psi0, oplist, dt=0.005, Nt=1):
        """<A B(t) C(t) D> (mol.py:1538-1554): the 3-operator form with [a, b @ c, d]."""
        _check_corr_args("correlation_4op_1t", oplist, 4, Nt=Nt)
        a_op, b_op, c_op, d_op = oplist
        return self.correlation_3op_1t(psi0, [a_op, b_op @ c_op, d_op], dt, Nt)

    def correlation_4op_2t(self, psi0, oplist, dt=0.005, Nt=1, Ntau=1):
        """<A(t) B(t+tau) C(t+tau) D(t)> (mol.py:1556-1566): the 3-operator form with [a, b @ c, d]."""
        _check_corr_args("correlation_4op_2t", oplist, 4, Nt=Nt, Ntau=Ntau)
        a_op, b_op, c_op, d_op = oplist
        return self.correlation_3op_2t(psi0, [a_op, b_op @ c_op, d_op], dt, Nt, Ntau)

    def run(self, psi0=None, dt=0.01, Nt=1, e_ops=None, nout=1, t0=0.0, edip=None, pulse=None, use_sparse=True):
        """mol.py:1392-1459: time-independent H -> _quantum_dynamics; with a pulse (or a list of
        pulses with a list of dipoles) -> driven_dynamics, H(t) = H - sum_i f_i(t) edip_i; a full [N, N, 3]
        dipole with a single pulse -> _driven_dynamics with the pulse's vector field pulse.E(t)."""
        if psi0 is None:
            psi0 = self.groundstate
        if pulse is None:
            return _quantum_dynamics(self.H, psi0, dt=dt, Nt=Nt, e_ops=e_ops, nout=nout, t0=t0)
        if edip is None:
            raise ValueError('Electric dipole must be provided for laser-driven dynamics.')
        if isinstance(pulse, list):
            H = [self.H] + [[edip[i], pulse[i].efield] for i in range(len(pulse))]
            return driven_dynamics(H=H, psi0=psi0, dt=dt, Nt=Nt, e_ops=e_ops, nout=nout, t0=t0)
        if np.ndim(edip) == 2:
            return driven_dynamics(H=[self.H, [edip, pulse.efield]], psi0=psi0, dt=dt, Nt=Nt, e_ops=e_ops,
                                   nout=nout, t0=t0, use_sparse=use_sparse)
        if np.ndim(edip) == 3:
            return _driven_dynamics(H=self.H, psi0=psi0, edip=edip, E=pulse.E, dt=dt, Nt=Nt, e_ops=e_ops, nout=nout,
                                    t0=t0)
        return None


class Mol:
    """Subset of pyqed.mol.Mol (mol.py:184-957) on the hot path: container, run, and the sum-over-states signals
    (photon_echo / PE, PE2, absorption, cars) with the setters of their decay and dephasing rates."""

    def __init__(self, H, edip=None, lowering=None, edip_rms=None, gamma=None):
        self.H = H
        self.h = H
        Hd = np.asarray(H.toarray() if hasattr(H, "toarray") else H)
        self.E = np.diag(Hd) if np.count_nonzero(Hd - np.diag(np.diagonal(Hd))) == 0 else None
        self.nonhermH = None
        self._edip = edip
        self.dip = self.edip = edip
        if lowering is not None:
            self.lowering = lowering
            self.raising = np.conj(np.transpose(lowering))
        self.nstates = self.dim = self.size = H.shape[0]
        self.gamma = gamma
        self.mdip = None
        self.dephasing = 0.
        self._edip_rms = edip_rms

    @property
    def edip(self):
        return self._edip

    @edip.setter
    def edip(self, edip):
        self._edip = edip

    def set_dipole(self, dip):
        self.dip = dip

    def set_edip(self, edip, pol=None):
        self.edip_rms = edip

    @property
    def edip_rms(self):
        if self._edip_rms is None:
            self._edip_rms = np.sqrt(np.abs(self.edip[:, :, 0]) ** 2 + np.abs(self.edip[:, :, 1]) ** 2 +
                                     np.abs(self.edip[:, :, 2]) ** 2)
        return self._edip_rms

    @edip_rms.setter
    def edip_rms(self, edip):
        self._edip_rms = edip

    def run(self, psi0=None, dt=0.01, e_ops=None, nt=1, nout=1, t0=0.0, edip=None, pulse=None):
        """mol.py:628-674: _quantum_dynamics, or driven_dynamics with H(t) = H - f(t) edip for a pulse
        (self.edip is used, as in the reference; a list of pulses pairs with a list of dipoles)."""
        if psi0 is None:
            raise ValueError("Please specify initial wavefunction psi0.")
        if pulse is None:
            return _quantum_dynamics(self.H, psi0, dt=dt, Nt=nt, e_ops=e_ops, nout=nout, t0=t0)
        edip = self.edip
        if isinstance(pulse, list):
            H = [self.H] + [[edip[i], pulse[i].efield] for i in range(len(pulse))]
        else:
            H = [self.H, [edip, pulse.efield]]
        return driven_dynamics(H, psi0, dt=dt, Nt=nt, e_ops=e_ops, nout=nout, t0=t0)

    def eigvals(self):
        """mol.py:459-463."""
        H = np.asarray(self.H.toarray() if hasattr(self.H, "toarray") else self.H)
        if np.count_nonzero(H - np.diag(np.diagonal(H))) == 0:
            return np.diagonal(H)
        return np.linalg.eigvals(H)

    def photon_echo(self, pump, probe, t2=0.0, **kwargs):
        """mol.py:804-829 -> sos.photon_echo (GPU)."""
        from . import sos
        return sos.photon_echo(self, pump=pump, probe=probe, t2=t2, **kwargs)

    def PE(self, pump, probe, t2=0.0, **kwargs):
        """mol.py:797-802: alias for photon_echo."""
        return self.photon_echo(pump, probe, t2=t2, **kwargs)

    def PE2(self, omega1, omega2, t3=0.0, **kwargs):
        """mol.py:831-855 -> sos.photon_echo_t3 (GPU): the echo on (omega1, omega2) at detection time t3."""
        from . import sos
        return sos.photon_echo_t3(self, omega1=omega1, omega2=omega2, t3=t3, **kwargs)

    def absorption(self, omegas, method='sos', **kwargs):
        """mol.py:766-795 -> sos.absorption (GPU); the array alone is returned, nothing plots."""
        if method == 'sos':
            from . import sos
            return sos.absorption(self, omegas, **kwargs)
        elif method == 'tcf':
            raise NotImplementedError('The method {} has not been implemented. \
                              Try "sos"'.format(method))

    def cars(self, shift, omega1, t2=0., plt_signal=False, fname=None):
        """mol.py:866-888 -> sos.cars (GPU) with edip_rms; plt_signal is accepted and ignored."""
        from . import sos
        return sos.cars(self.eigvals(), self.edip_rms, shift, omega1, t2=t2)

    def set_decay_for_all(self, gamma):
        """mol.py:363-379: one decay rate for every excited state, 0 for the ground state."""
        self.gamma = [gamma] * self.nstates
        self.gamma[0] = 0
        return

    def set_dephasing(self, gamma):
        """mol.py:381-395: the pure dephasing rate of all coherences (read by PE2)."""
        self.dephasing = gamma

    def set_decay(self, gamma):
        """mol.py:397-412: the decay rates of the states."""
        self.gamma = gamma
        return


# --------------------------------------------------------------------------- LVC
LVC_PATHS = {"auto": 0, "staged": 1, "resident": 2}


def _lvc_arrays(dims, omega):
    d = np.ascontiguousarray(np.asarray(dims, dtype=np.intc).reshape(-1))
    w = np.ascontiguousarray(np.asarray(omega, dtype=np.float64).reshape(-1))
    if d.size != w.size:
        raise ValueError(f"lvc: {d.size} dims but {w.size} frequencies")
    return d, w


def lvc_apply(psi, nel, dims, omega, Hel, W):
    """out [B, D] = H psi [B, D] of the LVC model on the GPU (qd_lvc_apply).  Hel [nel, nel], W [M, nel, nel] and psi
    torch complex128 on one device; dims and omega host sequences."""
    import torch
    from . import _lib
    dev = psi.device
    _lib.ensure_device(dev)
    d, w = _lvc_arrays(dims, omega)
    out = torch.empty_like(psi)
    with torch.cuda.device(dev):
        rc = _lib.load().qd_lvc_apply(_lib.ptr(psi), _lib.ptr(out), psi.shape[0], int(nel), d.size, d.ctypes.data,
                                      w.ctypes.data, _lib.ptr(Hel), _lib.ptr(W), _lib.stream_ptr(dev))
    _lib.check(rc, "qd_lvc_apply")
    return out


def lvc_nobs(nel, M):
    return nel * nel * (1 + M) + M


def lvc_rk4(psi, nel, dims, omega, Hel, W, dt, nsteps, save_every=0, store=True, observe=True, path="auto",
            snap=None, obs=None):
    """Batched matrix-free RK4 of the LVC model on the GPU (qd_lvc_rk4): psi [B, D] in place.  Returns
    (snap [B, nsave, D] | None, obs [B, nsave + 1, nobs] | None) with nsave = nsteps // save_every; store=False keeps
    no snapshots, observe=False no records.  path: "auto", "staged" or "resident".  snap and obs may be passed in
    (a graph capture replays into the same buffers)."""
    import torch
    from . import _lib
    dev = psi.device
    _lib.ensure_device(dev)
    d, w = _lvc_arrays(dims, omega)
    B = psi.shape[0]
    nsave = nsteps // save_every if save_every > 0 else 0
    if snap is None and store and nsave:
        snap = torch.empty((B, nsave, psi.shape[1]), dtype=torch.complex128, device=dev)
    if obs is None and observe:
        obs = torch.empty((B, nsave + 1, lvc_nobs(int(nel), d.size)), dtype=torch.complex128, device=dev)
    with torch.cuda.device(dev):
        rc = _lib.load().qd_lvc_rk4(_lib.ptr(psi), B, int(nel), d.size, d.ctypes.data, w.ctypes.data, _lib.ptr(Hel),
                                    _lib.ptr(W), float(dt), int(nsteps), int(save_every), _lib.ptr(snap),
                                    _lib.ptr(obs), LVC_PATHS[path], _lib.stream_ptr(dev))
    _lib.check(rc, "qd_lvc_rk4")
    return snap, obs


LVC_SAMPLES = {"hold": 0, "stage": 1}


def lvc_driven_rk4(psi, nel, dims, omega, Hel, W, A, modes, fvals, dt, nsteps, hold=1, sample="hold", save_every=0,
                   store=True, observe=True, path="auto", snap=None, obs=None):
    """Laser-driven lvc_rk4 (qd_lvc_driven_rk4): H(t) = H0 - sum_d f_d(t) A_d (x) (1 | x_j).  A [nd, nel, nel] and fvals
    [nf, nd] torch complex128 on psi's device (None with no drive), modes [nd] host integers, -1 (or None) for A (x) 1 and
    j for A (x) x_j.  sample "hold": step s takes row s // hold of fvals (the Horner step of lvc_rk4); "stage": classical
    RK4, row h is f(t0 + h dt / 2) and step s takes rows 2s, 2s + 1, 2s + 2.  fvals is read when the kernels run: the
    call is asynchronous.  Everything else as lvc_rk4."""
    import torch
    from . import _lib
    if sample not in LVC_SAMPLES:
        raise ValueError(f"lvc_driven_rk4: sample={sample!r}, expected 'hold' or 'stage'")
    dev = psi.device
    _lib.ensure_device(dev)
    d, w = _lvc_arrays(dims, omega)
    md = np.ascontiguousarray(np.array([-1 if k is None else int(k) for k in ([] if modes is None else modes)],
                                       dtype=np.intc))
    nd = md.size
    if nd and (A is None or fvals is None or A.shape[0] != nd or fvals.shape[-1] != nd):
        raise ValueError(f"lvc_driven_rk4: {nd} drive modes need A [{nd}, nel, nel] and fvals [nf, {nd}]")
    B = psi.shape[0]
    nsave = nsteps // save_every if save_every > 0 else 0
    if snap is None and store and nsave:
        snap = torch.empty((B, nsave, psi.shape[1]), dtype=torch.complex128, device=dev)
    if obs is None and observe:
        obs = torch.empty((B, nsave + 1, lvc_nobs(int(nel), d.size)), dtype=torch.complex128, device=dev)
    with torch.cuda.device(dev):
        rc = _lib.load().qd_lvc_driven_rk4(_lib.ptr(psi), B, int(nel), d.size, d.ctypes.data, w.ctypes.data,
                                           _lib.ptr(Hel), _lib.ptr(W), nd, _lib.ptr(A) if nd else None,
                                           md.ctypes.data if nd else None, _lib.ptr(fvals) if nd else None,
                                           int(fvals.shape[0]) if nd else 0, LVC_SAMPLES[sample], int(hold), float(dt),
                                           int(nsteps), int(save_every), _lib.ptr(snap), _lib.ptr(obs),
                                           LVC_PATHS[path], _lib.stream_ptr(dev))
    _lib.check(rc, "qd_lvc_driven_rk4")
    return snap, obs


def lvc_observe(psi, nel, dims):
    """The observable records [B, nobs] of the states psi [B, D] (qd_lvc_observe): rho [nel, nel], X[j] [nel, nel] for
    every mode, nbar [M]."""
    import torch
    from . import _lib
    dev = psi.device
    _lib.ensure_device(dev)
    d = np.ascontiguousarray(np.asarray(dims, dtype=np.intc).reshape(-1))
    obs = torch.empty((psi.shape[0], lvc_nobs(int(nel), d.size)), dtype=torch.complex128, device=dev)
    with torch.cuda.device(dev):
        rc = _lib.load().qd_lvc_observe(_lib.ptr(psi), psi.shape[0], int(nel), d.size, d.ctypes.data, _lib.ptr(obs),
                                        _lib.stream_ptr(dev))
    _lib.check(rc, "qd_lvc_observe")
    return obs


def _lvc_blocks(blocks):
    b = np.ascontiguousarray(np.asarray(blocks, dtype=np.intc).reshape(-1))
    if b.size < 1:
        raise ValueError("lvc: at least one block is needed")
    return b


def lvc_pair_observe(psi, nel, dims, blocks):
    """The pair records rec [P, nblk, nel, nel] of the pairs psi [P, 2, D] (ket, bra) (qd_lvc_pair_observe): block r is
    R_r[a, b] = sum_n L_r[a, n] conj(bra[b, n]) with L_0 = ket and L_{j+1} = x_j ket, so <bra| A (x) 1 |ket> = tr(A R_0)
    and <bra| A (x) x_j |ket> = tr(A R_{j+1}).  blocks: host integers in [0, M]."""
    import torch
    from . import _lib
    b = _lvc_blocks(blocks)
    dev = psi.device
    _lib.ensure_device(dev)
    d = np.ascontiguousarray(np.asarray(dims, dtype=np.intc).reshape(-1))
    if psi.dim() != 3 or psi.shape[1] != 2:
        raise ValueError(f"lvc_pair_observe: psi must be [P, 2, D], got {tuple(psi.shape)}")
    rec = torch.empty((psi.shape[0], b.size, int(nel), int(nel)), dtype=torch.complex128, device=dev)
    with torch.cuda.device(dev):
        rc = _lib.load().qd_lvc_pair_observe(_lib.ptr(psi), psi.shape[0], int(nel), d.size, d.ctypes.data, b.size,
                                             b.ctypes.data, _lib.ptr(rec), _lib.stream_ptr(dev))
    _lib.check(rc, "qd_lvc_pair_observe")
    return rec


def lvc_pair_rk4(psi, nel, dims, omega, Hel, W, dt, nsteps, save_every=1, blocks=(0,), path="auto", rec=None):
    """lvc_rk4 of both states of the pairs psi [P, 2, D] in place with the pair record of lvc_pair_observe at t0 and
    after every save_every steps (qd_lvc_pair_rk4).  Returns rec [P, nsteps // save_every + 1, nblk, nel, nel]; rec may
    be passed in (a graph capture replays into the same buffer).  path: "auto", "staged" or "resident"."""
    import torch
    from . import _lib
    dev = psi.device
    _lib.ensure_device(dev)
    d, w = _lvc_arrays(dims, omega)
    b = _lvc_blocks(blocks)
    if psi.dim() != 3 or psi.shape[1] != 2:
        raise ValueError(f"lvc_pair_rk4: psi must be [P, 2, D], got {tuple(psi.shape)}")
    nsave = nsteps // save_every if save_every > 0 else 0
    if rec is None:
        rec = torch.empty((psi.shape[0], nsave + 1, b.size, int(nel), int(nel)), dtype=torch.complex128, device=dev)
    with torch.cuda.device(dev):
        rc = _lib.load().qd_lvc_pair_rk4(_lib.ptr(psi), psi.shape[0], int(nel), d.size, d.ctypes.data, w.ctypes.data,
                                         _lib.ptr(Hel), _lib.ptr(W), float(dt), int(nsteps), int(save_every), b.size,
                                         b.ctypes.data, _lib.ptr(rec), LVC_PATHS[path], _lib.stream_ptr(dev))
    _lib.check(rc, "qd_lvc_pair_rk4")
    return rec


def _jump(f, i, dim, isherm=True):
    """phys.py:513-525 as a dense array: |f><i| (+ |i><f| when isherm), one diagonal entry for f == i."""
    A = np.zeros((dim, dim))
    A[f, i] = 1.0
    if isherm:
        A[i, f] = 1.0
    return A


def _x_sparse(N):
    """(a + a^+)/sqrt 2 truncated to N levels (phys.quadrature), csr."""
    from scipy.sparse import diags
    c = np.sqrt(np.arange(1, N) / 2.0)
    return diags([c, c], [1, -1], shape=(N, N), format="csr")


@dataclass
class Mode:
    """pyqed.mol.Mode (mol.py:952-956): couplings is a list of [[a, b], strength]."""
    omega: float
    couplings: list
    truncate: int = 2


class LVCOp:
    """An operator of the LVC product space held as factors: A (x) 1 (mode None) or A (x) x_j (mode j), A [nel, nel].
    What LVC.buildop, LVC.coordinate and LVC.promote(A, 'el') return; LVCSolver.run reads its expectation value from the
    on-device record (tr(A rho) or tr(A X[j])) instead of applying a D x D matrix."""
    __array_ufunc__ = None   # ndarray @ LVCOp comes to __rmatmul__

    def __init__(self, A, dims, mode=None):
        self.A = np.array(A.toarray() if hasattr(A, "toarray") else A, dtype=complex)
        self.nel = self.A.shape[0]
        self.dims = tuple(int(d) for d in dims)
        self.mode = mode
        if self.A.shape != (self.nel, self.nel):
            raise ValueError(f"LVCOp: electronic factor must be square, got {self.A.shape}")
        if mode is not None and not 0 <= mode < len(self.dims):
            raise ValueError(f"LVCOp: mode {mode} outside [0, {len(self.dims)})")
        D = self.nel * int(np.prod(self.dims, dtype=np.int64))
        self.shape = (D, D)

    def tocsr(self):
        from scipy.sparse import csr_matrix, identity, kron
        out = csr_matrix(self.A)
        for j, N in enumerate(self.dims):
            out = kron(out, _x_sparse(N) if j == self.mode else identity(N, format="csr"), format="csr")
        return out

    def toarray(self):
        return self.tocsr().toarray()

    def dot(self, other):
        from scipy.sparse import issparse
        if isinstance(other, LVCOp):
            if other.dims != self.dims or other.nel != self.nel:
                raise ValueError("LVCOp: product of operators on different spaces")
            if self.mode is None or other.mode is None:
                return LVCOp(self.A @ other.A, self.dims, self.mode if other.mode is None else other.mode)
            return self.tocsr() @ other.tocsr()
        if issparse(other):
            return self.tocsr() @ other
        v = np.asarray(other)
        if v.shape[0] != self.shape[0]:
            raise ValueError(f"LVCOp: operand has {v.shape[0]} rows, expected {self.shape[0]}")
        g = v.reshape((self.nel,) + self.dims + v.shape[1:])
        if self.mode is not None:
            ax, N = 1 + self.mode, self.dims[self.mode]
            c = np.sqrt(np.arange(1, N) / 2.0).reshape([N - 1 if k == ax else 1 for k in range(g.ndim)])
            lo = tuple(slice(0, N - 1) if k == ax else slice(None) for k in range(g.ndim))
            hi = tuple(slice(1, N) if k == ax else slice(None) for k in range(g.ndim))
            t = np.zeros(g.shape, dtype=np.result_type(g.dtype, float))
            t[hi] += c * g[lo]
            t[lo] += c * g[hi]
            g = t
        return np.tensordot(self.A, g, axes=(1, 0)).reshape(v.shape)

    def __matmul__(self, other):
        return self.dot(other)

    def __rmatmul__(self, other):
        return other @ self.tocsr()

    def from_record(self, rho, X):
        """<psi| op |psi> from the records rho [.., nel, nel] and X [.., M, nel, nel]."""
        R = rho if self.mode is None else X[..., self.mode, :, :]
        return np.einsum("ab,...ba->...", self.A, R)


class LVC:
    """Linear vibronic coupling model in Fock space: drop-in for pyqed.mol.LVC (mol.py:959-1293).  The Hamiltonian is
    never needed as a matrix for a run: wavepacket_dynamics() returns an LVCSolver that applies it matrix-free on the
    GPU.  Where the reference's paths are broken we serve the evident intent: per-mode truncations
    are honoured in buildH, one mode works, and 1 <= nel <= 8 states with 1 <= M <= 6 modes are taken; anything outside
    raises ValueError."""

    def __init__(self, E, modes):
        E = list(np.asarray(E).reshape(-1))
        modes = list(modes)
        if not 1 <= len(E) <= 8:
            raise ValueError(f"LVC: {len(E)} electronic states, 1 to 8 are supported")
        if not 1 <= len(modes) <= 6:
            raise ValueError(f"LVC: {len(modes)} modes, 1 to 6 are supported")
        self.e_fc = E
        self.nel = self.nstates = len(E)
        self.nmodes = len(modes)
        self.modes = modes
        self.truncate = None
        self.fock_dims = [int(m.truncate) for m in modes]
        for j, N in enumerate(self.fock_dims):
            if N < 1:
                raise ValueError(f"LVC: mode {j} is truncated to {N} levels, at least 1 is needed")
        self.nvib = int(np.prod(self.fock_dims, dtype=object))
        self.dim = self.nel * self.nvib
        if self.dim >= 2 ** 31:
            raise ValueError(f"LVC: D = nel * prod(truncations) = {self.dim} must stay below 2^31")
        for j, m in enumerate(modes):
            for c in m.couplings:
                a, b = c[0]
                if not (0 <= a < self.nel and 0 <= b < self.nel):
                    raise ValueError(f"LVC: mode {j} couples states ({a}, {b}) outside [0, {self.nel})")
        self.omegas = [mode.omega for mode in self.modes]
        self.H = None
        self._extra = np.zeros((self.nel, self.nel), dtype=complex)   # add_coupling terms
        self._x = None

    # nvib-sized identities only when asked for
    @property
    def idm_vib(self):
        from scipy.sparse import identity
        return identity(self.nvib)

    @property
    def idm_el(self):
        from scipy.sparse import identity
        return identity(self.nstates)

    def Hel(self):
        """diag(E) plus every add_coupling term, [nel, nel] complex."""
        return np.diag(np.asarray(self.e_fc, dtype=complex)) + self._extra

    def Wmats(self):
        """W [M, nel, nel]: mode j couples to x_j through sum_c strength_c jump(a_c, b_c)."""
        W = np.zeros((self.nmodes, self.nel, self.nel), dtype=complex)
        for j, mode in enumerate(self.modes):
            for c in mode.couplings:
                a, b = c[0]
                W[j] += c[1] * _jump(a, b, self.nel)
        return W

    def _mode_op(self, j, op):
        from scipy.sparse import identity, kron
        out = identity(1, format="csr")
        for k, N in enumerate(self.fock_dims):
            out = kron(out, op if k == j else identity(N, format="csr"), format="csr")
        return out

    MAX_HOST_NNZ = 2 ** 28

    def buildH(self):
        """The vibronic Hamiltonian as a scipy sparse matrix on the host (mol.py:1003-1058), every mode at its own
        truncation.  Not needed for a run."""
        from scipy.sparse import csr_matrix, diags, identity, kron
        if self.dim * (self.nel + 2 * self.nmodes * self.nel) > self.MAX_HOST_NNZ:
            raise ValueError(f"LVC.buildH: D = {self.dim} is too large to assemble H on the host; "
                             "wavepacket_dynamics() runs without it")
        xs = [self._mode_op(j, _x_sparse(N)) for j, N in enumerate(self.fock_dims)]
        hv = csr_matrix((self.nvib, self.nvib))
        for j, N in enumerate(self.fock_dims):
            hv = hv + self._mode_op(j, diags(np.arange(N) * self.omegas[j], format="csr"))
        Hel, W = self.Hel(), self.Wmats()
        real = not (np.iscomplexobj(self.e_fc) or np.any(Hel.imag) or np.any(W.imag))
        cast = (lambda a: a.real) if real else (lambda a: a)
        H = kron(csr_matrix(cast(Hel)), identity(self.nvib), format="csr") + \
            kron(identity(self.nel), hv, format="csr")
        for j in range(self.nmodes):
            H = H + kron(csr_matrix(cast(W[j])), xs[j], format="csr")
        self.H = H.tocsr()
        self._x = xs
        return self.H

    def APES(self, x):
        """Adiabatic surfaces at the point x [M]: the sorted eigenvalues of diag(E) + 1/2 sum_j omega_j x_j^2
        + sum_j W[j] x_j (mol.py:1060-1076; the omega-linear prefactor is the reference's)."""
        x = np.asarray(x, dtype=float).reshape(-1)
        if x.size != self.nmodes:
            raise ValueError(f"LVC.APES: x has {x.size} coordinates for {self.nmodes} modes")
        V = np.diag(np.asarray(self.e_fc, dtype=complex))
        V = V + 0.5 * np.sum(np.asarray(self.omegas) * x ** 2) * np.eye(self.nel)
        W = self.Wmats()
        for j in range(self.nmodes):
            V = V + W[j] * x[j]
        E = np.linalg.eigvals(V.real if not np.any(V.imag) else V)
        return np.sort(E)

    def calc_edip(self):
        pass

    def promote(self, A, which='el'):
        """mol.py:1081-1088: A (x) 1_vib as an LVCOp, or 1_el (x) A as a scipy sparse matrix."""
        from scipy.sparse import identity, kron
        if which in ['el', 'e', 'electronic']:
            return LVCOp(A, self.fock_dims)
        elif which in ['v', 'vib', 'vibrational']:
            return kron(identity(self.nstates), A)
        return A

    def vertical(self, n=1):
        """The state created by vertical excitation to electronic state n: |n> (x) |0 .. 0> (mol.py:1090-1116)."""
        if not 0 <= n < self.nel:
            raise ValueError(f"LVC.vertical: state {n} outside [0, {self.nel})")
        psi = np.zeros(self.dim, dtype=complex)
        psi[n * self.nvib] = 1.0
        return psi

    def groundstate(self):
        return self.vertical(n=0)

    def buildop(self, i, f=None, isherm=True):
        """|f><i| (+ |i><f| when isherm) (x) 1_vib as an LVCOp (mol.py:1130-1161)."""
        if f is None:
            f = i
        return LVCOp(_jump(f, i, self.nstates, isherm), self.fock_dims)

    def coordinate(self, n):
        """1_el (x) x_n as an LVCOp (mol.py:1163-1178); needs no buildH."""
        return LVCOp(np.eye(self.nel), self.fock_dims, mode=n)

    def dpes(self, q):
        pass

    def wavepacket_dynamics(self, method='RK4'):
        if method == 'RK4':
            sol = LVCSolver(self)
            sol.groundstate = self.groundstate()
            return sol
        else:
            raise ValueError('The number of modes {} is not \
                             supported.'.format(self.nmodes))

    def rdm_el(self, psi):
        """rho_ab = sum_n psi[a, n] conj(psi[b, n]) (mol.py:1222-1239)."""
        p = np.reshape(np.asarray(psi), (self.nel, self.nvib))
        return p.dot(p.conj().T)

    def add_coupling(self, coupling):
        """[[a, b], strength]: strength * jump(a, b) (x) 1_vib is added to the Hamiltonian (mol.py:1241-1262), built or
        not.  Returns the updated H when buildH() has run, else None."""
        from scipy.sparse import csr_matrix, identity, kron
        a, b = coupling[0]
        if not (0 <= a < self.nel and 0 <= b < self.nel):
            raise ValueError(f"LVC.add_coupling: states ({a}, {b}) outside [0, {self.nel})")
        term = coupling[1] * _jump(a, b, self.nel)
        self._extra = self._extra + term
        if self.H is not None:
            t = term if np.iscomplexobj(coupling[1]) and np.imag(coupling[1]) != 0 else np.real(term)
            self.H = (self.H + kron(csr_matrix(t), identity(self.nvib), format="csr")).tocsr()
        return self.H


class LVCSolver(SESolver):
    """What LVC.wavepacket_dynamics() returns: SESolver whose run() propagates matrix-free on the GPU (qd_lvc_rk4).
    and whose correlation functions stay matrix-free where the operators are held as factors (qd_lvc_pair_rk4).
    self.H is the model's sparse H, built on first access (correlation functions and pulsed runs with D x D operands
    use it, at sizes the dense path can hold)."""

    def __init__(self, model):
        self.model = model
        self._H = None
        self.groundstate = None

    @property
    def H(self):
        if self._H is None:
            self._H = self.model.H if self.model.H is not None else self.model.buildH()
        return self._H

    @H.setter
    def H(self, value):
        self._H = value

    def _drives(self, edip, pulse):
        """The drives of a matrix-free pulsed run: (A [nd, nel, nel], modes [nd], field) with field(t) the nd values
        f_d(t), or None where edip is a D x D matrix (or [D, D, nc]), which SESolver.run takes on the sparse H."""
        from ._util import issparse, to_numpy
        m = self.model
        if edip is None:
            raise ValueError('Electric dipole must be provided for laser-driven dynamics.')

        def factor(mu, what):
            """(A [nel, nel], mode) of one dipole, None for a D x D matrix"""
            if isinstance(mu, LVCOp):
                if mu.dims != tuple(m.fock_dims) or mu.nel != m.nel:
                    raise ValueError(f"{what} is an LVCOp of another space than the model's")
                return mu.A, -1 if mu.mode is None else int(mu.mode)
            shape = tuple(mu.shape) if hasattr(mu, "shape") else np.shape(mu)
            if shape[:2] == (m.dim, m.dim) or issparse(mu):
                return None
            if shape != (m.nel, m.nel):
                raise ValueError(f"{what} has shape {shape}: expected an LVCOp, [{m.nel}, {m.nel}] or "
                                 f"[{m.dim}, {m.dim}]")
            return to_numpy(mu, np.complex128), -1

        if isinstance(pulse, (list, tuple)):
            if not isinstance(edip, (list, tuple)) or len(edip) != len(pulse):
                raise ValueError("a list of pulses needs a list of as many dipoles")
            fac = [factor(mu, f"edip[{i}]") for i, mu in enumerate(edip)]
            if any(f is None for f in fac):
                return None
            fields = [p.efield for p in pulse]
            return (np.array([f[0] for f in fac], dtype=complex).reshape(-1, m.nel, m.nel), [f[1] for f in fac],
                    lambda t: [complex(f(t)) for f in fields])
        if not isinstance(edip, LVCOp) and not issparse(edip) and np.ndim(edip) == 3:
            shape = np.shape(edip)
            if shape[:2] == (m.dim, m.dim):
                return None
            if shape[:2] != (m.nel, m.nel):
                raise ValueError(f"edip has shape {shape}: expected [{m.nel}, {m.nel}, nc] or [{m.dim}, {m.dim}, nc]")
            nc = shape[2]
            A = np.ascontiguousarray(np.moveaxis(to_numpy(edip, np.complex128), 2, 0))
            return A, [-1] * nc, lambda t: np.asarray(pulse.E(t), dtype=complex).reshape(nc)
        fac = factor(edip, "edip")
        if fac is None:
            return None
        return fac[0].reshape(1, m.nel, m.nel), [fac[1]], lambda t: [complex(pulse.efield(t))]

    # ------------------------------------------------------------ correlation functions, matrix-free
    def _corr_factors(self, name, oplist):
        """[(A [nel, nel], block)] of the operands where every one is held as factors: an LVCOp of the model's space
        (block 0 for A (x) 1, j + 1 for A (x) x_j) or an [nel, nel] array meaning A (x) 1.  None where any operand is a
        D x D matrix, dense or sparse: the call then goes to SESolver's method on self.H."""
        from ._util import issparse, to_numpy
        m = self.model
        fac, dense = [], False
        for i, op in enumerate(oplist):
            if isinstance(op, LVCOp):
                if op.dims != tuple(m.fock_dims) or op.nel != m.nel:
                    raise ValueError(f"{name}: operator {i} is an LVCOp of another space than the model's")
                fac.append((op.A, 0 if op.mode is None else int(op.mode) + 1))
                continue
            shape = tuple(op.shape) if hasattr(op, "shape") else np.shape(op)
            if not issparse(op) and shape == (m.nel, m.nel):
                fac.append((to_numpy(op, np.complex128), 0))
            else:
                dense = True   # SESolver checks its shape
        return None if dense else fac

    @staticmethod
    def _corr_host_ops(oplist):
        return [op.tocsr() if isinstance(op, LVCOp) else op for op in oplist]

    @staticmethod
    def _corr_product(name, b, c):
        """The factors of b c for b, c held as factors; two coordinate factors have no single-block form."""
        if b[1] and c[1]:
            raise NotImplementedError(f"{name}: the product of two coordinate factors (A (x) x_j)(B (x) x_k) is no "
                                      "single block of the pair record; pass D x D operators for the dense path")
        return b[0] @ c[0], b[1] or c[1]

    def _corr_psi0(self, name, psi0):
        from ._util import to_numpy
        p0 = to_numpy(psi0, np.complex128).reshape(-1)
        if p0.size != self.model.dim:
            raise ValueError(f"{name}: psi0 has {p0.size} elements, expected {self.model.dim}")
        return p0

    def _factor_tables(self, fac, dev):
        """(omega, Hel, W) with which lvc_apply applies the factor alone: Hel = A for A (x) 1, W[j] = A for A (x) x_j."""
        import torch
        m = self.model
        A, blk = fac
        Hel = np.zeros((m.nel, m.nel), dtype=complex)
        W = np.zeros((m.nmodes, m.nel, m.nel), dtype=complex)
        if blk == 0:
            Hel[:] = A
        else:
            W[blk - 1] = A
        return np.zeros(m.nmodes), torch.from_numpy(Hel).to(dev), torch.from_numpy(W).to(dev)

    def _pair_bytes(self):
        """Device bytes one pair takes in a pair run: the pair, its copy while it is assembled, the two stage vectors of
        both states, and the partial rows of one block."""
        m = self.model
        tiles = -(-m.nvib // 256)
        return 8 * 16 * m.dim + min(tiles, 1024) * 2 * m.nel * m.nel * 8

    def _pair_corr(self, name, fac, psi_t, dt, ntau, path, chunk=None):
        """corr [B, ntau] of the states psi_t [B, D] (device) for the factors [a, b, c]: ket = c psi and bra = a^+ psi by
        lvc_apply, one lvc_pair_rk4 per chunk of pairs with the single block of b, the contraction on the host."""
        import torch
        m = self.model
        dev = psi_t.device
        B = psi_t.shape[0]
        if chunk is None:
            free = torch.cuda.mem_get_info(dev)[0]
            per = self._pair_bytes()
            chunk = min(B, 32767, (free // 4) // per)
            if chunk < 1:
                raise MemoryError(f"{name}: one pair of D = {m.dim} needs {per} bytes of states and scratch, a quarter "
                                  f"of the free device memory is {free // 4} bytes")
        chunk = max(1, min(int(chunk), 32767))
        (a, a_blk), (b, b_blk), c = fac
        t_ket = self._factor_tables(c, dev)
        t_bra = self._factor_tables((a.conj().T, a_blk), dev)   # x_j is Hermitian
        Hel = torch.from_numpy(np.ascontiguousarray(m.Hel())).to(dev)
        W = torch.from_numpy(np.ascontiguousarray(m.Wmats())).to(dev)
        corr = np.zeros((B, ntau), dtype=complex)
        for i0 in range(0, B, chunk):
            src = psi_t[i0:i0 + chunk].contiguous()
            pairs = torch.empty((src.shape[0], 2, m.dim), dtype=torch.complex128, device=dev)
            pairs[:, 0] = lvc_apply(src, m.nel, m.fock_dims, *t_ket)
            pairs[:, 1] = lvc_apply(src, m.nel, m.fock_dims, *t_bra)
            rec = lvc_pair_rk4(pairs, m.nel, m.fock_dims, m.omegas, Hel, W, dt, ntau - 1, save_every=1,
                               blocks=(b_blk,), path=path)
            corr[i0:i0 + chunk] = np.einsum("ab,...ba->...", b, rec[:, :, 0].cpu().numpy())
            del pairs, rec
        return corr

    def correlation_3op_1t(self, psi0, oplist, dt, Nt, device=None, path="auto"):
        """<A B(t) C> at t = 0 .. (Nt-1) dt (mol.py:1475-1501): complex ndarray (Nt,), corr[j] = <bra(j)| b |ket(j)>
        with ket = c psi0 and bra = a^+ psi0 after j steps.  Where every operator is held as factors (an LVCOp of the
        model's space, or an [nel, nel] array meaning A (x) 1) the call is matrix-free: c and a^+ by lvc_apply, one
        lvc_pair_rk4 with the block of b.  Any D x D operand (dense or sparse) takes SESolver's method on self.H, an
        LVCOp beside it converted with tocsr()."""
        _check_corr_args("correlation_3op_1t", oplist, 3, Nt=Nt)
        fac = self._corr_factors("correlation_3op_1t", oplist)
        if fac is None:
            return SESolver.correlation_3op_1t(self, psi0, self._corr_host_ops(oplist), dt, Nt)
        return self._corr_1t("correlation_3op_1t", psi0, fac, dt, Nt, device, path)

    def _corr_1t(self, name, psi0, fac, dt, Nt, device, path):
        import torch
        from ._util import default_device
        if path not in LVC_PATHS:
            raise ValueError(f"{name}: path={path!r}, expected 'auto', 'staged' or 'resident'")
        p0 = self._corr_psi0(name, psi0)
        dev = torch.device(device) if device is not None else default_device()
        psi = torch.from_numpy(p0.reshape(1, -1).copy()).to(dev)
        return self._pair_corr(name, fac, psi, dt, int(Nt), path)[0]

    def correlation_3op_2t(self, psi0, oplist, dt, Nt, Ntau, device=None, path="auto", _chunk=None):
        """<A(t) B(t+tau) C(t)> (mol.py:1503-1536): complex ndarray (Nt, Ntau).  With operators held as factors the
        states psi(t_i) are the snapshots of one lvc_rk4 run and stay on the device; their Nt pairs go through the pair
        run in chunks whose states and scratch stay under a quarter of the free device memory (MemoryError where one
        pair does not fit).  D x D operands as in correlation_3op_1t."""
        _check_corr_args("correlation_3op_2t", oplist, 3, Nt=Nt, Ntau=Ntau)
        fac = self._corr_factors("correlation_3op_2t", oplist)
        if fac is None:
            return SESolver.correlation_3op_2t(self, psi0, self._corr_host_ops(oplist), dt, Nt, Ntau)
        return self._corr_2t("correlation_3op_2t", psi0, fac, dt, Nt, Ntau, device, path, _chunk)

    def _corr_2t(self, name, psi0, fac, dt, Nt, Ntau, device, path, chunk):
        import torch
        from ._util import default_device
        if path not in LVC_PATHS:
            raise ValueError(f"{name}: path={path!r}, expected 'auto', 'staged' or 'resident'")
        m = self.model
        p0 = self._corr_psi0(name, psi0)
        dev = torch.device(device) if device is not None else default_device()
        psi = torch.from_numpy(p0.reshape(1, -1).copy()).to(dev)
        psi_t = psi.clone()
        if Nt > 1:
            Hel = torch.from_numpy(np.ascontiguousarray(m.Hel())).to(dev)
            W = torch.from_numpy(np.ascontiguousarray(m.Wmats())).to(dev)
            snap, _ = lvc_rk4(psi, m.nel, m.fock_dims, m.omegas, Hel, W, dt, int(Nt) - 1, save_every=1, observe=False)
            psi_t = torch.cat([psi_t, snap[0]], dim=0)
        return self._pair_corr(name, fac, psi_t, dt, int(Ntau), path, chunk)

    def correlation_4op_1t(self, psi0, oplist, dt=0.005, Nt=1, device=None, path="auto"):
        """<A B(t) C(t) D> (mol.py:1538-1554): the 3-operator form with [a, b c, d].  Matrix-free where all four are
        held as factors and b c is one: the product of two coordinate factors raises NotImplementedError."""
        _check_corr_args("correlation_4op_1t", oplist, 4, Nt=Nt)
        fac = self._corr_factors("correlation_4op_1t", oplist)
        if fac is None:
            return SESolver.correlation_4op_1t(self, psi0, self._corr_host_ops(oplist), dt, Nt)
        fac = [fac[0], self._corr_product("correlation_4op_1t", fac[1], fac[2]), fac[3]]
        return self._corr_1t("correlation_4op_1t", psi0, fac, dt, Nt, device, path)

    def correlation_4op_2t(self, psi0, oplist, dt=0.005, Nt=1, Ntau=1, device=None, path="auto", _chunk=None):
        """<A(t) B(t+tau) C(t+tau) D(t)> (mol.py:1556-1566): the 3-operator form with [a, b c, d], as
        correlation_4op_1t."""
        _check_corr_args("correlation_4op_2t", oplist, 4, Nt=Nt, Ntau=Ntau)
        fac = self._corr_factors("correlation_4op_2t", oplist)
        if fac is None:
            return SESolver.correlation_4op_2t(self, psi0, self._corr_host_ops(oplist), dt, Nt, Ntau)
        fac = [fac[0], self._corr_product("correlation_4op_2t", fac[1], fac[2]), fac[3]]
        return self._corr_2t("correlation_4op_2t", psi0, fac, dt, Nt, Ntau, device, path, _chunk)

    def run_batch(self, psi0s, dt=0.01, Nt=1, e_ops=None, nout=1, t0=0.0, store_states=True, device=None,
                  path="auto", edip=None, pulse=None, sample="hold"):
        """run() for the rows of psi0s [B, D] in one call: a list of B results.  With a pulse every member sees the
        same field (edip as in run(): an LVCOp, [nel, nel], a list of those with a list of pulses, or [nel, nel, nc]
        with a vector pulse; a D x D dipole is not taken here)."""
        import torch
        from ._util import default_device, issparse, to_numpy
        m = self.model
        drives = None
        if pulse is not None:
            if sample not in LVC_SAMPLES:
                raise ValueError(f"sample={sample!r}, expected 'hold' or 'stage'")
            drives = self._drives(edip, pulse)
            if drives is None:
                raise ValueError("run_batch: a D x D dipole has no matrix-free form; pass an LVCOp or [nel, nel] factors")
        e_ops = [] if e_ops is None else list(e_ops)
        for i, op in enumerate(e_ops):
            if isinstance(op, LVCOp):
                if op.shape[0] != m.dim or op.nel != m.nel:
                    raise ValueError(f"e_ops[{i}] acts on another space than the model's")
            elif not store_states:
                raise TypeError(f"e_ops[{i}] is no LVCOp: with store_states=False only LVCOp observables, read from "
                                "the on-device record, can be evaluated")
            elif tuple(op.shape) != (m.dim, m.dim):
                raise ValueError(f"e_ops[{i}] has shape {tuple(op.shape)}, expected {(m.dim, m.dim)}")
        p0 = to_numpy(psi0s, np.complex128)
        if p0.ndim != 2 or p0.shape[1] != m.dim:
            raise ValueError(f"psi0s must be [B, {m.dim}], got {p0.shape}")
        B = p0.shape[0]
        dev = torch.device(device) if device is not None else default_device()
        nblk = Nt // nout
        nsteps = max(nblk - 1, 0) * nout
        psi = torch.from_numpy(np.ascontiguousarray(p0).copy()).to(dev)
        Hel = torch.from_numpy(np.ascontiguousarray(m.Hel())).to(dev)
        W = torch.from_numpy(np.ascontiguousarray(m.Wmats())).to(dev)
        if drives is None:
            snap, obs = lvc_rk4(psi, m.nel, m.fock_dims, m.omegas, Hel, W, dt, nsteps, save_every=nout,
                                store=store_states, path=path)
        else:
            # driven_dynamics' rule: block k of nout steps holds f(t0 + k nout dt); stage mode samples the half-step grid
            A, modes, field = drives
            ts = t0 + 0.5 * dt * np.arange(2 * nsteps + 1) if sample == "stage" else \
                t0 + nout * dt * np.arange(max(nblk - 1, 0))
            fv = np.array([field(t) for t in ts], dtype=np.complex128).reshape(len(ts), len(modes))
            snap, obs = lvc_driven_rk4(psi, m.nel, m.fock_dims, m.omegas, Hel, W,
                                       torch.from_numpy(np.ascontiguousarray(A)).to(dev), modes,
                                       torch.from_numpy(fv).to(dev), dt, nsteps, hold=nout, sample=sample,
                                       save_every=nout, store=store_states, path=path)
        rec = obs.cpu().numpy()[:, :nblk]
        nn, M = m.nel * m.nel, m.nmodes
        rho = rec[..., :nn].reshape(B, -1, m.nel, m.nel)
        X = rec[..., nn:nn * (1 + M)].reshape(B, -1, M, m.nel, m.nel)
        nbar = rec[..., nn * (1 + M):].real
        states = snap.cpu().numpy() if snap is not None else None
        final = psi.cpu().numpy()
        results = []
        for b in range(B):
            result = Result(dt=dt, Nt=Nt, psi0=p0[b].copy(), t0=t0, nout=nout)
            observables = np.zeros((nblk, len(e_ops)), dtype=complex)
            if store_states:
                result.psilist = [p0[b].copy()] + ([states[b, k] for k in range(states.shape[1])]
                                                   if states is not None else [])
            for i, op in enumerate(e_ops):
                if isinstance(op, LVCOp):
                    observables[:, i] = op.from_record(rho[b], X[b])
                else:
                    A = op if issparse(op) else np.asarray(op)
                    observables[:, i] = [np.vdot(s, A @ s) for s in result.psilist[:nblk]]
            result.observables = observables
            result.psi = final[b]
            result.rdm_el = rho[b]
            result.x = np.einsum("kjaa->kj", X[b])
            result.nbar = nbar[b]
            results.append(result)
        return results

    def run(self, psi0=None, dt=0.01, Nt=1, e_ops=None, nout=1, t0=0.0, store_states=True, device=None, edip=None,
            pulse=None, use_sparse=True, path="auto", sample="hold"):
        """mol.py:1392-1459 with _quantum_dynamics's counts: (Nt//nout - 1) * nout steps, psilist = [psi0] + the state
        after every nout steps, observables (Nt//nout, n_e).  LVCOp e_ops come from the on-device record, any other
        matrix is applied on the host to the stored states.  result.rdm_el [Nt//nout, nel, nel], result.x and
        result.nbar [Nt//nout, M] come with every run.  store_states=False keeps and copies no state.

        With a pulse the run stays matrix-free (qd_lvc_driven_rk4) where edip is held as factors: an LVCOp of the
        model's space (A (x) 1 or A (x) x_j), an [nel, nel] array (A (x) 1), a list of those with a list of pulses, or
        an [nel, nel, nc] array with one pulse whose E(t) returns nc components.  Steps and times are driven_dynamics':
        sample="hold" holds f(t0 + k nout dt) over block k of nout steps; sample="stage" is classical RK4 with the field
        at the stage times.  The result has the form above (dense psilist, psi the final state).  A D x D edip falls
        through to SESolver.run on self.H."""
        if psi0 is None:
            psi0 = self.groundstate
        if pulse is not None:
            if sample not in LVC_SAMPLES:
                raise ValueError(f"sample={sample!r}, expected 'hold' or 'stage'")
            if self._drives(edip, pulse) is None:
                if sample != "hold":
                    raise ValueError(f"sample={sample!r} needs the dipole as factors (an LVCOp or [nel, nel]): a D x D "
                                     "edip runs on SESolver.run, which holds the field per block")
                e_host = None if e_ops is None else [op.tocsr() if isinstance(op, LVCOp) else op for op in e_ops]
                return SESolver.run(self, psi0=psi0, dt=dt, Nt=Nt, e_ops=e_host, nout=nout, t0=t0, edip=edip,
                                    pulse=pulse, use_sparse=use_sparse)
        p0 = np.asarray(psi0.toarray() if hasattr(psi0, "toarray") else psi0, dtype=complex).reshape(1, -1)
        result = self.run_batch(p0, dt=dt, Nt=Nt, e_ops=e_ops, nout=nout, t0=t0, store_states=store_states,
                                device=device, path=path, edip=edip, pulse=pulse, sample=sample)[0]
        result.psi0 = psi0
        return result
