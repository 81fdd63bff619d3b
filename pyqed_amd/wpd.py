"""Split-operator wavepacket dynamics on MI355X (drop-in for pyqed/wpd.py SPO, SPO2).

Setup: grids and exp_K on the host like the reference's build (wpd.py:217-223, 496-625);
the per-point propagators exp(-i V dt), exp(-i V dt/2) on the device (qd_spo_expv: closed form for
ns <= 2, a matrix exponential up to ns = 256).
Every propagation step runs in libqdyn (qd_spo1d_run / qd_spo2_run_ex / qd_spo3_run).
Populations, mean positions and the electronic reduced density matrix are reduced on the device
(qd_spo_observe), after the run from states or inside it (run(..., observe=...), qd_spo*_run_observed).
Curvilinear coordinates (wpd.py:1783-1940: adiabatic_2d, KEO, PEO, hpsi) apply the G-matrix kinetic operator and run
its RK4 steps in libqdyn (qd_wp2_gmat_apply / qd_wp2_gmat_rk4); on coupled surfaces (a potential [nx, ny, ns, ns];
SPO2(coords='curvilinear', G=G)) qd_wp2_gmat_ms_apply / qd_wp2_gmat_ms_rk4; in three coordinates (KEO3, hpsi3,
curvilinear_run3, SPO3(coords='curvilinear', G=G) with G [nx, ny, nz, 3, 3]) the qd_wp3_gmat_* calls.  One front
serves all of them: _gmat_check, _gmat_dev, _gmat_apply and _gmat_run take the k vectors or axes as a list, and the
number of coordinates and of states names the entry point (_gmat_call).
"""
from __future__ import annotations

import numpy as np
import torch
from scipy.fftpack import fftfreq

from . import _lib
from ._util import default_device
from .mol import Result

DEVICE_EXPM_MAX_NS = 1024   # qd_spo_expv / qd_spo_expm: work matrices in LDS to ns = 50, in device scratch above

pi = np.pi



def _check_finite(v):
    """The reference builds the point propagators with eigh / eig (wpd.py:585-623, 960-985), which raise LinAlgError on
    inf / NaN potentials; the device exponential would only produce NaN, so the same error is raised up front."""
    if not np.all(np.isfinite(v)):
        raise np.linalg.LinAlgError("Array must not contain infs or NaNs")

def interval(x):
    return x[1] - x[0]


def meshgrid(*args):
    return np.meshgrid(*args, indexing="ij")


class ResultSPO2(Result):
    """wpd.py:57-178 (result container with grid and population helpers)."""

    def __init__(self, **args):
        super().__init__(**args)
        self.x = None
        self.y = None
        self.population = None
        self.xAve = None
        self.rdm = None
        self._recorded = None   # run(observe=...): (population, xAve, yAve) reduced on the device during the run
        self.nstates = self.psi0.shape[-1]

    def _recorded_only(self):
        """The observables a run(observe=...) recorded, when the run kept no states to recompute them from."""
        rec = getattr(self, "_recorded", None)
        return rec if rec is not None and len(self.psilist) <= 1 else None

    def get_population(self, fname=None, plot=False):
        """wpd.py:104-127.  After run(observe=..., return_states=False) psilist holds only psi0 and the populations
        recorded during the run are returned instead (extension)."""
        rec = self._recorded_only()
        if rec is not None:
            p = self.population = rec[0]
            if fname is not None:
                np.savez(fname, p)
            return p
        dx = interval(self.x)
        dy = interval(self.y)
        p = np.zeros((len(self.psilist), self.nstates))
        for n in range(self.nstates):
            p[:, n] = [np.vdot(psi[:, :, n], psi[:, :, n]).real * dx * dy for psi in self.psilist]
        self.population = p
        if fname is not None:
            np.savez(fname, p)
        return p

    def position(self, plot=False, fname=None):
        """wpd.py:138-159.  After run(observe=..., return_states=False) the recorded mean positions are returned
        (extension); xAve.npz is written either way."""
        rec = self._recorded_only()
        if rec is not None:
            xAve, yAve = rec[1], rec[2]
            self.xAve = [xAve, yAve]
            np.savez('xAve', xAve, yAve)
            return xAve, yAve
        x, y = self.x, self.y
        dx, dy = interval(x), interval(y)
        xAve = [np.einsum('ijn, i, ijn', psi.conj(), x, psi) * dx * dy for psi in self.psilist]
        yAve = [np.einsum('ijn, j, ijn', psi.conj(), y, psi) * dx * dy for psi in self.psilist]
        xAve = np.real_if_close(xAve)  # wpd.py:150-151
        yAve = np.real_if_close(yAve)
        self.xAve = [xAve, yAve]
        np.savez('xAve', xAve, yAve)  # wpd.py:159 writes xAve.npz in the CWD
        return xAve, yAve


def _dev_c128(a, dev):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=complex))).to(dev)


def _dev_f64(a, dev):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=float))).to(dev)


def _volume(axes):
    return float(np.prod([interval(np.asarray(a)) for a in axes]))


def observe_states(psi, axes, basis=None, weight=None, moments=True):
    """Electronic reduced density matrix and first moments of split-operator states, reduced on the device
    (qd_spo_observe; extension).

    psi: [n0(, n1(, n2)), ns] or a batch [B, n0, ..., ns], a device tensor (used in place, not copied, when it is
    contiguous complex128) or anything numpy reads; axes: the ndim = 1..3 coordinate arrays; basis: None or
    M [n0, ..., ns, ns], applied as chi_a = sum_b M[p][a][b] psi_b; weight: the volume element (default: the product of
    the axes' spacings).  Returns device tensors (rdm [(B,) ns, ns] complex, mom [(B,) ndim, ns] float or None):
        rdm[a][b] = weight sum_p conj(chi_a) chi_b,    mom[d][a] = weight sum_p x_d(p) |chi_a|^2.
    """
    ndim = len(axes)
    if isinstance(psi, torch.Tensor):
        dev = psi.device
        t = psi.to(dtype=torch.complex128).contiguous()
    else:
        dev = default_device()
        t = _dev_c128(psi, dev)
    _lib.ensure_device(dev)
    if t.dim() not in (ndim + 1, ndim + 2):
        raise ValueError(f"psi must be [{'n, ' * ndim}ns] or a batch of those; got {tuple(t.shape)}")
    batched = t.dim() == ndim + 2
    dims = tuple(t.shape[-1 - ndim:-1])
    ns = int(t.shape[-1])
    if dims != tuple(len(a) for a in axes):
        raise ValueError(f"grid {dims} does not match the axes {tuple(len(a) for a in axes)}")
    B = int(t.shape[0]) if batched else 1
    if basis is not None:
        basis = basis.to(device=dev, dtype=torch.complex128).contiguous() if isinstance(basis, torch.Tensor) \
            else _dev_c128(basis, dev)
        if tuple(basis.shape) != dims + (ns, ns):
            raise ValueError(f"basis must be {dims + (ns, ns)}; got {tuple(basis.shape)}")
    if weight is None:
        weight = _volume(axes)
    ax = [_dev_f64(a, dev) for a in axes] if moments else []
    rdm = torch.empty((B, ns, ns), dtype=torch.complex128, device=dev)
    mom = torch.empty((B, ndim, ns), dtype=torch.float64, device=dev) if moments else None
    cdims = (_lib.c_int * ndim)(*dims)
    with torch.cuda.device(dev):
        rc = _lib.load().qd_spo_observe(t.data_ptr(), B, cdims, ndim, ns, _lib.ptr(basis),
                                        *(ax[d].data_ptr() if moments and d < ndim else None for d in range(3)),
                                        float(weight), rdm.data_ptr(), _lib.ptr(mom), _lib.stream_ptr(dev))
    _lib.check(rc, "qd_spo_observe")
    if not batched:
        return rdm[0], (mom[0] if moments else None)
    return rdm, mom


def _check_representation(representation):
    if representation not in ('diabatic', 'adiabatic'):
        raise ValueError('Representation = {}, which can only be diabatic or adiabatic'.format(representation))


class SPO:
    """Drop-in for pyqed.wpd.SPO (wpd.py:191-322): 1D, single surface."""

    def __init__(self, x, mass=1, nstates=1):
        self.x = x
        self.dx = interval(x)
        self.nx = len(x)
        self.k = 2. * pi * fftfreq(self.nx, self.dx)
        self.nstates = nstates
        self.V = None
        self.mass = mass
        self._exp_K = None
        self._exp_V = None
        self._exp_V_half = None

    def set_grid(self, xmin=-1, xmax=1, npts=32):
        self.x = np.linspace(xmin, xmax, npts)

    def set_potential(self, potential):
        self.V = potential(self.x)
        return

    def build(self, dt):
        """wpd.py:217-223."""
        self._exp_V = np.exp(-1j * self.V * dt)
        self._exp_V_half = np.exp(-1j * self.V * dt / 2.)
        m = self.mass
        k = self.k
        self._exp_K = np.exp(-0.5j / m * (k * k) * dt)

    def run(self, psi0, dt, nt=1, t0=0, nout=1):
        """wpd.py:225-273 step structure; psilist has nt//nout - 1 entries, r.psi the final state.
        psi0 may also be a batch [B, nx] (extension): B wavepackets propagated together."""
        self.build(dt)
        dev = default_device()
        _lib.ensure_device(dev)
        p0 = np.asarray(psi0)
        batched = p0.ndim == 2
        psi = _dev_c128(p0.reshape(-1, self.nx), dev)
        B = psi.shape[0]
        nsnap = max(nt // nout - 1, 0)
        snap = torch.empty((B, nsnap, self.nx), dtype=torch.complex128, device=dev) if nsnap else None
        eV, eVh, eK = (_dev_c128(a, dev) for a in (self._exp_V, self._exp_V_half, self._exp_K))
        with torch.cuda.device(dev):
            rc = _lib.load().qd_spo1d_run(psi.data_ptr(), eV.data_ptr(), eVh.data_ptr(), eK.data_ptr(), self.nx, B,
                                          int(nt), int(nout), _lib.ptr(snap), _lib.stream_ptr(dev))
        _lib.check(rc, "qd_spo1d_run")
        r = Result(psi0=psi0, dt=dt, Nt=nt, t0=t0, nout=nout)
        snaps = snap.cpu().numpy() if snap is not None else np.zeros((B, 0, self.nx), complex)
        out = psi.cpu().numpy()
        if batched:
            r.psilist = [snaps[:, k] for k in range(nsnap)]
            r.psi = out
        else:
            r.psilist = [snaps[0, k] for k in range(nsnap)]
            r.psi = out[0]
        return r


class _PointPropagators:
    """exp_V / exp_V_half of a Hermitian diabatic potential, built on the device.

    The reference's build (wpd.py:585-623, SPO3 :1290-1330) loops over grid points calling eigh and
    forming U e^{-i w tau} U^+.  qd_spo_expv evaluates the same point propagators on the GPU (LAPACK
    conventions: lower triangle, real diagonal): in closed form for ns <= 2, as a scaling-and-squaring
    matrix exponential for 2 < ns <= 1024; they stay on the device for the run and are copied to the
    host only when exp_V / exp_V_half are read.  The eigen data (d2a = U, apes = w) are host eigh
    results computed on first access.  ns > 1024 builds on the host with a vectorised eigh.
    """
    _eV_dev = _eVh_dev = None
    _exp_V_host = _exp_V_half_host = None
    _d2a = _apes = None
    _d2a_dev = None   # d2a on the device for observe='adiabatic' / population(..., 'adiabatic'): uploaded once per build
    _eig_pending = False

    @property
    def exp_V(self):
        if self._exp_V_host is None and self._eV_dev is not None:
            self._exp_V_host = self._eV_dev.cpu().numpy()
        return self._exp_V_host

    @exp_V.setter
    def exp_V(self, a):
        self._exp_V_host, self._eV_dev = a, None

    @property
    def exp_V_half(self):
        if self._exp_V_half_host is None and self._eVh_dev is not None:
            self._exp_V_half_host = self._eVh_dev.cpu().numpy()
        return self._exp_V_half_host

    @exp_V_half.setter
    def exp_V_half(self, a):
        self._exp_V_half_host, self._eVh_dev = a, None

    def _host_eig(self):
        v = self._pot()
        w, u = np.linalg.eigh(v)          # ascending eigenvalues per point (phys.sort order)
        self._d2a, self._d2a_dev = u, None
        self._apes = None if np.iscomplexobj(v) else w
        self._eig_pending = False
        return w, u

    @property
    def d2a(self):
        if self._eig_pending:
            self._host_eig()
        return self._d2a

    @d2a.setter
    def d2a(self, u):
        self._d2a, self._d2a_dev = u, None

    @property
    def apes(self):
        if self._eig_pending:
            self._host_eig()
        return self._apes

    @apes.setter
    def apes(self, w):
        self._apes = w

    def _build_point_ops(self, dt):
        v = self._pot()
        ns = v.shape[-1]
        _check_finite(v)
        if ns > DEVICE_EXPM_MAX_NS:   # beyond the device exponential's cap (qd_spo_expv): host eigh, as the reference
            w, u = self._host_eig()
            ud = np.conj(np.swapaxes(u, -1, -2))
            self.exp_V = (u * np.exp(-1j * w * dt)[..., None, :]) @ ud
            self.exp_V_half = (u * np.exp(-1j * w * dt / 2)[..., None, :]) @ ud
            return
        dev = default_device()
        _lib.ensure_device(dev)
        cplx = np.iscomplexobj(v)
        vd = torch.from_numpy(np.ascontiguousarray(v, dtype=complex if cplx else float)).to(dev)
        eV = torch.empty(v.shape, dtype=torch.complex128, device=dev)
        eVh = torch.empty_like(eV)
        with torch.cuda.device(dev):
            rc = _lib.load().qd_spo_expv(vd.data_ptr(), int(cplx), int(v.size // (ns * ns)), ns, float(dt),
                                         eV.data_ptr(), eVh.data_ptr(), _lib.stream_ptr(dev))
        _lib.check(rc, "qd_spo_expv")
        self.exp_V, self.exp_V_half = None, None
        self._eV_dev, self._eVh_dev = eV, eVh
        self._d2a = self._apes = self._d2a_dev = None
        self._eig_pending = True

    # ---- observables (qd_spo_observe); _axes() and nstates come from the solver class
    def _obs_basis(self, observe, dev):
        """The basis M of observe= / representation=: None ('diabatic'), d2a ('adiabatic') or an explicit
        [..., ns, ns] array, on the device."""
        if isinstance(observe, str):
            _check_representation(observe)
            if observe == 'diabatic':
                return None
            if self._d2a_dev is None or self._d2a_dev.device != dev:
                u = self.d2a
                if u is None:
                    raise ValueError("the adiabatic representation needs d2a (build() first, or set it)")
                self._d2a_dev = _dev_c128(u, dev)
            return self._d2a_dev
        shape = tuple(len(a) for a in self._axes()) + (self.nstates, self.nstates)
        b = observe.to(device=dev, dtype=torch.complex128).contiguous() if isinstance(observe, torch.Tensor) \
            else _dev_c128(observe, dev)
        if tuple(b.shape) != shape:
            raise ValueError(f"observe basis must be {shape}; got {tuple(b.shape)}")
        return b

    def _states_dev(self, psi):
        """(device tensor [B, grid..., ns], kind) of a state, a list of states, a stacked array or a device tensor;
        kind is 'one', 'list' or 'batch'."""
        nd = len(self._axes())
        if isinstance(psi, list):
            return _dev_c128(np.stack([np.asarray(p) for p in psi]) if psi else
                             np.zeros((0,) + tuple(len(a) for a in self._axes()) + (self.nstates,)),
                             default_device()), 'list'
        t = psi if isinstance(psi, torch.Tensor) else _dev_c128(psi, default_device())
        if t.dim() == nd + 1:
            return t[None], 'one'
        if t.dim() == nd + 2:
            return t, 'batch'
        raise ValueError(f"psi must be a state, a list of states or a stacked array; got shape {tuple(t.shape)}")

    def _rdm_of(self, psi, basis_spec):
        t, kind = self._states_dev(psi)
        ns = self.nstates
        if t.shape[0] == 0:
            return np.zeros((0, ns, ns), complex), kind
        basis = self._obs_basis(basis_spec, t.device)
        rdm, _ = observe_states(t, self._axes(), basis=basis, moments=False)
        return rdm.cpu().numpy(), kind

    def _population(self, psi, representation):
        _check_representation(representation)
        rdm, kind = self._rdm_of(psi, representation)
        P = np.ascontiguousarray(np.einsum('kaa->ka', rdm).real)
        return P[0] if kind == 'one' else P

    def rdm_el(self, psi):
        """Reduced electronic density matrix rho[a, b] = sum_p conj(psi_a) psi_b dV (wpd.py:760-794), reduced on the
        device (qd_spo_observe): an ndarray (or device tensor) state gives [ns, ns], a list a list of [ns, ns]; a
        stacked array [B, ..., ns] (extension) gives [B, ns, ns]."""
        rdm, kind = self._rdm_of(psi, 'diabatic')
        if kind == 'one':
            return rdm[0]
        return [rdm[k].copy() for k in range(len(rdm))] if kind == 'list' else rdm

    def _first_row(self, psi0, basis, dev):
        """rdm and mom of psi0: row 0 of a run's recorded observables."""
        rdm, mom = observe_states(_dev_c128(psi0, dev), self._axes(), basis=basis)
        return rdm[None], mom[None]

    def _point_ops_dev(self, dev, need_full=False):
        eVh = self._eVh_dev if self._eVh_dev is not None else _dev_c128(self.exp_V_half, dev)
        eV = None
        if need_full:
            eV = self._eV_dev if self._eV_dev is not None else _dev_c128(self.exp_V, dev)
        return eV, eVh


class SPO2(_PointPropagators):
    """Drop-in for pyqed.wpd.SPO2 (wpd.py:379-887), linear and Jacobi coordinates.

    coords='curvilinear' with a metric G [nx, ny, 2, 2] (extension: the reference's constructor takes both and its
    header says "for curvilinear coordinates, use RK4 method", but its run dies on an unbound KEO): no split operator
    exists for K = 1/2 sum p_r G_rs(x, y) p_s, so run / run_batch take RK4 steps of
    i dpsi_a/dt = K psi_a + sum_b v_ab psi_b (curvilinear_run, qd_wp2_gmat_ms_rk4) with the same results interface."""

    def __init__(self, x, y, mass=None, nstates=2, coords='linear', G=None, abc=False):
        self.x = x
        self.y = y
        self.X, self.Y = meshgrid(x, y)
        self.nx = len(x)
        self.ny = len(y)
        self.dx = interval(x)
        self.dy = interval(y)
        if mass is None:
            mass = [1, 1]
        self.mass = self.masses = mass
        self.kx = None
        self.ky = None
        self.apes = None
        self.dim = 2
        self.exp_V = None
        self.exp_V_half = None
        self.exp_K = None
        self.v = self.V = None
        self.G = G
        self.nstates = self.ns = nstates
        self.coords = coords
        self.abc = abc
        self.d2a = None
        self.a2d = None
        self.psilist = None

    def set_grid(self, x, y):
        self.x = x
        self.y = y

    def set_masses(self, mass):
        self.mass = mass

    def setG(self, G):
        self.G = G

    def set_DPES(self, surfaces, diabatic_couplings, eta=None):
        """wpd.py:436-484 (real potential array, as the reference: complex couplings lose Im)."""
        nx, ny, ns = self.nx, self.ny, self.ns
        v = np.zeros([nx, ny, ns, ns])
        for a in range(self.ns):
            v[:, :, a, a] = surfaces[a]
        for dc in diabatic_couplings:
            a, b = dc[0][:]
            v[:, :, a, b] = np.real(dc[1])
            v[:, :, b, a] = v[:, :, a, b].conj()
        if self.abc:
            v = v.astype(complex)
            for n in range(self.ns):
                v[:, :, n, n] = -1j * eta * (self.X - 9.) ** 2
        self.v = v
        return v

    def set_dpes(self, v):
        self.V = self.v = v
        return self

    def _pot(self):
        return self.v

    def _axes(self):
        return (self.x, self.y)

    def population(self, psi, representation='diabatic', plot=False):
        """Electronic populations (wpd.py:627-689), reduced on the device (qd_spo_observe): a list of states gives
        [N, ns], an ndarray [nx, ny, ns] gives [ns]; a stacked array [B, nx, ny, ns] or a device tensor is also
        accepted (extension; a device tensor is read in place, not copied).  The reference's ndarray branch dies on
        np.close, which does not exist (wpd.py:648, 670); P is returned here.

        representation='adiabatic' applies self.d2a exactly as the reference does, chi_a = sum_b d2a[i, j, a, b] psi_b
        (wpd.py:664, 674): M = d2a, NOT its adjoint, so these are not projections on the eigenvector columns, and the
        numbers depend on the eigenvector gauge: flipping the sign of one eigenvector column changes the result (by
        1.5e-2 on a 32 x 32 two-state model).  For projections pass the adjoint explicitly,
        run(..., observe=d2a.conj().swapaxes(-1, -2)).  Any other representation raises the reference's ValueError."""
        return self._population(psi, representation)

    def build(self, dt, inertia=None):
        """wpd.py:496-625: the kinetic propagator (linear: exp_K on the 'ij' k-grid; jacobi:
        exp_Kx and exp_Ky[i, ky] = exp(-i ky^2 / (2 I(x_i)) dt) with I = masses[1]) and the per-point
        U e^{-i w tau} U^+ (device build, _PointPropagators)."""
        nx, ny = self.nx, self.ny
        self.kx = 2. * np.pi * fftfreq(nx, interval(self.x))
        self.ky = 2. * np.pi * fftfreq(ny, interval(self.y))
        if self.coords == 'curvilinear':   # RK4 on the G-matrix operator: no exp_K, no exp_V
            _gmat_check_G(self.G, (nx, ny), f"the grid {(nx, ny)}")
            self._d2a = self._apes = self._d2a_dev = None
            self._eig_pending = self.v is not None   # d2a for observe='adiabatic': host eigh on first access
            return
        self._build_keo(dt)
        if self.v is None:
            raise ValueError('The diabatic PES is not specified.')
        self._build_point_ops(dt)

    def _build_keo(self, dt):
        if self.coords == 'linear':
            mx, my = self.masses
            Kx, Ky = meshgrid(self.kx, self.ky)
            self.exp_K = np.exp(-1j * (Kx ** 2 / 2. / mx + Ky ** 2 / 2. / my) * dt)
        elif self.coords == 'jacobi':
            mx = self.masses[0]
            self.exp_Kx = np.exp(-1j * self.kx ** 2 / 2. / mx * dt)
            Iinv = 1. / self.masses[1](self.x)  # y is the angle
            self.exp_Ky = np.exp(-1j * np.outer(Iinv, self.ky ** 2 / 2.) * dt)
        else:
            raise ValueError(f"unknown coordinates {self.coords!r}")

    def _propagate(self, psi0, dt, nt, nout, merged):
        """GPU run (qd_spo2_run_ex): Strang steps V/2 K V/2 with a snapshot after every nout
        steps (merged=False), or the merged V/2, [K V]..., K, V/2 structure (merged=True).
        Returns (final psi, list of snapshots)."""
        dev = default_device()
        _lib.ensure_device(dev)
        nsteps = (nt // nout) * nout
        psi = _dev_c128(psi0, dev)
        nsnap = nt // nout
        snap = torch.empty((nsnap, self.nx, self.ny, self.ns), dtype=torch.complex128, device=dev) if nsnap else None
        eV, eVh = self._point_ops_dev(dev, need_full=merged)
        if self.coords == 'jacobi':
            eK = _dev_c128(np.broadcast_to(self.exp_Kx[:, None], (self.nx, self.ny)), dev)
            eKy = _dev_c128(self.exp_Ky, dev)
        else:
            eK = _dev_c128(self.exp_K, dev)
            eKy = None
        with torch.cuda.device(dev):
            rc = _lib.load().qd_spo2_run_ex(psi.data_ptr(), eVh.data_ptr(), _lib.ptr(eV), eK.data_ptr(), _lib.ptr(eKy),
                                            self.nx, self.ny, self.ns, int(nsteps), int(nout), _lib.ptr(snap),
                                            _lib.stream_ptr(dev))
        _lib.check(rc, "qd_spo2_run_ex")
        states = []
        if snap is not None:
            host = snap.cpu().numpy()
            states = [host[k] for k in range(nsnap)]
        return psi.cpu().numpy(), states

    def _kinetic_dev(self, dev):
        if self.coords == 'jacobi':
            return _dev_c128(np.broadcast_to(self.exp_Kx[:, None], (self.nx, self.ny)), dev), _dev_c128(self.exp_Ky, dev)
        return _dev_c128(self.exp_K, dev), None

    def _run_observed_dev(self, psi, dt, nt, nout, keep, basis, dev):
        """qd_spo2_run_observed on the device batch psi [B, nx, ny, ns] (in place): Strang steps, observables after
        every nout.  Returns (snap [B, nsnap, nx, ny, ns] or None, rdm [B, nsnap, ns, ns], mom [B, nsnap, 2, ns])."""
        B, ns = int(psi.shape[0]), self.ns
        nsnap = nt // nout
        rows = max(nsnap, 1)
        snap = torch.empty((B, nsnap, self.nx, self.ny, ns), dtype=torch.complex128, device=dev) \
            if keep and nsnap else None
        rdm = torch.zeros((B, rows, ns, ns), dtype=torch.complex128, device=dev)
        mom = torch.zeros((B, rows, 2, ns), dtype=torch.float64, device=dev)
        _, eVh = self._point_ops_dev(dev, need_full=False)
        eK, eKy = self._kinetic_dev(dev)
        x, y = _dev_f64(self.x, dev), _dev_f64(self.y, dev)
        with torch.cuda.device(dev):
            rc = _lib.load().qd_spo2_run_observed(psi.data_ptr(), B, eVh.data_ptr(), eK.data_ptr(), _lib.ptr(eKy),
                                                  self.nx, self.ny, ns, int(nsnap * nout), int(nout), _lib.ptr(snap),
                                                  _lib.ptr(basis), x.data_ptr(), y.data_ptr(),
                                                  _volume((self.x, self.y)), rdm.data_ptr(), mom.data_ptr(),
                                                  _lib.stream_ptr(dev))
        _lib.check(rc, "qd_spo2_run_observed")
        return snap, rdm[:, :nsnap], mom[:, :nsnap]

    def _run_observed(self, psi0, dt, nt, t0, nout, return_states, observe):
        """run(observe=...): Strang steps with the observables of psi0 and of the state after every nout steps."""
        dev = default_device()
        _lib.ensure_device(dev)
        basis = self._obs_basis(observe, dev)
        psi = _dev_c128(psi0, dev)[None].clone()
        snap, rdm, mom = self._run_observed_dev(psi, dt, nt, nout, return_states, basis, dev)
        rdm0, mom0 = self._first_row(psi0, basis, dev)
        rdm = torch.cat([rdm0, rdm[0]]).cpu().numpy()
        mom = torch.cat([mom0, mom[0]]).cpu().numpy()
        r = ResultSPO2(dt=dt, psi0=psi0, Nt=nt, t0=t0, nout=nout)
        r.x = self.x
        r.y = self.y
        r.psilist = [psi0]
        if snap is not None:
            host = snap[0].cpu().numpy()
            r.psilist += [host[k] for k in range(host.shape[0])]
        r.psi = psi[0].cpu().numpy()
        r.rdm = rdm
        r.population = np.ascontiguousarray(np.einsum('kaa->ka', rdm).real)
        r.xAve = [mom[:, 0].sum(axis=-1), mom[:, 1].sum(axis=-1)]
        r._recorded = (r.population, r.xAve[0], r.xAve[1])
        return r

    def _curvilinear_states(self, psi0s, dt, nt, nout):
        """curvilinear_run of psi0s [B, nx, ny, ns] on self.v and self.G: device tensors (psi, snap)."""
        if self.v is None:
            raise ValueError('The diabatic PES is not specified.')
        shape = tuple(psi0s.shape) if isinstance(psi0s, torch.Tensor) else np.shape(psi0s)
        if shape[1:] != (self.nx, self.ny, self.ns):
            raise ValueError(f"psi0s must be [B, {self.nx}, {self.ny}, {self.ns}]; got {shape}")
        return curvilinear_run(self.x, self.y, psi0s, self.v, self.G, dt, nt, nout)

    def _observe_snapshots(self, snap, basis):
        """rdm [B, nsnap, ns, ns] and mom [B, nsnap, 2, ns] of recorded states snap [B, nsnap, nx, ny, ns]
        (qd_spo_observe, after the run)."""
        B, nsnap, ns = int(snap.shape[0]), int(snap.shape[1]), self.ns
        if B * nsnap == 0:
            return (torch.zeros((B, nsnap, ns, ns), dtype=torch.complex128, device=snap.device),
                    torch.zeros((B, nsnap, 2, ns), dtype=torch.float64, device=snap.device))
        rdm, mom = observe_states(snap.reshape((B * nsnap,) + tuple(snap.shape[2:])), self._axes(), basis=basis)
        return rdm.reshape(B, nsnap, ns, ns), mom.reshape(B, nsnap, 2, ns)

    def _run_curvilinear(self, psi0, dt, nt, t0, nout, return_states, observe):
        """run on curvilinear coordinates: RK4 steps, the observables reduced from the recorded states after the run.
        The snapshots [nt // nout, nx, ny, ns] (16 (nt // nout) nx ny ns bytes) stay on the device until they are
        reduced, also with return_states=False, which only spares their copy to the host."""
        psi, snap = self._curvilinear_states(np.asarray(psi0)[None], dt, nt, nout)
        r = ResultSPO2(dt=dt, psi0=psi0, Nt=nt, t0=t0, nout=nout)
        r.x = self.x
        r.y = self.y
        r.psilist = [psi0]
        if return_states:
            host = snap[0].cpu().numpy()
            r.psilist += [host[k] for k in range(host.shape[0])]
        r.psi = psi[0].cpu().numpy()
        if observe is not None:
            basis = self._obs_basis(observe, psi.device)
            rdm0, mom0 = self._first_row(psi0, basis, psi.device)
            rdm, mom = self._observe_snapshots(snap, basis)
            rdm = torch.cat([rdm0, rdm[0]]).cpu().numpy()
            mom = torch.cat([mom0, mom[0]]).cpu().numpy()
            r.rdm = rdm
            r.population = np.ascontiguousarray(np.einsum('kaa->ka', rdm).real)
            r.xAve = [mom[:, 0].sum(axis=-1), mom[:, 1].sum(axis=-1)]
            r._recorded = (r.population, r.xAve[0], r.xAve[1])
        return r

    def run_batch(self, psi0s, dt=0.01, nt=1, nout=1, device=None, observe=None, keep_states=True):
        """Extension: B independent wavepackets psi0s [B, nx, ny, ns] on one potential, Strang steps as
        run(return_states=True) for each (qd_spo2_run_batch: one launch per pass for the whole batch).
        Returns (final states [B, nx, ny, ns], snapshots [B, nt//nout, nx, ny, ns]) as device tensors.
        Jacobi coordinates run the _KEO_jacobi step structure (qd_spo2_run_ex) member by member.

        observe ('diabatic', 'adiabatic' or a basis [nx, ny, ns, ns], see run) also reduces every recorded state
        inside the run (qd_spo2_run_observed) and returns (psi, snap or None, obs): obs is a dict of device tensors,
        rdm [B, nt//nout, ns, ns], mom [B, nt//nout, 2, ns] (mom[b, k, d, a] = <x_d> on state a) and population
        [B, nt//nout, ns], for the recorded states only (no psi0 row).  keep_states=False keeps no snapshots: the
        run then holds one scratch state per member instead of nt//nout.

        Curvilinear coordinates: curvilinear_run with self.v and self.G (RK4 steps; a device tensor psi0s stays on its
        device, `device` is not consulted), the same returns; observe reduces the recorded states after the run, so the
        snapshots are on the device until then whatever keep_states says."""
        self.build(dt=dt)
        if self.coords == 'curvilinear':
            psi, snap = self._curvilinear_states(psi0s, dt, nt, nout)
            if observe is None:
                return psi, snap
            rdm, mom = self._observe_snapshots(snap, self._obs_basis(observe, psi.device))
            return psi, (snap if keep_states else None), \
                {"rdm": rdm, "mom": mom, "population": torch.diagonal(rdm, dim1=-2, dim2=-1).real}
        dev = device or default_device()
        _lib.ensure_device(dev)
        psi = psi0s if isinstance(psi0s, torch.Tensor) else _dev_c128(psi0s, dev)
        psi = psi.to(device=dev, dtype=torch.complex128).contiguous().clone()
        B = psi.shape[0]
        if tuple(psi.shape[1:]) != (self.nx, self.ny, self.ns):
            raise ValueError(f"psi0s must be [B, {self.nx}, {self.ny}, {self.ns}]")
        nsnap = nt // nout
        if observe is not None:
            snap, rdm, mom = self._run_observed_dev(psi, dt, nt, nout, keep_states, self._obs_basis(observe, dev), dev)
            return psi, snap, {"rdm": rdm, "mom": mom, "population": torch.diagonal(rdm, dim1=-2, dim2=-1).real}
        snap = torch.empty((B, nsnap, self.nx, self.ny, self.ns), dtype=torch.complex128, device=dev) if nsnap \
            else None
        _, eVh = self._point_ops_dev(dev, need_full=False)
        if self.coords == 'jacobi':
            eK = _dev_c128(np.broadcast_to(self.exp_Kx[:, None], (self.nx, self.ny)), dev)
            eKy = _dev_c128(self.exp_Ky, dev)
            with torch.cuda.device(dev):
                for b in range(B):
                    rc = _lib.load().qd_spo2_run_ex(psi[b].data_ptr(), eVh.data_ptr(), None, eK.data_ptr(),
                                                    eKy.data_ptr(), self.nx, self.ny, self.ns, int(nsnap * nout),
                                                    int(nout), snap[b].data_ptr() if nsnap else None,
                                                    _lib.stream_ptr(dev))
                    _lib.check(rc, "qd_spo2_run_ex")
            return psi, snap
        eK = _dev_c128(self.exp_K, dev)
        with torch.cuda.device(dev):
            rc = _lib.load().qd_spo2_run_batch(psi.data_ptr(), B, eVh.data_ptr(), eK.data_ptr(), self.nx, self.ny,
                                               self.ns, int(nsnap * nout), int(nout), _lib.ptr(snap),
                                               _lib.stream_ptr(dev))
        _lib.check(rc, "qd_spo2_run_batch")
        return psi, snap

    def run(self, psi0, e_ops=[], dt=0.01, nt=1, t0=0., nout=1, return_states=True, observe=None):
        """wpd.py:692-758.  return_states=True: psilist = [psi0] + the state after every nout
        Strang steps (nt//nout*nout steps).  return_states=False: the merged-V arithmetic runs
        but, as in the reference, psilist is only [psi0].  r.psi is the final state (the
        reference leaves it unset).

        observe (extension; None changes nothing): 'diabatic', 'adiabatic' (M = d2a, see population) or an explicit
        basis [nx, ny, ns, ns].  The run then uses the Strang arithmetic whatever return_states says, and the
        populations, reduced density matrix and mean positions of psi0 and of the state after every nout steps are
        reduced on the device inside the run (qd_spo2_run_observed): r.population [nt//nout + 1, ns], r.rdm
        [nt//nout + 1, ns, ns], r.xAve = [xAve, yAve] (summed over states, as position()).  return_states=True keeps
        the states too; return_states=False keeps none -- psilist == [psi0], one state of device scratch instead of
        nt//nout, Strang not merged arithmetic -- and get_population() / position() return the recorded arrays.

        coords='curvilinear' (extension): nt//nout*nout RK4 steps of the G-matrix operator in place of Strang steps,
        the same psilist, r.psi and observe results (_run_curvilinear: observables reduced after the run)."""
        self.build(dt=dt)
        if self.coords == 'curvilinear':
            return self._run_curvilinear(psi0, dt, nt, t0, nout, return_states, observe)
        if observe is not None:
            return self._run_observed(psi0, dt, nt, t0, nout, return_states, observe)
        psi, states = self._propagate(psi0, dt, nt, nout, merged=not return_states)
        r = ResultSPO2(dt=dt, psi0=psi0, Nt=nt, t0=t0, nout=nout)
        r.x = self.x
        r.y = self.y
        r.psilist = [psi0] + (states if return_states else [])
        r.psi = psi
        return r


class SPO2NH(SPO2):
    """Drop-in for pyqed.wpd.SPO2NH (wpd.py:921-1081): complex (non-Hermitian) diabatic
    potential; exp_V = U_R e^{-i w dt} U_R^-1 from the right eigenvectors (nonherm.eig,
    nonherm.py:26-76, eigenvalues sorted by np.argsort)."""

    def __init__(self, x, y, *args, **kwargs):
        self.right_eigenstates = None
        super().__init__(x, y, *args, **kwargs)

    _ur = _ovlp = None

    def build(self, dt):
        """wpd.py:960-985.  exp_V = U_R e^{-i w dt} U_R^-1 is the matrix exponential exp(-i V dt); it is evaluated on
        the GPU (qd_spo_expm, scaling and squaring, no eigenvectors) for ns <= 1024.  The right eigenvectors and their
        overlap (right_eigenstates, ovlp_rr; nonherm.eig order, eigenvalues by argsort) are host eig results made
        on first access (position() reads ovlp_rr)."""
        if self.coords == 'curvilinear':
            raise NotImplementedError("SPO2NH with coords='curvilinear': the non-Hermitian class is not covered; "
                                      "SPO2(coords='curvilinear', G=G) propagates a complex potential (RK4 assumes no "
                                      "Hermiticity), without SPO2NH's right-eigenvector observables")
        nx, ny = self.nx, self.ny
        self.kx = 2. * np.pi * fftfreq(nx, interval(self.x))
        self.ky = 2. * np.pi * fftfreq(ny, interval(self.y))
        self._build_keo(dt)
        v = np.asarray(self.v, dtype=complex)
        self._ur = self._ovlp = None
        ns = v.shape[-1]
        _check_finite(v)
        if ns > DEVICE_EXPM_MAX_NS:
            ur = self.right_eigenstates
            w = self._w
            ul = np.linalg.inv(ur)
            self.exp_V = (ur * np.exp(-1j * w * dt)[..., None, :]) @ ul
            self.exp_V_half = (ur * np.exp(-1j * w * dt / 2)[..., None, :]) @ ul
            return
        dev = default_device()
        _lib.ensure_device(dev)
        vd = _dev_c128(v, dev)
        eV = torch.empty(v.shape, dtype=torch.complex128, device=dev)
        eVh = torch.empty_like(eV)
        with torch.cuda.device(dev):
            rc = _lib.load().qd_spo_expm(vd.data_ptr(), 0, int(v.size // (ns * ns)), ns, float(dt), eV.data_ptr(),
                                         eVh.data_ptr(), _lib.stream_ptr(dev))
        _lib.check(rc, "qd_spo_expm")
        self.exp_V, self.exp_V_half = None, None
        self._eV_dev, self._eVh_dev = eV, eVh

    def _host_eig_nh(self):
        w, ur = np.linalg.eig(np.asarray(self.v, dtype=complex))
        idx = np.argsort(w, axis=-1)
        self._w = np.take_along_axis(w, idx, axis=-1)
        self._ur = np.take_along_axis(ur, idx[..., None, :], axis=-1)
        self._ovlp = np.conj(np.swapaxes(self._ur, -1, -2)) @ self._ur

    @property
    def right_eigenstates(self):
        if self._ur is None and getattr(self, "v", None) is not None:
            self._host_eig_nh()
        return self._ur

    @right_eigenstates.setter
    def right_eigenstates(self, u):
        self._ur = u

    @property
    def ovlp_rr(self):
        if self._ovlp is None and getattr(self, "v", None) is not None:
            self._host_eig_nh()
        return self._ovlp

    def position(self, psilist):
        """wpd.py:997-1017 (no plot, no xAve.npz file)."""
        dx, dy = interval(self.x), interval(self.y)
        S = self.ovlp_rr
        xAve = [np.einsum('ijm, i, ijmn, ijn ->', psi.conj(), self.x, S, psi) * dx * dy for psi in psilist]
        yAve = [np.einsum('ijn, j, ijmn, ijn ->', psi.conj(), self.y, S, psi) * dx * dy for psi in psilist]
        self.xAve = [xAve, yAve]
        return xAve, yAve

    def run(self, psi0, e_ops=[], dt=0.01, nt=1, t0=0., nout=1, return_states=True, observe=None):
        """wpd.py:1019-1077: Strang steps (return_states=True) or the merged structure
        (False); psilist = [psi0] + the state after every nout steps in both cases; r.psi set.
        observe: as SPO2.run (Strang steps; with return_states=False no states are kept, psilist == [psi0]); the
        recorded quantities are the plain sums of SPO2.population / ResultSPO2.position, without the right-eigenvector
        overlap of SPO2NH.position, and decay with the norm."""
        self.build(dt=dt)
        if observe is not None:
            return self._run_observed(psi0, dt, nt, t0, nout, return_states, observe)
        psi, states = self._propagate(psi0, dt, nt, nout, merged=not return_states)
        r = ResultSPO2(dt=dt, psi0=psi0, Nt=nt, t0=t0, nout=nout)
        r.x = self.x
        r.y = self.y
        r.psilist = [psi0] + states
        r.psi = psi
        return r


def axis_propagator(k, m, dt):
    """First column m_a = ifft(e_a) of the circulant kinetic propagator of one axis, M_a = F^-1 diag(e_a) F with
    e_a = exp(-i k^2/(2m) dt) (M_a[i][j] = m_a[(i - j) mod n]; M_a @ v = ifft(e_a * fft(v))): exp_K of linear
    coordinates (wpd.py:1255-1262) is the outer product of the axis factors, so fftn, * exp_K, ifftn (wpd.py:1418-1432)
    is M_x (x) M_y (x) M_z.  Host setup, like exp_K itself."""
    k = np.asarray(k, dtype=float)
    return np.ascontiguousarray(np.fft.ifft(np.exp(-1j * k * k / 2. / m * dt)))


class SPO3(_PointPropagators):
    """Drop-in for pyqed.wpd.SPO3 (wpd.py:1105-1432), linear coordinates.

    kinetic_path: "auto" takes the separable kinetic step (qd_spo3_run_axes) when every axis has at most AXES_MAX_N
    points and there are one or two states: 64^3 as three register-FFT passes of F^-1 diag(e_a / n) F (22 us per
    64^3 x 2 step against 26 on the four passes of the 3-D exp_K), every other such grid as three per-axis mode
    products on the MFMAs (60^3 x 2: 31 us against 52 on the mixed-radix FFT passes; profiles/r06/spo/);
    larger grids or more states the FFT passes (qd_spo3_run).  "axes" / "fft" force one (tests).
    """

    AXES_MAX_N = 64
    kinetic_path = "auto"

    def _use_axes(self):
        dims = (self.nx, self.ny, self.nz)
        fits = max(dims) <= self.AXES_MAX_N and self.nstates <= 2
        if self.kinetic_path == "axes":
            if not fits:
                raise ValueError(f"kinetic_path='axes' needs every axis <= {self.AXES_MAX_N} points and nstates <= 2")
            return True
        if self.kinetic_path == "fft":
            return False
        return fits

    def __init__(self, x, y, z, masses, nstates=2, coords='linear', G=None, abc=False):
        self.x, self.y, self.z = x, y, z
        self.X, self.Y, self.Z = meshgrid(x, y, z)
        self.nx, self.ny, self.nz = len(x), len(y), len(z)
        self.dx, self.dy, self.dz = interval(x), interval(y), interval(z)
        self.masses = masses
        self.kx = self.ky = self.kz = None
        self.dim = 3
        self.exp_V = self.exp_V_half = self.exp_K = None
        self.V = None
        self.G = G
        self.nstates = nstates
        self.coords = coords
        self.abc = abc

    def set_grid(self, x, y, z):
        self.x, self.y, self.z = x, y, z

    def set_masses(self, masses):
        self.masses = masses

    def setG(self, G):
        self.G = G

    def set_DPES(self, surfaces, diabatic_couplings, eta=None):
        """wpd.py:1163-1200 (real array; couplings written symmetrically)."""
        ns = self.nstates
        v = np.zeros([self.nx, self.ny, self.nz, ns, ns])
        for a in range(ns):
            v[:, :, :, a, a] = surfaces[a]
        for dc in diabatic_couplings:
            a, b = dc[0][:]
            v[:, :, :, a, b] = v[:, :, :, b, a] = np.real(dc[1])
        self.V = v
        return v

    def build(self, dt, inertia=None):
        """wpd.py:1210-1340 (linear): exp_K on the 'ij' grid, exp(-i V dt/2) per point.
        coords='jacobi' is not a working path of the reference: its SPO3._KEO_jacobi (wpd.py:1434-1469) contracts the
        4-index wavefunction [nx, ny, nz, ns] with 'ij, ija -> ija' (the 2-D SPO2 form), which numpy rejects, and its
        build never forms a z kinetic factor; there is no step structure to reproduce, so it is refused here."""
        if self.coords == 'jacobi':
            raise NotImplementedError("SPO3 with coords='jacobi': the reference's _KEO_jacobi (wpd.py:1434-1469) is the "
                                      "2-D SPO2 operator applied to a 3-D grid and fails there; no 3-D Jacobi KEO exists")
        if self.coords == 'curvilinear':   # RK4 on the 3 x 3 G-matrix operator: no exp_K, no exp_V
            dims = (self.nx, self.ny, self.nz)
            if self.G is not None and len(_shape_of(self.G)) == 4:
                raise NotImplementedError("SPO3 with coords='curvilinear' needs a 3-D metric G [nx, ny, nz, 3, 3]; two "
                                          "curvilinear coordinates with a rectilinear third (a four-dimensional G "
                                          f"{_shape_of(self.G)}) are not built")
            _gmat_check_G(self.G, dims, f"the grid {dims}")
            self.kx, self.ky, self.kz = (_gmat_k(n, a) for n, a in zip(dims, self._axes()))
            self._d2a = self._apes = self._d2a_dev = None
            self._eig_pending = self.V is not None   # d2a for observe='adiabatic': host eigh on first access
            return
        if self.coords != 'linear':
            raise ValueError(f"unknown coordinates {self.coords!r}")
        self.kx = 2. * np.pi * fftfreq(self.nx, self.dx)
        self.ky = 2. * np.pi * fftfreq(self.ny, self.dy)
        self.kz = 2. * np.pi * fftfreq(self.nz, self.dz)
        mx, my, mz = self.masses
        Kx, Ky, Kz = meshgrid(self.kx, self.ky, self.kz)
        self.exp_K = np.exp(-1j * (Kx ** 2 / 2. / mx + Ky ** 2 / 2. / my + Kz ** 2 / 2. / mz) * dt)
        if self.V is None:
            raise ValueError('The diabatic PES is not specified.')
        self._build_point_ops(dt)

    def _pot(self):
        return self.V

    def _axes(self):
        return (self.x, self.y, self.z)

    def population(self, psi, representation='diabatic'):
        """Electronic populations of a state [nx, ny, nz, ns] -> [ns], a list -> [N, ns] (stacked arrays and device
        tensors as SPO2.population), reduced on the device.  Deviation: the reference's SPO3.population (wpd.py:1316-1346)
        indexes psi[:, :, j], which takes j along z, not the state, and weights by dx dy only; here the whole grid is
        summed per state with dx dy dz.  representation as SPO2.population (extension)."""
        return self._population(psi, representation)

    def run(self, psi0, e_ops=[], dt=0.01, nt=1, t0=0., nout=1, return_states=True, observe=None):
        """wpd.py:1349-1411: nt//nout*nout Strang steps; psilist = state after every nout steps
        (psi0 NOT included, as the reference); r.psi the final state.

        observe (extension, as SPO2.run): r.population [nt//nout + 1, ns], r.rdm [nt//nout + 1, ns, ns] and
        r.xAve = [xAve, yAve, zAve] of psi0 (row 0) and of the state after every nout steps, reduced inside the run
        (qd_spo3_run_observed); with return_states=False no states are kept (psilist == []).

        coords='curvilinear' (extension): nt//nout*nout RK4 steps of the 3 x 3 G-matrix operator on self.V
        (curvilinear_run3, qd_wp3_gmat_ms_rk4) with the same psilist, r.psi and observe results; the observables are
        reduced from the recorded states after the run, as SPO2._run_curvilinear does."""
        self.build(dt=dt)
        if self.coords == 'curvilinear':
            return self._run_curvilinear(psi0, dt, nt, t0, nout, return_states, observe)
        dev = default_device()
        _lib.ensure_device(dev)
        nsteps = (nt // nout) * nout
        nsnap = nt // nout
        psi = _dev_c128(psi0, dev)
        shape = (self.nx, self.ny, self.nz, self.nstates)
        observed = observe is not None
        keep = return_states or not observed
        snap = torch.empty((nsnap,) + shape, dtype=torch.complex128, device=dev) if nsnap and keep else None
        _, eVh = self._point_ops_dev(dev)
        if observed:
            ns = self.nstates
            basis = self._obs_basis(observe, dev)
            rdm = torch.zeros((max(nsnap, 1), ns, ns), dtype=torch.complex128, device=dev)
            mom = torch.zeros((max(nsnap, 1), 3, ns), dtype=torch.float64, device=dev)
            if self._use_axes():
                M = [_dev_c128(axis_propagator(k, m, dt), dev)
                     for k, m in zip((self.kx, self.ky, self.kz), self.masses)]
                kin = [None] + [m.data_ptr() for m in M]
            else:
                eK = _dev_c128(self.exp_K, dev)
                kin = [eK.data_ptr(), None, None, None]
            ax = [_dev_f64(a, dev) for a in self._axes()]
            with torch.cuda.device(dev):
                rc = _lib.load().qd_spo3_run_observed(psi.data_ptr(), eVh.data_ptr(), *kin, self.nx, self.ny, self.nz,
                                                      ns, int(nsteps), int(nout), _lib.ptr(snap), _lib.ptr(basis),
                                                      *(a.data_ptr() for a in ax), _volume(self._axes()),
                                                      rdm.data_ptr(), mom.data_ptr(), _lib.stream_ptr(dev))
            _lib.check(rc, "qd_spo3_run_observed")
            rdm0, mom0 = self._first_row(psi0, basis, dev)
            rdm = torch.cat([rdm0, rdm[:nsnap]]).cpu().numpy()
            mom = torch.cat([mom0, mom[:nsnap]]).cpu().numpy()
        elif self._use_axes():
            M = [_dev_c128(axis_propagator(k, m, dt), dev) for k, m in zip((self.kx, self.ky, self.kz), self.masses)]
            with torch.cuda.device(dev):
                rc = _lib.load().qd_spo3_run_axes(psi.data_ptr(), eVh.data_ptr(), *(m.data_ptr() for m in M),
                                                  self.nx, self.ny, self.nz, self.nstates, int(nsteps), int(nout),
                                                  _lib.ptr(snap), _lib.stream_ptr(dev))
            _lib.check(rc, "qd_spo3_run_axes")
        else:
            eK = _dev_c128(self.exp_K, dev)
            with torch.cuda.device(dev):
                rc = _lib.load().qd_spo3_run(psi.data_ptr(), eVh.data_ptr(), eK.data_ptr(), self.nx, self.ny,
                                             self.nz, self.nstates, int(nsteps), int(nout), _lib.ptr(snap),
                                             _lib.stream_ptr(dev))
            _lib.check(rc, "qd_spo3_run")
        r = Result(dt=dt, psi0=psi0, Nt=nt, t0=t0, nout=nout)
        if snap is not None:
            host = snap.cpu().numpy()
            r.psilist = [host[k] for k in range(nsnap)]
        r.psi = psi.cpu().numpy()
        if observed:
            r.rdm = rdm
            r.population = np.ascontiguousarray(np.einsum('kaa->ka', rdm).real)
            r.xAve = [mom[:, d].sum(axis=-1) for d in range(3)]
        return r

    def _run_curvilinear(self, psi0, dt, nt, t0, nout, return_states, observe):
        """run on curvilinear coordinates (build has checked G).  The snapshots [nt // nout, nx, ny, nz, ns] stay on the
        device until they are reduced, also with return_states=False, which only spares their copy to the host."""
        if self.V is None:
            raise ValueError('The diabatic PES is not specified.')
        shape = (self.nx, self.ny, self.nz, self.nstates)
        if np.shape(psi0) != shape:
            raise ValueError(f"psi0 must be {list(shape)}; got {np.shape(psi0)}")
        psi, snap = curvilinear_run3(self.x, self.y, self.z, np.asarray(psi0)[None], self.V, self.G, dt, nt, nout)
        observed = observe is not None
        r = Result(dt=dt, psi0=psi0, Nt=nt, t0=t0, nout=nout)
        if return_states or not observed:
            host = snap[0].cpu().numpy()
            r.psilist = [host[k] for k in range(host.shape[0])]
        r.psi = psi[0].cpu().numpy()
        if observed:
            basis = self._obs_basis(observe, psi.device)
            rdm, mom = self._first_row(psi0, basis, psi.device)
            if snap.shape[1]:
                rdm1, mom1 = observe_states(snap[0], self._axes(), basis=basis)
                rdm, mom = torch.cat([rdm, rdm1]), torch.cat([mom, mom1])
            rdm, mom = rdm.cpu().numpy(), mom.cpu().numpy()
            r.rdm = rdm
            r.population = np.ascontiguousarray(np.einsum('kaa->ka', rdm).real)
            r.xAve = [mom[:, d].sum(axis=-1) for d in range(3)]
        return r


# ---------------------------------------------------------------------------------------------------------------------
# Curvilinear coordinates: the G-matrix kinetic operator and its RK4 propagation (wpd.py:1783-1940)

def _is_complex_nonzero(a):
    """A non-zero imaginary part anywhere.  Host data is checked on the host; a complex tensor that already lives on
    the device is reduced there (the one check that touches the device before a refusal)."""
    if isinstance(a, torch.Tensor):
        return a.is_complex() and bool((a.imag != 0).any())
    return np.iscomplexobj(a) and bool(np.any(np.imag(a) != 0))


_AXES = ("nx", "ny", "nz")


def _shape_of(a):
    return tuple(a.shape) if isinstance(a, torch.Tensor) else np.shape(a)


def _gmat_k(n, axis):
    """k = 2 pi fftfreq(n, d) of an axis of n points, zeros(1) for an axis of length 1."""
    return 2. * np.pi * fftfreq(n, interval(axis)) if n > 1 else np.zeros(1)


def _gmat_check_G(G, dims, what):
    D = len(dims)
    if G is None:
        raise ValueError(f"curvilinear coordinates need the metric G [{', '.join(_AXES[:D])}, {D}, {D}]")
    if _shape_of(G) != dims + (D, D):
        raise ValueError(f"G must be {dims + (D, D)} for {what}; got {_shape_of(G)}")
    if _is_complex_nonzero(G):
        raise ValueError("G must be real: the kernels read a float64 metric (a complex G is not supported)")


def _gmat_check(psi, G, v, nk):
    """Shape and type checks of a curvilinear call in D = len(nk) coordinates, before any device call for ndarray and
    host-tensor operands (a complex G held on the device is tested there).  With `grid` the D extents, v [grid] (or
    None) takes psi [grid] or a batch [B, grid]; v [grid, ns, ns] takes psi [grid, ns] or [B, grid, ns].  Returns
    (dims, ns, batched), ns = 0 on a single surface."""
    D = len(nk)
    grid = ", ".join(_AXES[:D])
    shape = _shape_of(psi)
    vshape = None if v is None else _shape_of(v)
    if vshape is not None and len(vshape) == D + 2:
        want = f"v [{grid}, ns, ns] needs psi [{grid}, ns] or a batch [B, {grid}, ns]"
        if len(shape) not in (D + 1, D + 2):
            raise ValueError(f"{want}; got psi {shape}")
        dims, ns = tuple(int(n) for n in shape[-D - 1:-1]), int(vshape[-1])
        if vshape != dims + (ns, ns) or ns < 1:
            raise ValueError(f"v must be [{grid}, ns, ns] = {dims} + (ns, ns) for psi {shape}; got {vshape}")
        if int(shape[-1]) != ns:
            raise ValueError(f"{want}: v {vshape} has ns = {ns}; got psi {shape}")
        batched = len(shape) == D + 2
    else:
        if len(shape) not in (D, D + 1):
            raise ValueError(f"psi must be [{grid}] or a batch [B, {grid}]; got {shape}")
        dims, ns, batched = tuple(int(n) for n in shape[-D:]), 0, len(shape) == D + 1
        if vshape is not None and vshape != dims:
            raise ValueError(f"v must be {dims} (or [{grid}, ns, ns]) for psi {shape}; got {vshape}")
    _gmat_check_G(G, dims, f"psi {shape}")
    if tuple(nk) != dims:
        raise ValueError(f"{', '.join('k' + a[1] for a in _AXES[:D])} have lengths {tuple(nk)}; psi {shape} needs "
                         f"{dims}")
    return dims, ns, batched


def _gmat_dev(psi, G, v, ks, ns, copy=False):
    """Device operands in the kernels' plane layout: psi [B, max(ns, 1), *dims], G float64, V [ns, ns, *dims] or
    v [*dims] complex128 or None, and the k vectors float64.  On a single surface a contiguous complex128 device tensor
    is used in place, not copied (its state axis of size 1 is a view); copy=True makes the planes a tensor of their
    own, for a run, which advances them in place."""
    dev = psi.device if isinstance(psi, torch.Tensor) and psi.device.type == "cuda" else default_device()
    _lib.ensure_device(dev)
    t = psi.to(device=dev, dtype=torch.complex128) if isinstance(psi, torch.Tensor) else _dev_c128(psi, dev)
    if t.dim() == len(ks) + (1 if ns else 0):
        t = t[None]
    t = t.movedim(-1, 1) if ns else t[:, None]
    t = t.clone(memory_format=torch.contiguous_format) if copy else t.contiguous()
    if isinstance(G, torch.Tensor):
        Gd = (G.real if G.is_complex() else G).to(device=dev, dtype=torch.float64).contiguous()
    else:
        Gd = _dev_f64(np.real(G), dev)
    vd = None
    if v is not None:
        vd = v.to(device=dev, dtype=torch.complex128) if isinstance(v, torch.Tensor) else _dev_c128(v, dev)
        vd = (vd.movedim((-2, -1), (0, 1)) if ns else vd).contiguous()
    f64 = lambda k: k.to(device=dev, dtype=torch.float64).contiguous() if isinstance(k, torch.Tensor) \
        else _dev_f64(k, dev)
    return dev, t, Gd, vd, [f64(k) for k in ks]


def _gmat_call(what, dev, t, ns, Gd, vd, kd, dims, *tail):
    """qd_wp{D}_gmat[_ms]_{what} on the planes t [B, max(ns, 1), *dims]: D and ns name the entry point."""
    name = f"qd_wp{len(dims)}_gmat{'_ms' if ns else ''}_{what}"
    head = (t.data_ptr(), int(t.shape[0])) + ((ns,) if ns else ())
    with torch.cuda.device(dev):
        rc = getattr(_lib.load(), name)(*head, Gd.data_ptr(), _lib.ptr(vd), *(k.data_ptr() for k in kd), *dims, *tail,
                                        _lib.stream_ptr(dev))
    _lib.check(rc, name)


def _gmat_apply(psi, ks, v, G):
    """(K + v) psi on the device in len(ks) coordinates (qd_wp{2,3}_gmat_apply, or the _ms_apply call for
    v [grid, ns, ns]); returns a device tensor shaped like psi."""
    dims, ns, batched = _gmat_check(psi, G, v, [len(k) for k in ks])
    dev, t, Gd, vd, kd = _gmat_dev(psi, G, v, ks, ns)
    out = torch.empty_like(t)
    _gmat_call("apply", dev, t, ns, Gd, vd, kd, dims, out.data_ptr())
    out = out.movedim(1, -1).contiguous() if ns else out[:, 0]
    return out if batched else out[0]


def _gmat_run(axes, psi0s, v, G, dt, nt, nout):
    """(nt // nout) nout RK4 steps on the coordinate arrays `axes` (qd_wp{2,3}_gmat_rk4, or the _ms_rk4 call for
    v [grid, ns, ns]): device tensors (final states [B, grid], snapshots [B, nt // nout, grid]), with a trailing state
    axis on coupled surfaces.  psi0s is not modified."""
    if nout < 1 or nt < 0:
        raise ValueError(f"nt = {nt} must be >= 0 and nout = {nout} >= 1")
    dims, ns, _ = _gmat_check(psi0s, G, v, [len(a) for a in axes])
    ks = [_gmat_k(n, a) for n, a in zip(dims, axes)]
    dev, psi, Gd, vd, kd = _gmat_dev(psi0s, G, v, ks, ns, copy=True)
    B, nsnap = int(psi.shape[0]), int(nt) // int(nout)
    snap = torch.empty((B, nsnap, max(ns, 1)) + dims, dtype=torch.complex128, device=dev)
    _gmat_call("rk4", dev, psi, ns, Gd, vd, kd, dims, float(dt), nsnap * int(nout), int(nout),
               snap.data_ptr() if nsnap else None)
    if ns:
        return psi.movedim(1, -1).contiguous(), snap.movedim(2, -1).contiguous()
    return psi[:, 0], snap[:, :, 0]


def _like_input(out, psi):
    """The device result where the input lives: an ndarray for an ndarray, a tensor on psi's device for a tensor."""
    return out.to(psi.device) if isinstance(psi, torch.Tensor) else out.cpu().numpy()


def KEO(psi, kx, ky, G):
    """wpd.py:1861-1915: K psi = 1/2 sum_rs p_r G_rs p_s psi, with p_x psi = ifft2(kx fft2 psi) (the transform along
    the other axis cancels: one line transform pair per derivative).  G [nx, ny, 2, 2] real, all four entries read.
    Extensions: psi may carry a leading batch axis [B, nx, ny]; a tensor in gives a tensor out on the same device (a
    device tensor stays on the device, a host tensor comes back to the host)."""
    return _like_input(_gmat_apply(psi, (kx, ky), None, G), psi)


def PEO(psi, v):
    """wpd.py:1917-1933: v psi."""
    return v * psi


def hpsi(psi, kx, ky, v, G):
    """wpd.py:1935-1940: -1j (K psi + v psi), one library call for K psi + v psi; v real or complex.
    Extension: v [nx, ny, ns, ns] (any complex matrix per point) with psi [nx, ny, ns] or [B, nx, ny, ns] is the
    coupled-surface operator, -1j (K psi_a + sum_b v_ab psi_b)."""
    return _like_input(-1j * _gmat_apply(psi, (kx, ky), v, G), psi)


def curvilinear_run(x, y, psi0s, v, G, dt, nt, nout=1):
    """Extension: RK4 propagation of B wavepackets psi0s [B, nx, ny] (or one, [nx, ny]) in curvilinear coordinates on
    one potential and metric (qd_wp2_gmat_rk4, one launch per pass for the whole batch).  Runs (nt // nout) nout steps,
    as SPO2.run_batch; returns (final states [B, nx, ny], snapshots [B, nt // nout, nx, ny]) as device tensors,
    whatever psi0s was (ndarray, host or device tensor).  psi0s is not modified.

    Coupled surfaces: v [nx, ny, ns, ns] with psi0s [B, nx, ny, ns] (or one, [nx, ny, ns]) integrates
    i dpsi_a/dt = K psi_a + sum_b v_ab psi_b (qd_wp2_gmat_ms_rk4) and returns ([B, nx, ny, ns],
    [B, nt // nout, nx, ny, ns]).  The kernels hold the states as planes; the permutes happen on the device."""
    return _gmat_run((x, y), psi0s, v, G, dt, nt, nout)


def adiabatic_2d(x, y, psi0, v, dt, Nt=0, coords='linear', mass=None, G=None):
    """wpd.py:1783-1859, coords='curvilinear': Nt RK4 steps (phys.rk4, phys.py:1051-1064, in Horner form) of
    i dpsi/dt = (K + v) psi with hpsi (wpd.py:1935-1940); kx, ky = 2 pi fftfreq(n, dx) as the reference builds them.
    Returns the final psi (psi0 is untouched; Nt=0 returns a copy); `mass` is unused on this branch, as there.

    coords='linear' raises NotImplementedError: the reference's branch fails in x_evolve_2d (wpd.py:1826, an einsum
    with 4-index subscripts on a 2-D array) before its first step, and a broken path is not reproduced as a failure;
    SPO2(x, y, mass, nstates=1) is the split-operator propagation on one surface.  Any other coords raises ValueError
    (the reference silently returns a copy of psi0).

    Extensions: psi0 may carry a leading batch axis [B, nx, ny]; a tensor in gives a tensor out on the same device.
    The refusals below come before any device call, but for a complex G that already lives on the device, whose
    imaginary part is tested there."""
    if coords == 'linear':
        raise NotImplementedError(
            "adiabatic_2d(coords='linear'): the reference's branch is broken (x_evolve_2d raises ValueError, "
            "wpd.py:1826); use SPO2(x, y, mass, nstates=1) for split-operator dynamics on one surface")
    if coords != 'curvilinear':
        raise ValueError(f"coords = {coords!r}; adiabatic_2d knows 'curvilinear' (and refuses 'linear')")
    dims, ns, batched = _gmat_check(psi0, G, v, (len(x), len(y)))
    if ns:
        raise ValueError(f"v must be {dims} for psi {_shape_of(psi0)}; got {_shape_of(v)} (coupled surfaces: "
                         "curvilinear_run)")
    psi, _ = curvilinear_run(x, y, psi0, v, G, dt, int(Nt), 1)
    return _like_input(psi if batched else psi[0], psi0)


# ---------------------------------------------------------------------------------------------------------------------
# Three curvilinear coordinates (extension): the 3 x 3 G-matrix operator and its RK4 propagation

def KEO3(psi, kx, ky, kz, G):
    """Extension: K psi = 1/2 sum_rs p_r G_rs p_s psi in three curvilinear coordinates, p_a psi = IFFT_a(k_a FFT_a psi),
    G [nx, ny, nz, 3, 3] real with all nine entries read.  psi [nx, ny, nz] or a batch [B, nx, ny, nz]; ndarray in
    gives ndarray out, a tensor comes back on its own device, as KEO."""
    return _like_input(_gmat_apply(psi, (kx, ky, kz), None, G), psi)


def hpsi3(psi, kx, ky, kz, v, G):
    """Extension: -1j (K psi + v psi) with KEO3's K; v [nx, ny, nz] real or complex.  v [nx, ny, nz, ns, ns] with
    psi [nx, ny, nz, ns] or [B, nx, ny, nz, ns] is the coupled-surface operator, -1j (K psi_a + sum_b v_ab psi_b)."""
    return _like_input(-1j * _gmat_apply(psi, (kx, ky, kz), v, G), psi)


def curvilinear_run3(x, y, z, psi0s, v, G, dt, nt, nout=1):
    """Extension: curvilinear_run in three coordinates (qd_wp3_gmat_rk4; v [nx, ny, nz, ns, ns]: qd_wp3_gmat_ms_rk4).
    Runs (nt // nout) nout RK4 steps of B wavepackets psi0s [B, nx, ny, nz] (or one) on one potential and metric
    G [nx, ny, nz, 3, 3]; returns (final states [B, nx, ny, nz], snapshots [B, nt // nout, nx, ny, nz]) as device
    tensors, with a trailing state axis on coupled surfaces.  psi0s is not modified."""
    return _gmat_run((x, y, z), psi0s, v, G, dt, nt, nout)
