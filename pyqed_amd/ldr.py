"""Conical-intersection dynamics in the local diabatic representation on MI355X (drop-in for pyqed/ldr/ldr.py LDR2,
LDRN, LDR2_Jacobi, ResultLDR and for the sine DVR of pyqed/dvr/dvr_1d.py they are built on).

The reference propagates psi[i, j, a] (grid point, adiabatic state) with a Strang splitting whose kinetic factor
exp_T[ija, klb] = A[ija, klb] expKx[i, k] expKy[j, l], A = U(R_ij)^+ U(R_kl), it materialises as a dense
(nx ny ns)^2 array.  A is a Gram matrix, so the step factorises: expand psi with U, one dense mode product per axis,
project with U^+ (csrc/ldr_plan.hpp).  Every step runs in libqdyn (qd_ldr_run); nothing of size npts^2 is formed by
run().  Setup (eigh of the diabatic potential, the DVR propagators, np.exp of the surfaces) is host work, as in the
reference, so the phases are the reference's own values.

LDR2_Jacobi (ldr.py:1779-1987), whose angular propagator differs for every row of the grid, runs the same way with two
real sine-transform passes around a phase table in place of the last axis' matrix (qd_ldr_jacobi_run).

Dense objects of the reference's interface (A, short_time_propagator, rdm_nuc) are offered up to D = npts ns <=
DENSE_MAX_D and refused with a message above it.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib
from ._util import default_device
from .wpd import ResultSPO2, interval, observe_states

DENSE_MAX_D = 4096          # D = npts * ns up to which A, short_time_propagator and rdm_nuc are formed (256 MiB at D)
MAX_DIM = 3                 # qd_ldr_run: ndim in [1, 3]
LDR_PATHS = {"auto": 0, "fused": 1, "split": 2}


# --------------------------------------------------------------------------- sine DVR
class sine_dvr:
    """Sine (particle-in-a-box) DVR with `npts` grid points strictly inside (xmin, xmax); the interface of the
    reference's SineDVR (dvr_1d.py:575-732): x, t(), expT(dt), fbr2dvr().

    The box eigenfunctions sqrt(2 / L) sin(k pi (x - xmin) / L), k = 1 .. npts, have kinetic energies
    E_k = (k pi / L)^2 / (2 mass).  Sampled on the grid they form the orthogonal, symmetric sine-transform matrix S, so
    every function of the kinetic operator is S f(E) S in the DVR: t() with f = identity, expT(dt) with
    f = exp(-i E dt)."""

    def __init__(self, xmin, xmax, npts, mass=1):
        npts = int(npts)
        if npts < 1 or not xmax > xmin:
            raise ValueError(f"sine_dvr: needs npts >= 1 and xmax > xmin; got {npts}, ({xmin}, {xmax})")
        self.npts, self.xmin, self.xmax, self.mass = npts, xmin, xmax, mass
        self.L = float(xmax) - float(xmin)
        self.n = 1 + np.arange(npts)                       # basis and grid labels
        self.dx = self.L / (npts + 1)
        self.x = float(xmin) + self.n * self.dx
        self.T = self.U = None

    def levels(self):
        """E_k, the kinetic energies of the box eigenfunctions."""
        return np.square(self.n * (np.pi / self.L)) / (2.0 * self.mass)

    def fbr2dvr(self):
        """S[k, a] = sqrt(2 / (npts + 1)) sin(pi k a / (npts + 1)): basis function k at grid point a."""
        ka = np.multiply.outer(self.n, self.n)
        self.U = np.sqrt(2.0 / (self.npts + 1)) * np.sin(ka * np.pi / (self.npts + 1))
        return self.U

    def _function(self, f):
        S = self.fbr2dvr()
        return (S * f[None, :]) @ S                        # S is symmetric: S diag(f) S

    def t(self):
        """The kinetic-energy matrix on the grid, real symmetric."""
        self.T = self._function(self.levels())
        return self.T

    def expT(self, dt=1):
        """exp(-i T dt) on the grid: complex symmetric and unitary."""
        return self._function(np.exp(-1j * dt * self.levels()))


# --------------------------------------------------------------------------- tensor-level call
def _dev(a, dev):
    if isinstance(a, torch.Tensor):
        return a.to(device=dev, dtype=torch.complex128).contiguous()
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=complex))).to(dev)


def _ldr_inputs(fn, psi, U, apes, expK, ndim, dt, nt, nout, path, expV, expVh, snap):
    """The checks ldr_run and ldr_jacobi_run share; everything the C call takes but the kinetic factor."""
    if path not in LDR_PATHS:
        raise ValueError(f"{fn}: path={path!r}, expected one of {sorted(LDR_PATHS)}")
    if not isinstance(psi, torch.Tensor) or psi.dtype != torch.complex128:
        raise ValueError(f"{fn}: psi must be a torch complex128 tensor on the device")
    dev = psi.device
    _lib.ensure_device(dev)
    if psi.dim() != ndim + 2:
        raise ValueError(f"{fn}: psi must be [B, {'n, ' * ndim}ns] for {ndim} axes; got {tuple(psi.shape)}")
    B, dims, ns = int(psi.shape[0]), tuple(int(n) for n in psi.shape[1:-1]), int(psi.shape[-1])
    U = _dev(U, dev)
    if U.dim() != ndim + 2 or tuple(U.shape[:ndim]) != dims or U.shape[-1] != ns:
        raise ValueError(f"{fn}: U must be {dims + ('M', ns)}; got {tuple(U.shape)}")
    if expV is None or expVh is None:
        if isinstance(apes, torch.Tensor):
            apes = apes.detach().cpu().numpy()
        apes = np.asarray(apes)
        if apes.shape != dims + (ns,):
            raise ValueError(f"{fn}: apes must be {dims + (ns,)}; got {apes.shape}")
        expV, expVh = np.exp(-1j * dt * apes), np.exp(-1j * (0.5 * dt) * apes)
    expV, expVh = _dev(expV, dev), _dev(expVh, dev)
    if tuple(expV.shape) != dims + (ns,) or tuple(expVh.shape) != dims + (ns,):
        raise ValueError(f"{fn}: expV and expVh must be {dims + (ns,)}")
    Ks = [_dev(k, dev) for k in expK]
    for d, k in enumerate(Ks):
        if tuple(k.shape) != (dims[d], dims[d]):
            raise ValueError(f"{fn}: expK[{d}] must be {(dims[d], dims[d])}; got {tuple(k.shape)}")
    nout = int(nout)
    nsnap = int(nt) // nout if nout >= 1 else 0
    if snap is None:
        snap = torch.empty((B, nsnap) + dims + (ns,), dtype=torch.complex128, device=dev)
    elif tuple(snap.shape) != (B, nsnap) + dims + (ns,) or snap.dtype != torch.complex128 or snap.device != dev \
            or not snap.is_contiguous():
        raise ValueError(f"{fn}: snap must be a contiguous complex128 {(B, nsnap) + dims + (ns,)} on {dev}")
    return dev, B, dims, ns, U, expV, expVh, Ks, nout, nsnap, snap


def _ldr_result(snap, return_states, weight):
    """The snapshots, or their populations and electronic density matrices reduced on the device."""
    if return_states:
        return snap
    B, nsnap, dims, ns = int(snap.shape[0]), int(snap.shape[1]), tuple(snap.shape[2:-1]), int(snap.shape[-1])
    if nsnap == 0:
        return (torch.empty((B, 0, ns), dtype=torch.float64, device=snap.device),
                torch.empty((B, 0, ns, ns), dtype=torch.complex128, device=snap.device))
    rdm, _ = observe_states(snap.reshape((B * nsnap,) + dims + (ns,)), [np.arange(n) for n in dims], weight=weight,
                            moments=False)
    rdm = rdm.reshape(B, nsnap, ns, ns)
    return torch.diagonal(rdm, dim1=-2, dim2=-1).real.contiguous(), rdm


def ldr_run(psi, U, apes, expK, dt, nt, nout=1, path="auto", return_states=True, weight=1.0, expV=None, expVh=None,
            snap=None):
    """Batched LDR split-operator run on the GPU (qd_ldr_run).

    psi [B, n0(, n1(, n2)), ns] torch complex128 on the device (read only); U [n0, ..., M, ns] the kept adiabatic
    states; apes [n0, ..., ns] the surfaces (host or device: exp(-i apes dt) and exp(-i apes dt / 2) are taken on the
    host with np.exp, the reference's values; expV / expVh override them); expK the per-axis kinetic propagators
    [n_d, n_d].  Step structure of the reference: * expVh, then nt // nout blocks of nout x (kinetic, * expV) with a
    snapshot after each block.  Returns the snapshots [B, nt // nout, n0, ..., ns] on the device, or with
    return_states=False (populations [B, nt // nout, ns], rdm [B, nt // nout, ns, ns]) reduced on the device from the
    snapshot buffer (observe_states, times `weight`); the states are then never copied to the host.
    path: "auto", "fused" or "split".  snap may be passed in; with it and U, expV, expVh and expK given as complex128
    device tensors the call does nothing but launch, so it can be captured into a graph that replays into snap."""
    ndim = len(expK)
    dev, B, dims, ns, U, expV, expVh, Ks, nout, nsnap, snap = _ldr_inputs("ldr_run", psi, U, apes, expK, ndim, dt, nt,
                                                                          nout, path, expV, expVh, snap)
    M = int(U.shape[-2])
    cdims = (_lib.c_int * ndim)(*dims)
    kp = [Ks[d].data_ptr() if d < ndim else None for d in range(MAX_DIM)]
    with torch.cuda.device(dev):
        rc = _lib.load().qd_ldr_run(_lib.ptr(psi), B, ndim, cdims, M, ns, U.data_ptr(), expV.data_ptr(),
                                    expVh.data_ptr(), kp[0], kp[1], kp[2], int(nt), nout, snap.data_ptr(),
                                    LDR_PATHS[path], _lib.stream_ptr(dev))
    _lib.check(rc, "qd_ldr_run")
    return _ldr_result(snap, return_states, weight)


def _dev_real(a, dev):
    if isinstance(a, torch.Tensor):
        return a.to(device=dev, dtype=torch.float64).contiguous()
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=float))).to(dev)


def ldr_jacobi_run(psi, U, apes, F, Fb, ph, expK, dt, nt, nout=1, path="auto", return_states=True, weight=1.0,
                   expV=None, expVh=None, snap=None):
    """ldr_run for a kinetic factor whose last-axis propagator differs for every row of the grid but shares its
    eigenvectors (qd_ldr_jacobi_run): per step chi = expand(psi); chi <- F chi along the last axis, times ph; chi <-
    expK[d] chi along every other axis; chi <- Fb chi along the last axis; psi' = expV project(chi).

    F, Fb [n_last, n_last] real; ph [n0, ..., n_last] complex, the grid's shape with the index of F's rows in the last
    axis' place; expK the list of the ndim - 1 plain-axis matrices.  Everything else, the return values and the
    graph-capture contract (F and Fb then float64, the rest complex128 device tensors) are ldr_run's."""
    fn = "ldr_jacobi_run"
    ndim = len(expK) + 1
    dev, B, dims, ns, U, expV, expVh, Ks, nout, nsnap, snap = _ldr_inputs(fn, psi, U, apes, expK, ndim, dt, nt, nout,
                                                                          path, expV, expVh, snap)
    M = int(U.shape[-2])
    if any(a.is_complex() if isinstance(a, torch.Tensor) else np.iscomplexobj(a) for a in (F, Fb)):
        raise ValueError(f"{fn}: F and Fb must be real")
    F, Fb, ph = _dev_real(F, dev), _dev_real(Fb, dev), _dev(ph, dev)
    if tuple(F.shape) != (dims[-1],) * 2 or tuple(Fb.shape) != (dims[-1],) * 2:
        raise ValueError(f"{fn}: F and Fb must be {(dims[-1],) * 2}; got {tuple(F.shape)}, {tuple(Fb.shape)}")
    if tuple(ph.shape) != dims:
        raise ValueError(f"{fn}: ph must be {dims}; got {tuple(ph.shape)}")
    cdims = (_lib.c_int * ndim)(*dims)
    kp = [Ks[d].data_ptr() if d < ndim - 1 else None for d in range(MAX_DIM - 1)]
    with torch.cuda.device(dev):
        rc = _lib.load().qd_ldr_jacobi_run(_lib.ptr(psi), B, ndim, cdims, M, ns, U.data_ptr(), expV.data_ptr(),
                                           expVh.data_ptr(), F.data_ptr(), Fb.data_ptr(), ph.data_ptr(), kp[0], kp[1],
                                           int(nt), nout, snap.data_ptr(), LDR_PATHS[path], _lib.stream_ptr(dev))
    _lib.check(rc, "qd_ldr_jacobi_run")
    return _ldr_result(snap, return_states, weight)


# --------------------------------------------------------------------------- results
class ResultLDR(ResultSPO2):
    """ldr.py:285-318.  get_population sums |psi[..., n]|^2 prod(dx) over the grid; the reference's takes psi[:, :, n]
    and so runs in two dimensions only, where the two agree."""

    def __init__(self, dx=None, **kwargs):
        super().__init__(**kwargs)
        self.dx = dx

    def get_population(self, fname=None, plot=False):
        d = np.prod(self.dx)
        p = np.array([[np.vdot(psi[..., n], psi[..., n]).real * d for n in range(self.nstates)]
                      for psi in self.psilist])
        self.population = p
        if fname is not None:
            np.savez(fname, p)
        if plot:
            import matplotlib.pyplot as plt
            fig, ax = plt.subplots()
            for n in range(self.nstates):
                ax.plot(self.times, p[:, n], label=str(n))
            plt.legend()
            return fig, ax
        return p


# --------------------------------------------------------------------------- solvers
class _LDR:
    """What LDR2 and LDRN share: surfaces, states, propagators and the runs on a product grid of self._axes()."""

    def _init_state(self):
        self.H = None
        self.K = None
        self.exp_K = None
        self.exp_V = None
        self.exp_V_half = None
        self.exp_T = None
        self._v = None
        self._apes = None
        self.adiabatic_states = None
        self.electronic_overlap = self.A = None

    @property
    def apes(self):
        return self._apes

    @apes.setter
    def apes(self, v):
        self._apes = v

    def _shape(self):
        return tuple(len(a) for a in self._axes())

    def _D(self):
        return int(np.prod(self._shape())) * self.nstates

    def _states(self):
        U = self.adiabatic_states
        if U is None or (isinstance(U, list) and not U):
            if self.A is not None:
                raise ValueError(f"{type(self).__name__}: only the dense overlap A was given; the propagation is "
                                 "matrix-free and needs the states it is built from: set adiabatic_states "
                                 "[*nx, M, nstates] (and apes [*nx, nstates])")
            if self._v is None:
                raise ValueError(f"{type(self).__name__}: set v (diabatic potential) or apes and adiabatic_states first")
            self.build_apes()
            U = self.adiabatic_states
        U = np.asarray(U)
        if U.ndim != len(self._shape()) + 2 or U.shape[:-2] != self._shape() or U.shape[-1] != self.nstates \
                or U.shape[-2] < self.nstates:
            raise ValueError(f"{type(self).__name__}: adiabatic_states must be {self._shape() + ('M', self.nstates)} "
                             f"with M >= nstates; got {U.shape}")
        return U

    def build_apes(self):
        """Adiabatic surfaces and states of the diabatic potential v by a batched host eigh, ascending
        (ldr.py:1306-1348; the reference's LDRN calls a build_apes it never defines)."""
        if self._v is None:
            raise ValueError(f"{type(self).__name__}.build_apes: the diabatic potential v is not set")
        w, u = np.linalg.eigh(self._v)
        self.apes = w
        self.adiabatic_states = u
        return w

    def buildV(self, dt):
        """ldr.py:1440-1443, 483-486"""
        self.exp_V = np.exp(-1j * dt * self.apes)
        self.exp_V_half = np.exp(-1j * (0.5 * dt) * self.apes)

    def _dvrs(self):
        raise NotImplementedError

    def buildK(self, dt):
        dvrs = self._dvrs()
        self.K = [d.t() for d in dvrs]
        self.exp_K = [d.expT(dt) for d in dvrs]
        return self.exp_K

    def _prepare(self, dt):
        U = self._states()
        if self.apes is None:
            raise ValueError(f"{type(self).__name__}: apes [*nx, nstates] must be set with adiabatic_states")
        if np.shape(self.apes) != self._shape() + (self.nstates,):
            raise ValueError(f"{type(self).__name__}: apes must be {self._shape() + (self.nstates,)}; "
                             f"got {np.shape(self.apes)}")
        self.buildV(dt)
        self._build_kinetic(dt)
        return U

    def _build_kinetic(self, dt):
        """What a run needs of the kinetic factor."""
        self.buildK(dt)

    def _launch(self, psi, U, dt, nt, nout, **kw):
        """The run on the device with the kinetic factor _build_kinetic left."""
        return ldr_run(psi, U, None, self.exp_K, dt, nt, nout, **kw)

    def _dense_check(self, what):
        if self._D() > DENSE_MAX_D:
            raise ValueError(f"{type(self).__name__}.{what}: D = npts * nstates = {self._D()} exceeds {DENSE_MAX_D}; "
                             f"the dense [{self._D()}, {self._D()}] array is not formed (run() does not need it)")

    def build_ovlp(self, dtype=None):
        """The dense electronic overlap A[i.., a, k.., b] = sum_mu conj(U[i.., mu, a]) U[k.., mu, b] on the host
        (ldr.py:1479-1527), for users who read sol.A; D <= DENSE_MAX_D.  run() never needs it."""
        self._dense_check("build_ovlp")
        U = self._states()
        sh, ns = self._shape(), self.nstates
        u = U.reshape(-1, U.shape[-2], ns)
        A = np.einsum('pma,qmb->paqb', u.conj(), u).reshape(sh + (ns,) + sh + (ns,))
        if dtype is not None and not np.iscomplexobj(np.zeros(0, dtype=dtype)):
            A = A.real.astype(dtype)
        self.electronic_overlap = self.A = A
        return A

    def run_batch(self, psi0s, dt, nt, nout=1, path="auto", return_states=True):
        """B initial states [B, *nx, nstates] propagated together (extension).  Returns the snapshots
        [B, nt // nout, *nx, nstates] as a device tensor, or with return_states=False the populations and electronic
        density matrices of every snapshot (ldr_run)."""
        U = self._prepare(dt)
        dev = psi0s.device if isinstance(psi0s, torch.Tensor) and psi0s.is_cuda else default_device()
        psi = _dev(psi0s, dev)
        if tuple(psi.shape[1:]) != self._shape() + (self.nstates,):
            raise ValueError(f"run_batch: psi0s must be [B, {self._shape() + (self.nstates,)}]; got {tuple(psi.shape)}")
        return self._launch(psi, U, dt, nt, nout, path=path, return_states=return_states,
                            weight=float(np.prod(self._dx())), expV=self.exp_V, expVh=self.exp_V_half)

    def _run_states(self, psi0, dt, nt, nout):
        assert psi0.shape == self._shape() + (self.nstates,)
        snap = self.run_batch(np.asarray(psi0)[None], dt, nt, nout)
        return [psi0] + list(snap[0].cpu().numpy())

    def rdm_el(self, psi):
        """Electronic reduced density matrix (times the volume element) of a state, or of each state of a list,
        reduced on the device (observe_states)."""
        if isinstance(psi, list):
            rdm, _ = observe_states(np.array(psi), self._axes(), weight=float(np.prod(self._dx())), moments=False)
            return list(rdm.cpu().numpy())
        rdm, _ = observe_states(psi, self._axes(), weight=float(np.prod(self._dx())), moments=False)
        return rdm.cpu().numpy()

    def short_time_propagator(self, dt):
        """exp_V_half exp_T exp_V_half in the reference's [*nx, ns, *nx, ns] layout (ldr.py:1719-1741, 525-548): the
        identity run as a batch of D unit vectors through one kinetic step; D <= DENSE_MAX_D."""
        self._dense_check("short_time_propagator")
        U = self._prepare(dt)
        D = self._D()
        dev = default_device()
        eye = torch.eye(D, dtype=torch.complex128, device=dev).reshape((D,) + self._shape() + (self.nstates,))
        # one step whose closing factor is the half step: snapshot = exp_V_half exp_T exp_V_half e_m
        snap = self._launch(eye, U, dt, 1, 1, expV=self.exp_V_half, expVh=self.exp_V_half)
        out = snap.reshape(D, D).T.contiguous().cpu().numpy()
        return out.reshape(self._shape() + (self.nstates,) + self._shape() + (self.nstates,))


class LDR2(_LDR):
    """Drop-in for pyqed.ldr.ldr.LDR2 (ldr.py:1111-1776): N-state two-mode conical-intersection dynamics, sine DVR,
    split operator in the local diabatic representation."""

    def __init__(self, x, y, nstates=2, ndim=2, mass=None, dvr='sine'):
        if ndim != 2:
            raise NotImplementedError(f"LDR2 is two-dimensional (ndim={ndim}); LDRN covers ndim 1 to {MAX_DIM}")
        if dvr != 'sine':
            raise NotImplementedError(f"LDR2 with dvr={dvr!r}: the reference's buildK uses the sine DVR whatever dvr "
                                      "says (ldr.py:1264-1270); only 'sine' is accepted")
        self.x, self.y = x, y
        self.dx, self.dy = interval(x), interval(y)
        self.nstates = nstates
        self.nx, self.ny = len(x), len(y)
        self.size = self.nx * self.ny * nstates
        self.dvr = dvr
        self.mass = [1, ] * ndim if mass is None else mass
        self.ngrid = [self.nx, self.ny]
        self.nbasis = self.nx * self.ny
        self._init_state()
        self.adiabatic_states = []      # as the reference leaves it until the states are set or built

    def _axes(self):
        return [np.asarray(self.x), np.asarray(self.y)]

    def _dx(self):
        return [self.dx, self.dy]

    @property
    def v(self):
        return self._v

    @v.setter
    def v(self, v):
        assert (v.shape == (self.nx, self.ny, self.nstates, self.nstates))
        self._v = v

    def _dvrs(self):
        # the reference's rule (ldr.py:1264, 1268): the box is [x[0], x[-1]] with nx interior points, whatever the
        # spacing of the user's grid is
        return [sine_dvr(a[0], a[-1], len(a), mass=m) for a, m in zip(self._axes(), self.mass)]

    def run(self, psi0, dt, nt, nout=1, t0=0):
        """ldr.py:1564-1611: psilist holds psi0 and nt // nout snapshots."""
        r = ResultSPO2(dt=dt, psi0=psi0, Nt=nt, t0=t0, nout=nout)
        r.x, r.y = self.x, self.y
        r.psilist = self._run_states(psi0, dt, nt, nout)
        return r

    def fast_run(self, *a, **k):
        raise NotImplementedError("LDR2.fast_run squares the dense short-time propagator (ldr.py:1613-1635): a "
                                  "(nx ny ns)^2 method with no matrix-free form; use run()")

    def fast_LvN(self, *a, **k):
        raise NotImplementedError("LDR2.fast_LvN appends to results['rho'], a key it never creates (ldr.py:1679)")

    def buildH(self, *a, **k):
        raise NotImplementedError("LDR2.buildH reads self.build, an attribute that does not exist (ldr.py:1532)")

    def HEOM(self, *a, **k):
        raise NotImplementedError("LDR2.HEOM is a stub in the reference (ldr.py:1770-1776)")


class LDRN(_LDR):
    """Drop-in for pyqed.ldr.ldr.LDRN (ldr.py:320-675) in one to three dimensions on sine-DVR grids of 2^l - 1 points.
    The reference takes the dense overlap A as input; this class takes the states it is the Gram matrix of,
    adiabatic_states [*nx, M, nstates], or builds them from v (build_apes)."""

    def __init__(self, domains, levels, ndim=3, nstates=2, x0=None, mass=None, dvr_type='sine'):
        assert (len(domains) == len(levels) == ndim)
        if ndim > MAX_DIM:
            raise NotImplementedError(f"LDRN with ndim={ndim}: qd_ldr_run covers ndim 1 to {MAX_DIM}")
        if dvr_type != 'sine':
            raise NotImplementedError(f"LDRN with dvr_type={dvr_type!r}: only 'sine' is covered (the reference's "
                                      "'gauss_hermite' branch calls HermiteDVR.copy, which does not exist, "
                                      "ldr.py:371)")
        self.domains = domains
        self.mass = [1, ] * ndim if mass is None else mass
        self.L = [d[1] - d[0] for d in domains]
        self.dvr = [sine_dvr(*domains[d], 2 ** levels[d] - 1, self.mass[d]) for d in range(ndim)]
        self.x = [d.x for d in self.dvr]
        self.w = []
        self.dx = [interval(x) for x in self.x]
        self.nx = [len(x) for x in self.x]
        self.dvr_type = [dvr_type, ] * ndim
        self.nstates = nstates
        self.ndim = ndim
        self.ntot = int(np.prod(self.nx))
        self._init_state()

    def _axes(self):
        return [np.asarray(x) for x in self.x]

    def _dx(self):
        return self.dx

    @property
    def v(self):
        return self._v

    @v.setter
    def v(self, v):
        assert (v.shape == (*self.nx, self.nstates, self.nstates))
        if abs(np.min(v)) > 0.1:
            raise ValueError('The PES minimum is not 0. Shift the PES.')
        self._v = v

    def _dvrs(self):
        return [sine_dvr(*self.domains[d], self.nx[d], mass=self.mass[d]) for d in range(self.ndim)]

    def run(self, psi0, dt, nt, nout=1, t0=0):
        """ldr.py:579-625"""
        r = ResultLDR(dx=self.dx, dt=dt, psi0=psi0, Nt=nt, t0=t0, nout=nout)
        r.psilist = self._run_states(psi0, dt, nt, nout)
        return r

    def rdm_nuc(self, psi):
        """rho[i.., k..] = sum_a conj(psi[i.., a]) psi[k.., a] on the host (ldr.py:652-675); D <= DENSE_MAX_D."""
        self._dense_check("rdm_nuc")
        sh = tuple(self.nx)
        f = np.asarray(psi).reshape(-1, self.nstates)
        return np.einsum('pa,qa->pq', f.conj(), f).reshape(sh + sh)


JACOBI_ROWS_MAX = 1 << 24   # nx * ny^2 up to which LDR2_Jacobi.buildK forms the per-row propagators (256 MiB)


class LDR2_Jacobi(_LDR):
    """Drop-in for pyqed.ldr.ldr.LDR2_Jacobi (ldr.py:1779-1987): a stretch x = r and an angle y = theta with
    T = p_r^2 / 2 mx + p_theta^2 / 2 I(r), mass = [mx, I] with I a callable of x.

    The reference's angular propagator is one [ny, ny] matrix per row of the grid, expTy[i] = SineDVR(theta-domain, ny,
    mass=I(x_i)).expT(dt), multiplied into the dense exp_T.  Every row's matrix has the sine-transform matrix S as its
    eigenvectors, expTy[i] = S diag(exp(-i E_m dt / I(x_i))) S with E_m the unit-mass box levels, so run() forms S, the
    [nx, ny] phase table and expTx only and propagates through qd_ldr_jacobi_run (ldr_jacobi_run).

    Kept from the reference: buildK takes the constructor's dt for both kinetic factors whatever dt run() is given
    (buildV takes run's); where the constructor's dt is None the reference raises inside expT, and run's dt is used
    here."""

    def __init__(self, domains, levels, dvr_types, mass=None, ndim=2, nstates=2, dt=None, nt=None, nout=1):
        assert (len(domains) == len(levels) == ndim)
        if ndim != 2:
            raise NotImplementedError(f"LDR2_Jacobi is two-dimensional (ndim={ndim}): the reference unpacks "
                                      "self.x, self.y = x (ldr.py:1830)")
        for t in dvr_types:
            if t in ('sinc', 'sine'):
                continue
            if t == 'gauss_hermite':
                raise NotImplementedError("LDR2_Jacobi with dvr_types 'gauss_hermite': the reference's branch rebinds "
                                          "its own loop variable d (ldr.py:1816)")
            if t == 'fourier':
                raise NotImplementedError("LDR2_Jacobi with dvr_types 'fourier': the reference's branch is `pass` "
                                          "(ldr.py:1824)")
            raise ValueError('DVR {} is not supported. Please use sinc.'.format(t))
        self.domains = domains
        self.nstates = nstates
        self.L = [d[1] - d[0] for d in domains]
        self.x0 = [0.5 * (d[1] + d[0]) for d in domains]
        # discretize(a, b, l, endpoints=False): the 2^l - 1 points strictly inside, the sine DVR's grid
        x = [np.linspace(*domains[d], 2 ** levels[d], endpoint=False)[1:] for d in range(ndim)]
        self.x, self.y = x
        self.w = [[1 / (2 ** l - 1), ] * (2 ** l - 1) for l in levels]
        self.dvr = []
        self.nx, self.ny = [len(_x) for _x in x]
        self.dx, self.dy = interval(self.x), interval(self.y)   # the reference leaves them unset, and its rdm_el fails
        self.dvr_types = dvr_types
        self.mass = [1, ] * ndim if mass is None else mass
        self.ndim = ndim
        self.npts = self.nx * self.ny
        self._init_state()
        self.wf_overlap = None
        self.dt, self.nt, self.nout = dt, nt, nout
        self._F = self._ph = None

    def _axes(self):
        return [np.asarray(self.x), np.asarray(self.y)]

    def _dx(self):
        return [self.dx, self.dy]

    @property
    def v(self):
        return self._v

    @v.setter
    def v(self, v):
        assert (v.shape == (self.nx, self.ny, self.nstates, self.nstates))
        self._v = v

    def metric(self, q):
        """g = diag(1 / mx, 1 / I(r)) at q = (r, theta).  The reference's np.diag(1 / self.mass) divides by a list
        (ldr.py:1867)."""
        mx, inertia = self.mass
        return np.diag([1.0 / mx, 1.0 / (inertia(q[0]) if callable(inertia) else inertia)])

    def _inertia(self):
        mx, inertia = self.mass
        if not callable(inertia):
            raise TypeError("LDR2_Jacobi: mass must be [mx, I] with I a callable of x (the moment of inertia)")
        I = np.asarray(inertia(self.x), dtype=float)
        if I.shape != (self.nx,):
            raise ValueError(f"LDR2_Jacobi: I(x) must have shape {(self.nx,)}; got {I.shape}")
        return mx, I

    def _kinetic_dt(self, dt):
        return dt if self.dt is None else self.dt

    def _factors(self, dt):
        """expTx, S and the phase table ph[i, m] = exp(-i E_m dt / I(x_i)), with the reference's expression for the
        exponent (dvr_1d.py:705)."""
        mx, I = self._inertia()
        dvr_x = sine_dvr(*self.domains[0], self.nx, mass=mx)
        dvr_y = sine_dvr(*self.domains[1], self.ny)
        ph = np.exp(-1j * dt / (2 * I[:, None]) * dvr_y.n[None, :] ** 2 * np.pi ** 2 / dvr_y.L ** 2)
        return dvr_x, dvr_x.expT(dt), dvr_y.fbr2dvr(), ph

    def buildK(self, dt):
        """The reference's [expTx, expTy[nx, ny, ny]] (ldr.py:1870-1936) while nx ny^2 <= 2^24; run() does not call
        it."""
        if self.nx * self.ny ** 2 > JACOBI_ROWS_MAX:
            raise ValueError(f"LDR2_Jacobi.buildK: nx * ny^2 = {self.nx * self.ny ** 2} exceeds {JACOBI_ROWS_MAX}; "
                             f"the [{self.nx}, {self.ny}, {self.ny}] array of per-row propagators is not formed "
                             "(run() does not need it)")
        dvr_x, expTx, S, ph = self._factors(self._kinetic_dt(dt))
        self.K = [dvr_x.t()]
        self.exp_K = [expTx, np.einsum('am,im,mb->iab', S, ph, S)]
        return self.exp_K

    def _build_kinetic(self, dt):
        _, expTx, self._F, self._ph = self._factors(self._kinetic_dt(dt))
        self._expTx = expTx

    def _launch(self, psi, U, dt, nt, nout, **kw):
        return ldr_jacobi_run(psi, U, None, self._F, self._F, self._ph, [self._expTx], dt, nt, nout, **kw)

    def run(self, psi0, dt, nt, nout=1, t0=0):
        """ldr.py:1938-1987: psilist holds psi0 and nt // nout snapshots."""
        r = ResultSPO2(dt=dt, psi0=psi0, Nt=nt, t0=t0, nout=nout)
        r.x, r.y = self.x, self.y
        r.psilist = self._run_states(psi0, dt, nt, nout)
        return r
