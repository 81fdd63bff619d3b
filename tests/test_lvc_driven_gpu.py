"""LVCSolver.run / run_batch with a pulse on the matrix-free path (pyqed_amd.mol over qd_lvc_driven_rk4) against the
fall-through it replaces, SESolver.run on model.buildH() with the dipole as a D x D matrix (itself pinned to the
reference by the tdse_driven goldens): states and observables within 1e-10, the project's class-level bound, for an
LVCOp dipole, a list of two pulses and two dipoles, an [nel, nel, 3] dipole in a vector field and a Herzberg-Teller
dipole; run_batch against single runs, store_states=False, nout = 3, stage mode against the restatement of
tests/lvc_drive_models.py, the order of both modes through the class, and the D x D dipole still falling through."""
import numpy as np
import pytest

import lvc_drive_models as dm
import lvc_models as lm
from conftest import took

pytestmark = pytest.mark.gpu
BOUND = 1e-10
KW = dict(dt=0.05, Nt=41, t0=0.5)


class VecPulse:
    """A pulse with a vector field E(t), as SESolver.run's three-dimensional branch takes it."""

    def __init__(self, pulse, pol):
        self.pulse, self.pol = pulse, np.asarray(pol, dtype=float)

    def efield(self, t):
        return self.pulse.efield(t)

    def E(self, t):
        return self.pol * self.pulse.efield(t)


def _model():
    from pyqed_amd import LVC, Mode
    modes = [Mode(0.12, [[[1, 1], 0.06], [[0, 1], 0.02]], truncate=4), Mode(0.2, [[[1, 2], 0.05], [[2, 2], -0.04]],
                                                                            truncate=5)]
    return LVC([0.0, 0.5, 0.62], modes)


def _pulse(tc=1.0, amplitude=0.3, omegac=0.5):
    from pyqed_amd.optics import Pulse
    return Pulse(omegac=omegac, tau=0.6, tc=tc, amplitude=amplitude)


def _dense(states):
    return np.array([np.asarray(s.toarray() if hasattr(s, "toarray") else s).reshape(-1) for s in states])


def _err(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(1.0, np.abs(np.asarray(b)).max()))


def _compare(label, got, ref_psit, ref_obs):
    """got: a matrix-free result; ref_psit [D, nrec] and ref_obs of the fall-through (result.psi, result.observables)."""
    states = _dense(got.psilist)
    es, eo = _err(states, ref_psit.T), _err(got.observables, ref_obs)
    print(f"{label}: states {es:.2e}, observables {eo:.2e}")
    assert states.shape == ref_psit.T.shape and got.observables.shape == ref_obs.shape
    assert es < BOUND and eo < BOUND
    assert np.array_equal(got.psi, states[-1])


@pytest.mark.parametrize("nout", [1, 3])
def test_lvcop_dipole_against_the_fall_through(nout):
    mol = _model()
    sol = mol.wavepacket_dynamics()
    e_ops = [mol.buildop(1), mol.coordinate(0), mol.buildop(0, 2)]
    mu, p = mol.buildop(0, 1), _pulse()
    took("")
    got = sol.run(pulse=p, edip=mu, e_ops=e_ops, nout=nout, **KW)
    assert took("")[1] == ["lvc_driven_resident"]
    ref = sol.run(pulse=p, edip=mu.tocsr(), e_ops=e_ops, nout=nout, **KW)
    noted = took("")[1]
    assert not any(n.startswith("lvc") for n in noted), noted     # a D x D dipole still falls through: no LVC kernel
    _compare(f"LVCOp dipole nout={nout}", got, ref.psi, ref.observables)
    nblk = KW["Nt"] // nout
    assert len(got.psilist) == nblk and got.rdm_el.shape == (nblk, 3, 3) and got.x.shape == got.nbar.shape == (nblk, 2)
    # the block times: block k of nout steps holds f(t0 + k nout dt)
    fv = np.array([[p.efield(KW["t0"] + k * nout * KW["dt"])] for k in range(nblk - 1)], dtype=complex)
    rpsi, rsnap, _ = dm.driven_rk4(mol.groundstate()[None], 3, mol.fock_dims, mol.omegas, mol.Hel(), mol.Wmats(),
                                   mu.A[None], [-1], fv, KW["dt"], (nblk - 1) * nout, nout, "hold", nout)
    assert _err(_dense(got.psilist)[1:], rsnap[0]) < BOUND and _err(got.psi, rpsi[0]) < BOUND
    # an [nel, nel] array means A (x) 1
    arr = sol.run(pulse=p, edip=mu.A, e_ops=e_ops, nout=nout, **KW)
    assert np.array_equal(arr.psi, got.psi) and np.array_equal(arr.observables, got.observables)
    # store_states=False returns the same records and keeps no state
    light = sol.run(pulse=p, edip=mu, e_ops=e_ops, nout=nout, store_states=False, **KW)
    assert light.psilist == [] and np.array_equal(light.observables, got.observables)
    assert np.array_equal(light.psi, got.psi) and np.array_equal(light.rdm_el, got.rdm_el)
    assert np.array_equal(light.x, got.x) and np.array_equal(light.nbar, got.nbar)


@pytest.mark.parametrize("sample", ["hold", "stage"])
def test_a_run_without_steps_returns_the_t0_record(sample):
    """Nt // nout = 1: no block, no field row read (hold mode has none to pass); the record at t0 alone."""
    mol = _model()
    sol = mol.wavepacket_dynamics()
    r = sol.run(psi0=mol.vertical(1), pulse=_pulse(), edip=mol.buildop(0, 1), e_ops=[mol.buildop(1)], dt=0.05, Nt=1,
                sample=sample)
    assert r.observables.shape == (1, 1) and abs(r.observables[0, 0] - 1) < 1e-15
    assert len(r.psilist) == 1 and np.array_equal(r.psi, mol.vertical(1))


def test_two_pulses_and_two_dipoles():
    from pyqed_amd import LVCOp
    mol = _model()
    sol = mol.wavepacket_dynamics()
    e_ops = [mol.buildop(2), mol.coordinate(1)]
    mus = [mol.buildop(0, 1), LVCOp(np.array([[0, 0, 0.7], [0, 0, 0], [0.7, 0, 0.1]]), mol.fock_dims)]
    ps = [_pulse(), _pulse(tc=1.6, amplitude=0.2, omegac=0.62)]
    got = sol.run(pulse=ps, edip=mus, e_ops=e_ops, **KW)
    ref = sol.run(pulse=ps, edip=[m.tocsr() for m in mus], e_ops=e_ops, **KW)
    _compare("two pulses", got, ref.psi, ref.observables)


def test_vector_dipole_in_a_vector_field():
    mol = _model()
    sol = mol.wavepacket_dynamics()
    rng = np.random.default_rng(3)
    ed = rng.standard_normal((3, 3, 3))
    ed = ed + ed.transpose(1, 0, 2)
    p = VecPulse(_pulse(), [0.6, -0.3, 0.74])
    e_ops = [mol.buildop(1)]
    got = sol.run(pulse=p, edip=ed, e_ops=e_ops, **KW)
    full = np.stack([np.kron(ed[:, :, c], np.eye(mol.nvib)) for c in range(3)], axis=2)
    ref = sol.run(pulse=p, edip=full, e_ops=e_ops, **KW)
    _compare("vector dipole", got, ref.psi, ref.observables)


def test_herzberg_teller_dipole():
    from pyqed_amd import LVCOp
    mol = _model()
    sol = mol.wavepacket_dynamics()
    mu = LVCOp(np.array([[0, 1.0, 0.2], [1.0, 0, 0], [0.2, 0, 0]]), mol.fock_dims, mode=1)
    e_ops = [mol.buildop(1), mol.coordinate(1)]
    got = sol.run(pulse=_pulse(), edip=mu, e_ops=e_ops, **KW)
    ref = sol.run(pulse=_pulse(), edip=mu.tocsr(), e_ops=e_ops, **KW)
    _compare("Herzberg-Teller dipole", got, ref.psi, ref.observables)
    # the dipole moved the mode it couples to, by far more than the bound the comparison is made at
    assert np.abs(got.x[:, 1]).max() > 1e4 * BOUND


@pytest.mark.parametrize("sample", ["hold", "stage"])
def test_run_batch_equals_the_single_runs(sample):
    mol = _model()
    sol = mol.wavepacket_dynamics()
    e_ops = [mol.buildop(1), mol.coordinate(0)]
    psi0s = np.stack([mol.vertical(0), mol.vertical(1), (mol.vertical(0) + 1j * mol.vertical(2)) / np.sqrt(2)])
    kw = dict(pulse=_pulse(), edip=mol.buildop(0, 1), e_ops=e_ops, nout=2, sample=sample, **KW)
    batch = sol.run_batch(psi0s, **kw)
    assert len(batch) == 3
    for b in range(3):
        one = sol.run(psi0=psi0s[b], **kw)
        assert np.array_equal(_dense(batch[b].psilist), _dense(one.psilist))
        assert np.array_equal(batch[b].observables, one.observables) and np.array_equal(batch[b].psi, one.psi)


@pytest.mark.parametrize("path", ["staged", "resident"])
def test_stage_mode_against_the_restatement(path):
    from pyqed_amd import LVCOp
    mol = _model()
    sol = mol.wavepacket_dynamics()
    mus = [mol.buildop(0, 1), LVCOp(np.array([[0, 0.3, 0], [0.3, 0, 0], [0, 0, 0]]), mol.fock_dims, mode=0)]
    ps = [_pulse(), _pulse(tc=1.6, amplitude=0.2, omegac=0.62)]
    nout = 2
    took("")
    got = sol.run(pulse=ps, edip=mus, e_ops=[mol.buildop(1)], nout=nout, sample="stage", path=path, **KW)
    assert took("")[1] == [f"lvc_driven_{path}"]
    nsteps = (KW["Nt"] // nout - 1) * nout
    ts = KW["t0"] + 0.5 * KW["dt"] * np.arange(2 * nsteps + 1)
    fv = np.array([[p.efield(t) for p in ps] for t in ts], dtype=complex)
    rpsi, rsnap, robs = dm.driven_rk4(mol.groundstate()[None], 3, mol.fock_dims, mol.omegas, mol.Hel(), mol.Wmats(),
                                      np.array([m.A for m in mus]), [-1, 0], fv, KW["dt"], nsteps, 1, "stage", nout)
    rho, _, _ = lm.split_record(robs[0], 3, 2)
    es, eo = _err(_dense(got.psilist)[1:], rsnap[0]), _err(got.observables[:, 0], rho[:, 1, 1])
    print(f"stage mode {path}: states {es:.2e}, observable {eo:.2e}")
    assert es < BOUND and eo < BOUND and _err(got.psi, rpsi[0]) < BOUND


def test_orders_of_the_two_sampling_modes_through_the_class():
    """The order check of tests/test_lvc_drive_host.py on the resident path: from 100 to 200 steps the stage-mode error
    falls by more than 12, the hold-mode error by between 1.7 and 2.4; the reference is the host restatement in stage
    mode at 6400 steps."""
    from pyqed_amd import LVC, Mode
    from pyqed_amd.optics import Pulse
    o = dm.ORDER
    mol = LVC(list(o["E"]), [Mode(o["omega"][0], [[[0, 1], 0.1], [[1, 1], 0.15]], truncate=o["dims"][0])])
    assert np.array_equal(mol.Wmats(), o["W"])
    sol = mol.wavepacket_dynamics()
    p = Pulse(omegac=o["omegac"], tau=o["tau"], tc=o["tc"], amplitude=o["amplitude"])
    ref = dm.order_run("stage", o["nref"])[0]
    err = {}
    for sample in ("stage", "hold"):
        for n in (100, 200):
            took("")
            r = sol.run(pulse=p, edip=mol.buildop(0, 1), dt=o["T"] / n, Nt=n + 1, sample=sample, path="resident",
                        store_states=False)
            assert took("")[1] == ["lvc_driven_resident"]
            err[sample, n] = float(np.linalg.norm(r.psi - ref))
    r_stage, r_hold = err["stage", 100] / err["stage", 200], err["hold", 100] / err["hold", 200]
    print(f"stage {err['stage', 100]:.2e} -> {err['stage', 200]:.2e} ratio {r_stage:.2f}; "
          f"hold {err['hold', 100]:.2e} -> {err['hold', 200]:.2e} ratio {r_hold:.2f}")
    assert r_stage > 12 and 1.7 < r_hold < 2.4
