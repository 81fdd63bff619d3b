"""The class surface of LDR2_Jacobi on the GPU against tests/golden/ldr_jacobi.npz (the real reference's
LDR2_Jacobi.run and rdm_el): the states are the fixture's and are handed to the class, because the gauge of eigh is not
portable.  Bound: 1e-10 relative, the project's standing bound for fp64 GPU paths against reference data.
"""
import numpy as np
import pytest

from conftest import load_golden, relerr, took

pytestmark = pytest.mark.gpu

TOL = 1e-10
MASS_X = 1.3


def inertia(r):
    return 2.0 * r ** 2


@pytest.fixture(scope="module")
def g():
    return load_golden("ldr_jacobi")


def solver_of(g, tag):
    from pyqed_amd import LDR2_Jacobi
    sol = LDR2_Jacobi([tuple(d) for d in g["domains"]], (4, 3) if tag == "b" else (3, 3), ['sine', 'sine'],
                      mass=[MASS_X, inertia], nstates=2, dt=float(g[f"{tag}_dt_ctor"]))
    sol.apes = g[f"{tag}_apes"]
    sol.adiabatic_states = g[f"{tag}_U"]
    return sol


@pytest.mark.parametrize("tag", ["a", "b", "q"])
def test_run_against_the_reference(g, tag):
    """Case q runs with the constructor's dt 0.03 in the kinetic factor and run's 0.05 in the potential one."""
    sol = solver_of(g, tag)
    psi0 = g[f"{tag}_psi0"]
    took("ldr")
    r = sol.run(psi0, float(g["dt"]), int(g["nt"]), nout=int(g["nout"]))
    assert took("ldr_jacobi_fused")[0]
    ref = g[f"{tag}_states"]
    assert len(r.psilist) == int(g["nt"]) // int(g["nout"]) + 1 == len(ref) and r.psilist[0] is psi0
    assert len(r.times) == len(r.psilist) and r.x is sol.x and r.y is sol.y
    err = relerr(np.array(r.psilist[1:]), ref[1:])
    print(f"LDR2_Jacobi case {tag}: {err:.2e}")
    assert err < TOL
    rdm = sol.rdm_el(r.psilist[-1])
    assert relerr(rdm, g[f"{tag}_rdm"]) < TOL
    rl = sol.rdm_el(r.psilist)
    assert isinstance(rl, list) and len(rl) == len(r.psilist) and np.array_equal(rl[-1], rdm)
    # run() formed nothing of the reference's per-row or dense size
    assert sol.exp_K is None and sol.exp_T is None and sol.A is None


def test_build_path_in_gauge_free_quantities(g):
    """Case a with sol.v = v and nothing else: the class's eigh fixes its own signs, so psi0 is carried over through
    chi = U psi and the run is compared in chi."""
    from pyqed_amd import LDR2_Jacobi
    sol = LDR2_Jacobi([tuple(d) for d in g["domains"]], (3, 3), ['sine', 'sine'], mass=[MASS_X, inertia], dt=0.05)
    sol.v = g["a_v"]
    sol.build_apes()
    sign = np.einsum('...ma,...ma->...a', sol.adiabatic_states.conj(), g["a_U"])
    assert np.abs(np.abs(sign) - 1).max() < 1e-12
    sol = LDR2_Jacobi([tuple(d) for d in g["domains"]], (3, 3), ['sine', 'sine'], mass=[MASS_X, inertia], dt=0.05)
    sol.v = g["a_v"]
    r = sol.run(g["a_psi0"] * sign, float(g["dt"]), int(g["nt"]), nout=int(g["nout"]))
    chi = np.einsum('...ma,z...a->z...m', sol.adiabatic_states, np.array(r.psilist[1:]))
    chi_ref = np.einsum('...ma,z...a->z...m', g["a_U"], g["a_states"][1:])
    assert relerr(chi, chi_ref) < TOL


def test_run_batch_members_against_single_runs(g):
    """A member's columns see the same products in the same order whatever the batch is: bit for bit, as
    test_ldr_gpu holds it for LDR2."""
    import torch
    sol = solver_of(g, "b")
    rng = np.random.default_rng(8)
    psis = np.stack([g["b_psi0"], g["b_psi0"][::-1].copy(), rng.standard_normal((15, 7, 2)) + 0j])
    dt, nt, nout = float(g["dt"]), int(g["nt"]), int(g["nout"])
    snap = sol.run_batch(psis, dt, nt, nout)
    assert isinstance(snap, torch.Tensor) and tuple(snap.shape) == (3, nt // nout, 15, 7, 2)
    snap = snap.cpu().numpy()
    assert relerr(snap[0], g["b_states"][1:]) < TOL
    for b in range(3):
        r = sol.run(psis[b], dt, nt, nout=nout)
        assert np.array_equal(np.array(r.psilist[1:]), snap[b]), b


def test_observed_run_against_rdm_el_of_the_states(g):
    sol = solver_of(g, "b")
    psis = np.stack([g["b_psi0"], g["b_psi0"][:, ::-1].copy()])
    dt, nt = float(g["dt"]), int(g["nt"])
    pop, rdm = sol.run_batch(psis, dt, nt, 1, return_states=False)
    assert pop.is_cuda and rdm.is_cuda and tuple(pop.shape) == (2, nt, 2) and tuple(rdm.shape) == (2, nt, 2, 2)
    snap = sol.run_batch(psis, dt, nt, 1).cpu().numpy()
    for b in range(2):
        post = np.array(sol.rdm_el(list(snap[b])))
        assert np.array_equal(rdm[b].cpu().numpy(), post), b
        assert np.array_equal(pop[b].cpu().numpy(), np.real(np.einsum('kaa->ka', post))), b
    # truncated states: the populations decay, as the reference's do
    assert float(pop[0, -1].sum()) < float(pop[0, 0].sum())


def test_short_time_propagator_against_the_reference_formula(g):
    """Case a, D = 98: exp_V_half exp_T exp_V_half with exp_T = einsum('ijaklb,ik,kjl->ijaklb', A, expKx, expKy) formed
    in numpy from the fixture's arrays (ldr.py:1961)."""
    sol = solver_of(g, "a")
    dt = float(g["dt"])
    stp = sol.short_time_propagator(dt)
    assert stp.shape == (7, 7, 2, 7, 7, 2)
    U = g["a_U"]
    A = np.einsum('ijma,klmb->ijaklb', U.conj(), U)
    exp_T = np.einsum('ijaklb,ik,kjl->ijaklb', A, g["a_expKx"], g["a_expKy"])
    eh = np.exp(-0.5j * dt * g["a_apes"])
    ref = eh[..., None, None, None] * exp_T * eh[None, None, None]
    err = relerr(stp, ref)
    print(f"short_time_propagator 7x7: {err:.2e}")
    assert err < TOL
