"""The class surface of the local-diabatic-representation solvers on the GPU against tests/golden/ldr.npz (the real
reference's LDR2.run, LDRN.run, rdm_el, get_population and short_time_propagator): the states are the fixture's and
are handed to the classes, because the gauge of eigh is not portable; the build path (case d) is compared in
gauge-free quantities.  Bound: 1e-10 relative, the project's standing bound for fp64 GPU paths against reference data.
"""
import numpy as np
import pytest

from conftest import load_golden, relerr, took

pytestmark = pytest.mark.gpu

TOL = 1e-10


@pytest.fixture(scope="module")
def g():
    return load_golden("ldr")


def ldr2_of(g, tag, mass=(1.0, 1.7), states=True):
    from pyqed_amd import LDR2
    sol = LDR2(g[f"{tag}_x"], g[f"{tag}_y"], nstates=2, mass=list(mass))
    if states:
        sol.apes = g[f"{tag}_apes"]
        sol.adiabatic_states = g[f"{tag}_U"]
    return sol


def ldrn_of(g, tag, ndim):
    from pyqed_amd import LDRN
    sol = LDRN([tuple(d) for d in g[f"{tag}_domains"]], tuple(int(l) for l in g[f"{tag}_levels"]), ndim=ndim,
               nstates=2, mass=list(g[f"{tag}_mass"]))
    sol.apes = g[f"{tag}_apes"]
    sol.adiabatic_states = g[f"{tag}_U"]
    return sol


@pytest.mark.parametrize("tag", ["a", "b", "c"])
def test_ldr2_run_against_the_reference(g, tag):
    sol = ldr2_of(g, tag)
    psi0 = g[f"{tag}_psi0"]
    took("ldr")
    r = sol.run(psi0, float(g["dt"]), int(g["nt"]), nout=int(g["nout"]))
    assert took("ldr_axes_fused")[0]
    ref = g[f"{tag}_states"]
    assert len(r.psilist) == int(g["nt"]) // int(g["nout"]) + 1 == len(ref) and r.psilist[0] is psi0
    assert len(r.times) == len(r.psilist) and r.x is sol.x and r.y is sol.y
    err = relerr(np.array(r.psilist[1:]), ref[1:])
    print(f"LDR2 case {tag}: {err:.2e}")
    assert err < TOL
    # rdm_el of an array and of a list, on the device
    rdm = sol.rdm_el(r.psilist[-1])
    assert relerr(rdm, g[f"{tag}_rdm"]) < TOL
    rl = sol.rdm_el(r.psilist)
    assert isinstance(rl, list) and len(rl) == len(r.psilist) and np.array_equal(rl[-1], rdm)
    pop = r.get_population()
    assert np.abs(pop[-1] - np.real(np.diag(g[f"{tag}_rdm"]))).max() < TOL


def test_ldr2_build_path_in_gauge_free_quantities(g):
    """Case d: sol.v = v and nothing else.  The class's eigh fixes its own signs, so psi0 (given in the reference's
    gauge) is carried over through chi = U psi, and the run is compared in chi and in the populations."""
    sol = ldr2_of(g, "d", mass=(1, 1), states=False)
    sol.v = g["d_v"]
    sol.build_apes()
    U, Uref = sol.adiabatic_states, g["d_U"]
    sign = np.einsum('...ma,...ma->...a', U.conj(), Uref)
    assert relerr(sol.apes, g["d_apes"]) < 1e-13 and np.abs(np.abs(sign) - 1).max() < 1e-12
    # a fresh solver that builds everything itself inside run()
    sol = ldr2_of(g, "d", mass=(1, 1), states=False)
    sol.v = g["d_v"]
    r = sol.run(g["d_psi0"] * sign, float(g["dt"]), int(g["nt"]), nout=int(g["nout"]))
    got, ref = np.array(r.psilist[1:]), g["d_states"][1:]
    chi = np.einsum('...ma,z...a->z...m', sol.adiabatic_states, got)
    chi_ref = np.einsum('...ma,z...a->z...m', Uref, ref)
    assert relerr(chi, chi_ref) < TOL
    assert np.abs(np.abs(got) ** 2 - np.abs(ref) ** 2).max() < TOL
    assert relerr(sol.rdm_el(got[-1]).diagonal(), g["d_rdm"].diagonal()) < TOL


def test_ldrn_run_against_the_reference(g):
    sol = ldrn_of(g, "n", 3)
    psi0 = g["n_psi0"]
    r = sol.run(psi0, float(g["dt"]), int(g["nt"]), nout=int(g["nout"]))
    ref = g["n_states"]
    assert len(r.psilist) == len(ref) and r.psilist[0] is psi0 and list(r.dx) == list(sol.dx)
    err = relerr(np.array(r.psilist[1:]), ref[1:])
    print(f"LDRN 7x3x3: {err:.2e}")
    assert err < TOL
    assert relerr(sol.rdm_el(r.psilist[-1]), g["n_rdm"]) < TOL
    # two dimensions, with the reference's get_population
    sol = ldrn_of(g, "m", 2)
    r = sol.run(g["m_psi0"], float(g["dt"]), int(g["nt"]), nout=int(g["nout"]))
    assert relerr(np.array(r.psilist[1:]), g["m_states"][1:]) < TOL
    p = r.get_population(plot=False)
    assert p.shape == g["m_pop"].shape and np.abs(p - g["m_pop"]).max() < TOL
    # one dimension: no reference run (its get_population and A are two- and more-dimensional); against the
    # factorised restatement
    from ldr_models import ldr_factorised, random_case
    from pyqed_amd import LDRN
    c = random_case(4, (15,), 3, 2, 1)
    s1 = LDRN([(-2.0, 2.0)], [4], ndim=1, nstates=2, mass=[1.3])
    s1.apes, s1.adiabatic_states = c["apes"], c["U"]
    r = s1.run(c["psi"][0], 0.05, 3)
    s1.buildV(0.05)
    want = ldr_factorised(c["psi"], c["U"], s1.exp_V, s1.exp_V_half, s1.exp_K, 3, 1)[0]
    assert relerr(np.array(r.psilist[1:]), want) < TOL


def test_short_time_propagator_against_the_reference(g):
    sol = ldr2_of(g, "s", mass=(0.8, 1.1))
    stp = sol.short_time_propagator(float(g["dt"]))
    assert stp.shape == g["s_stp"].shape == (6, 5, 2, 6, 5, 2)
    err = relerr(stp, g["s_stp"])
    print(f"short_time_propagator 6x5: {err:.2e}")
    assert err < TOL
    sol = ldr2_of(g, "a")
    stp = sol.short_time_propagator(float(g["dt"])).reshape(15, 11, 2, -1)
    assert relerr(stp[..., g["a_stp_cols"]], g["a_stp"]) < TOL
    # the propagator takes psi0 to the state half a potential step short of the first snapshot's expV
    psi0 = g["a_psi0"]
    one = sol.run(psi0, float(g["dt"]), 1).psilist[1]
    via = (stp.reshape(330, 330) @ psi0.reshape(-1)).reshape(15, 11, 2) * sol.exp_V_half
    assert relerr(via, one) < TOL


def test_run_batch_members_equal_run_bit_for_bit(g):
    import torch
    sol = ldr2_of(g, "b")
    rng = np.random.default_rng(8)
    psis = np.stack([g["b_psi0"], g["c_psi0"], rng.standard_normal((17, 13, 2)) + 0j])
    dt, nt, nout = float(g["dt"]), int(g["nt"]), int(g["nout"])
    snap = sol.run_batch(psis, dt, nt, nout)
    assert isinstance(snap, torch.Tensor) and tuple(snap.shape) == (3, nt // nout, 17, 13, 2)
    snap = snap.cpu().numpy()
    for b in range(3):
        r = sol.run(psis[b], dt, nt, nout=nout)
        assert np.array_equal(np.array(r.psilist[1:]), snap[b]), b


def test_observed_run_keeps_no_states_and_equals_post_hoc_bit_for_bit(g):
    import torch
    sol = ldr2_of(g, "b")
    psis = np.stack([g["b_psi0"], g["c_psi0"]])
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


def test_63x63_runs_and_keeps_the_norm():
    """D = 7938: the reference needs 1 GB of exp_T here, so nothing is compared to it.  M = ns = 2: the step is
    unitary, and the norm holds to 1e-12 per step."""
    from pyqed_amd import LDR2
    x = y = np.linspace(-4, 4, 63)
    X, Y = np.meshgrid(x, y, indexing="ij")
    v = np.zeros((63, 63, 2, 2))
    v[..., 0, 0] = 0.5 * ((X + 1) ** 2 + Y ** 2)
    v[..., 1, 1] = 0.5 * ((X - 1) ** 2 + Y ** 2)
    v[..., 0, 1] = v[..., 1, 0] = 0.4 * Y
    sol = LDR2(x, y, nstates=2)
    sol.v = v
    psi0 = np.zeros((63, 63, 2), dtype=complex)
    psi0[..., 1] = np.exp(-((X - 0.5) ** 2 + Y ** 2))
    psi0 /= np.linalg.norm(psi0)
    nt = 6
    took("ldr")
    r = sol.run(psi0, 0.02, nt, nout=2)
    assert took("ldr_axes_fused")[0] and len(r.psilist) == 4
    norms = np.array([np.linalg.norm(p) for p in r.psilist])
    print("63x63 norms - 1:", norms - 1)
    assert np.abs(norms - 1).max() < 1e-12 * nt
    assert np.linalg.norm(r.psilist[-1] - psi0) > 1e-2          # it moved
    with pytest.raises(ValueError, match="exceeds 4096"):
        sol.short_time_propagator(0.02)
