"""LVC(...).wavepacket_dynamics().run(...) on the GPU (pyqed_amd.mol: LVC, LVCOp, LVCSolver over qd_lvc_rk4): against
the reference's own run (tests/golden/lvc.npz), norm and trace conservation of a Hermitian model, and the contracts of
store_states, run_batch and host-evaluated observables."""
import numpy as np
import pytest

import lvc_models as lm
from conftest import load_golden
from test_lvc_host import _model

pytestmark = pytest.mark.gpu


def _pyrazine_like(trunc=(6, 5, 4)):
    from pyqed_amd import LVC, Mode
    modes = [Mode(0.074, [[[1, 1], -0.05], [[2, 2], 0.06]], truncate=trunc[0]),
             Mode(0.126, [[[1, 1], 0.03], [[2, 2], 0.04]], truncate=trunc[1]),
             Mode(0.118, [[[1, 2], 0.08]], truncate=trunc[2])]
    mol = LVC([0.0, 0.5, 0.62], modes)
    mol.add_coupling([[0, 1], 0.01])
    return mol


@pytest.mark.parametrize("path", ["auto", "staged"])
@pytest.mark.parametrize("tag", ["a", "b"])
def test_run_against_reference_fixture(tag, path):
    """The reference's LVC run with Nt = 10, nout = 3 and e_ops [buildop(1), coordinate(0)]: 3 states, observables
    (3, 2).  The other reference-fixture comparisons of RK4 runs hold 1e-10; this one holds 1e-13 (seen on an MI355X:
    states 2.8e-17, observables 1.1e-16)."""
    g = load_golden("lvc")
    mol, extra = _model(g, tag)
    mol.add_coupling(extra)
    sol = mol.wavepacket_dynamics()
    res = sol.run(psi0=mol.vertical(1), dt=float(g["dt"]), Nt=int(g["Nt"]), nout=int(g["nout"]),
                  e_ops=[mol.buildop(1), mol.coordinate(0)], path=path)
    states = np.array(res.psilist)
    err_s = np.abs(states - g[tag + "_states"]).max()
    err_o = np.abs(res.observables - g[tag + "_obs"]).max()
    print(f"lvc fixture {tag} {path}: states {err_s:.2e}, observables {err_o:.2e}")
    assert states.shape == g[tag + "_states"].shape and res.observables.shape == (3, 2)
    assert err_s < 1e-13 and err_o < 1e-13
    assert res.rdm_el.shape == (3, 3, 3) and res.x.shape == res.nbar.shape == (3, mol.nmodes)
    assert np.abs(res.rdm_el[-1] - mol.rdm_el(states[-1])).max() < 1e-13
    assert mol.H is None    # the run needed no H


@pytest.mark.parametrize("trunc,path", [((6, 5, 4), "resident"), ((6, 5, 4), "staged"), ((12, 11, 12), "staged")])
def test_hermitian_model_keeps_norm_and_trace(trunc, path):
    """200 steps of a Hermitian model from the vertical state: the norm stays 1 to 1e-12 and result.rdm_el has unit
    trace at every record.  RK4 itself loses (dt |E|)^6 / 72 of an eigencomponent's norm per step, so dt is set from the
    model's bound of ||H||_1 to dt |E| <= 0.005: at most 200 * 2.2e-16 = 4.3e-14 over the run, the rest of the 1e-12
    is for the rounding of 800 stages."""
    mol = _pyrazine_like(trunc)
    dt = 0.005 / lm.h_bound(mol.fock_dims, mol.omegas, mol.Hel(), mol.Wmats())
    res = mol.wavepacket_dynamics().run(psi0=mol.vertical(1), dt=dt, Nt=205, nout=5, e_ops=[mol.buildop(2)],
                                        path=path)
    assert len(res.psilist) == 41 and res.rdm_el.shape == (41, 3, 3)
    norms = np.array([np.linalg.norm(s) for s in res.psilist])
    tr = np.einsum("kaa->k", res.rdm_el)
    print(f"lvc hermitian {trunc} {path}: |norm - 1| {np.abs(norms - 1).max():.2e}, |tr - 1| {np.abs(tr - 1).max():.2e}")
    assert np.abs(norms - 1).max() < 1e-12 and np.abs(tr - 1).max() < 1e-12
    assert np.abs(res.rdm_el - np.conj(np.swapaxes(res.rdm_el, 1, 2))).max() < 1e-14
    assert np.abs(res.observables[:, 0] - res.rdm_el[:, 2, 2]).max() < 1e-15
    assert np.abs(np.linalg.norm(res.psi) - 1) < 1e-12 and np.array_equal(res.psi, res.psilist[-1])


@pytest.mark.parametrize("path", ["resident", "staged"])
def test_store_states_false_gives_the_same_observables(path):
    mol = _pyrazine_like()
    ops = [mol.buildop(1), mol.buildop(1, 2), mol.coordinate(2), mol.promote(np.diag([0.0, 1.0, 2.0]), "el")]
    sol = mol.wavepacket_dynamics()
    kw = dict(psi0=mol.vertical(2), dt=0.02, Nt=23, nout=4, e_ops=ops, path=path)
    a = sol.run(store_states=True, **kw)
    b = sol.run(store_states=False, **kw)
    assert a.observables.shape == (5, 4) and len(a.psilist) == 5 and b.psilist == []
    assert np.array_equal(a.observables, b.observables) and np.array_equal(a.rdm_el, b.rdm_el)
    assert np.array_equal(a.x, b.x) and np.array_equal(a.nbar, b.nbar) and np.array_equal(a.psi, b.psi)
    with pytest.raises(TypeError, match="is no LVCOp"):
        sol.run(store_states=False, **dict(kw, e_ops=[mol.buildop(1).tocsr()]))


@pytest.mark.parametrize("path", ["resident", "staged"])
def test_run_batch_member_equals_single_run(path):
    mol = _pyrazine_like()
    rng = np.random.default_rng(3)
    psi0s = rng.standard_normal((3, mol.dim)) + 1j * rng.standard_normal((3, mol.dim))
    psi0s /= np.linalg.norm(psi0s, axis=1, keepdims=True)
    sol = mol.wavepacket_dynamics()
    ops = [mol.buildop(0, 1), mol.coordinate(0)]
    kw = dict(dt=0.02, Nt=13, nout=3, e_ops=ops, path=path)
    batch = sol.run_batch(psi0s, **kw)
    assert len(batch) == 3
    for b in range(3):
        one = sol.run(psi0=psi0s[b], **kw)
        assert np.array_equal(np.array(one.psilist), np.array(batch[b].psilist))
        assert np.array_equal(one.observables, batch[b].observables) and np.array_equal(one.rdm_el, batch[b].rdm_el)
        assert np.array_equal(one.nbar, batch[b].nbar) and np.array_equal(one.psi, batch[b].psi)


def test_host_evaluated_operator_equals_the_lvcop():
    """A scipy sparse (or dense) e_op is applied on the host to the stored states; the same operator as an LVCOp comes
    from the on-device record.  Both to 1e-13."""
    mol = _pyrazine_like()
    sol = mol.wavepacket_dynamics()
    lops = [mol.buildop(1, 2), mol.coordinate(1), mol.buildop(0, 1) @ mol.coordinate(2)]
    hops = [lops[0].tocsr(), lops[1].toarray(), lops[2].tocsr()]
    kw = dict(psi0=mol.vertical(1), dt=0.02, Nt=21, nout=4)
    a = sol.run(e_ops=lops, **kw)
    b = sol.run(e_ops=hops, **kw)
    assert a.observables.shape == b.observables.shape == (5, 3)
    assert np.abs(a.observables - b.observables).max() < 1e-13
    assert np.abs(a.observables[:, 1] - a.x[:, 1]).max() < 1e-15
    assert np.abs(a.observables[1:]).max() > 1e-4   # not a comparison of zeros


def test_inherited_paths_on_the_lazy_h():
    """self.H is built on first access; the inherited correlation function runs on it and a direct SESolver on the
    same H gives the same numbers."""
    from pyqed_amd.mol import SESolver
    mol = _pyrazine_like((3, 2, 2))
    sol = mol.wavepacket_dynamics()
    assert mol.H is None
    ops = [mol.buildop(0, 1).toarray(), mol.coordinate(0).toarray(), mol.buildop(0, 1).toarray()]
    c = sol.correlation_3op_1t(mol.vertical(0), ops, 0.05, 4)
    assert mol.H is not None and sol.H.shape == (mol.dim, mol.dim)
    ref = SESolver(mol.H).correlation_3op_1t(mol.vertical(0), ops, 0.05, 4)
    assert c.shape == (4,) and np.array_equal(c, ref)
