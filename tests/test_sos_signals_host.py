"""Sum-over-states signals, host side (no GPU): the NumPy restatement tests/sos_models.py against every entry of the
reference fixture tests/golden/sos_signals.npz, every refusal of pyqed_amd.sos / Mol (raised before any device call) and
the argument checks of the three C entries."""
import numpy as np
import pytest

import sos_models as sm
from conftest import load_golden, relerr

TOL = 1e-12


@pytest.fixture(scope="module")
def fx():
    return load_golden("sos_signals")


def _m(fx, tag):
    return {k: fx[f"{tag}_{k}"] for k in ("E", "dip", "gamma", "g", "e", "f")}


def model_outputs(fx, tag):
    """name -> the restatement's value for every reference output of model `tag` in the fixture."""
    m = _m(fx, tag)
    E, dip, gamma, g, e, f = (m[k] for k in ("E", "dip", "gamma", "g", "e", "f"))
    v = lambda k: fx[f"{tag}_{k}"]
    N = len(E)
    out = {}
    out["GSB"] = sm.GSB(E, dip, v("w1s"), v("w3s"), float(v("tau2")), g, e, gamma)
    out["SE"] = sm.SE(E, dip, v("w1s"), v("w3s"), float(v("tau2")), g, e, gamma)
    out["ESA"] = sm.ESA(E, dip, v("w1s"), v("w3s"), float(v("tau2")), g, e, f, gamma)
    t3, deph = float(v("t3")), float(v("deph"))
    out["SE_t3"] = sm.SE_t3(E, dip, v("w1"), v("w2"), t3, g, e, gamma, deph)
    out["ESA_t3"] = sm.ESA_t3(E, dip, v("w1"), v("w2"), t3, g, e, f, gamma, deph)
    out["SE_t3_default"] = sm.SE_t3(E, dip, v("w1"), v("w2"), t3, g, e, gamma, 10 / sm.au2mev)
    pd = float(v("pe_deph"))
    se, esa = sm.photon_echo_t3(E, dip, v("pe_w1"), v("w2"), t3, [0], range(1, N), range(1, N), gamma, pd)
    out.update(PE2=se + esa, PE2_se=se, PE2_esa=esa)
    out["PE2_se_lists"], out["PE2_esa_lists"] = sm.photon_echo_t3(E, dip, v("pe_w1"), v("w2"), t3, g, e, f, gamma, pd)
    kw = dict(g_idx=g, e_idx=e, f_idx=f, gamma=gamma)
    tau = float(v("dq_tau"))
    out["DQC_R1_t3"] = sm.DQC_R1(E, dip, omega1=v("dq_w1"), omega2=v("dq_w2"), tau3=tau, **kw)
    out["DQC_R1_t1"] = sm.DQC_R1(E, dip, omega2=v("dq_w2"), omega3=v("dq_w3"), tau1=tau, **kw)
    out["DQC_R2_t3"] = sm.DQC_R2(E, dip, omega1=v("dq_w1"), omega2=v("dq_w2"), tau3=tau, **kw)
    out["DQC_R2_t1"] = sm.DQC_R2(E, dip, omega2=v("dq_w2"), omega3=v("dq_w3"), tau1=tau, **kw)
    out["TPA_scalar"] = sm.TPA(E, dip, 2.1, g, e, f, gamma)
    out["TPA_array"] = sm.TPA(E, dip, v("tpa_wp"), g, e, f, gamma)
    out["TPA2D"] = sm.TPA2D(E, dip, v("tpa_wp"), v("tpa_w1"), g, e, f, gamma)
    out["TPA2D_time_order"] = sm.TPA2D_time_order(E, dip, v("tpa_wp"), v("tpa_w1"), g, e, f, gamma)
    out["cars"] = sm.cars(E, dip, v("cars_shift"), v("cars_w1"), gamma=float(v("cars_gamma")))
    out["Mol_cars"] = sm.cars(E, dip, v("cars_shift"), v("cars_w1"))
    lw = float(v("abs_linewidth"))
    out["absorption_lw"] = sm.absorption(E, dip, v("abs_w"), linewidth=lw)
    out["absorption_default"] = sm.absorption(E, dip, v("abs_w"))
    out["absorption_norm"] = sm.absorption(E, dip, v("abs_w"), linewidth=lw, normalize=True)
    lg = float(v("la_gamma"))
    out["linear_absorption"] = sm.linear_absorption(v("abs_w"), v("la_e"), v("la_d"), gamma=lg)
    out["linear_absorption_norm"] = sm.linear_absorption(v("abs_w"), v("la_e"), v("la_d"), gamma=lg, normalize=True)
    return out


OUTPUTS = ["GSB", "SE", "ESA", "SE_t3", "ESA_t3", "SE_t3_default", "PE2", "PE2_se", "PE2_esa", "PE2_se_lists",
           "PE2_esa_lists", "DQC_R1_t3", "DQC_R1_t1", "DQC_R2_t3", "DQC_R2_t1", "TPA_scalar", "TPA_array", "TPA2D",
           "TPA2D_time_order", "cars", "Mol_cars", "absorption_lw", "absorption_default", "absorption_norm",
           "linear_absorption", "linear_absorption_norm"]
INPUTS = ["E", "dip", "gamma", "g", "e", "f", "w1s", "w3s", "tau2", "w1", "w2", "t3", "deph", "pe_w1", "pe_deph", "dq_w1",
          "dq_w2", "dq_w3", "dq_tau", "tpa_wp", "tpa_w1", "cars_shift", "cars_w1", "cars_gamma", "abs_w", "abs_linewidth",
          "la_e", "la_d", "la_gamma"]


def test_fixture_holds_exactly_the_listed_entries(fx):
    want = {f"{t}_{k}" for t in "ab" for k in OUTPUTS + INPUTS} | {"lib_versions"}
    assert set(fx) == want
    assert fx["b_dip"].dtype == np.complex128 and np.abs(fx["b_dip"].imag).max() > 0.05
    assert fx["a_gamma"][0] == 0 and fx["b_gamma"][0] == 0
    assert fx["a_SE_t3"].shape == (7, 11) and fx["a_TPA2D"].shape == (11, 7)


@pytest.mark.parametrize("tag", ["a", "b"])
def test_restatement_matches_every_reference_output(fx, tag):
    got = model_outputs(fx, tag)
    assert sorted(got) == sorted(OUTPUTS)
    for name in OUTPUTS:
        ref = fx[f"{tag}_{name}"]
        assert np.shape(got[name]) == ref.shape, name
        err = relerr(got[name], ref)
        print(f"{tag} {name}: relerr {err:.2e}")
        assert err < TOL, (name, err)


def test_dqc_r1_t3_ignores_the_values_of_omega1(fx):
    """Reference behaviour 2: both Green's functions sit at omega2, every row of the result is the same."""
    S = fx["b_DQC_R1_t3"]
    assert S.shape == (11, 7) and np.array_equal(S, np.tile(S[0], (11, 1)))


def test_restatement_with_empty_lists_is_zero(fx):
    m = _m(fx, "a")
    w1, w2 = fx["a_w1"], fx["a_w2"]
    S = sm.ESA(m["E"], m["dip"], w1, w2, 1.0, [0], m["e"], [], m["gamma"])
    assert S.shape == (7, 11) and not S.any()
    assert not sm.GSB(m["E"], m["dip"], w1, w2, 1.0, [0], [], m["gamma"]).any()


# ------------------------------------------------------------------------------------------------ refusals
def _mol(fx, tag="a", gamma=True):
    from pyqed_amd.mol import Mol
    mol = Mol(np.diag(fx[f"{tag}_E"]), fx[f"{tag}_dip"])
    mol.edip_rms = fx[f"{tag}_dip"]
    if gamma:
        mol.set_decay(fx[f"{tag}_gamma"])
    return mol


def test_mol_setters(fx):
    mol = _mol(fx, gamma=False)
    assert mol.gamma is None and mol.dephasing == 0.
    mol.set_decay_for_all(0.03)
    assert mol.gamma == [0] + [0.03] * 5
    mol.set_decay([1, 2, 3])
    assert mol.gamma == [1, 2, 3]
    mol.set_dephasing(0.4)
    assert mol.dephasing == 0.4
    for name in ("DQC", "TPA", "ETPA"):   # empty stubs in the reference: nothing is added for them
        assert not hasattr(mol, name)


def test_photon_echo_t3_needs_gamma(fx):
    mol = _mol(fx, gamma=False)
    with pytest.raises(ValueError, match="Please set the decay constants gamma first."):
        mol.PE2(fx["a_pe_w1"], fx["a_w2"], t3=1.0)


def test_absorption_refusals(fx):
    from pyqed_amd import sos
    from pyqed_amd.mol import Mol
    mol = _mol(fx)
    with pytest.raises(NotImplementedError, match="has not been implemented"):
        mol.absorption(fx["a_abs_w"], method="tcf")
    E = fx["a_E"].copy()
    E[[2, 3]] = E[[3, 2]]
    with pytest.raises(ValueError, match="Eigenenergies are not sorted."):
        Mol(np.diag(E), fx["a_dip"]).absorption(fx["a_abs_w"])
    with pytest.raises(ValueError, match="complex"):
        Mol(np.diag(fx["a_E"] - 0.01j), fx["a_dip"]).absorption(fx["a_abs_w"])
    with pytest.raises(ValueError, match="complex"):
        sos.linear_absorption(fx["a_abs_w"], fx["a_la_e"] + 0.01j, fx["a_la_d"])


@pytest.mark.parametrize("fn", ["DQC_R1", "DQC_R2"])
@pytest.mark.parametrize("kw", [dict(), dict(omega1=[1.0]), dict(tau3=1.0), dict(omega3=[1.0]),
                                dict(omega1=[1.0], omega3=[1.0], tau1=1.0, tau3=1.0)])
def test_dqc_needs_a_grid_and_delay_pair(fx, fn, kw):
    from pyqed_amd import sos
    m = _m(fx, "a")
    with pytest.raises(Exception, match="Input Error! Please specify either omega1, tau3 or omega3, tau1."):
        getattr(sos, fn)(m["E"], m["dip"], omega2=[2.0], g_idx=[0], e_idx=m["e"], f_idx=m["f"], gamma=m["gamma"], **kw)


def test_tpa_refusals(fx):
    from pyqed_amd import sos
    m = _m(fx, "a")
    args = (m["g"], m["e"], m["f"], m["gamma"])
    with pytest.raises(ValueError, match="degenerate"):
        sos.TPA(m["E"], m["dip"], 2.0, *args, degenerate=False)
    Ec = m["E"] - 0.01j
    for call in (lambda: sos.TPA(Ec, m["dip"], 2.0, *args),
                 lambda: sos.TPA2D(Ec, m["dip"], [2.0], [1.0], *args),
                 lambda: sos.TPA2D_time_order(Ec, m["dip"], [2.0], [1.0], *args)):
        with pytest.raises(ValueError, match="complex"):
            call()


def test_bad_models_are_refused_on_the_host(fx):
    from pyqed_amd import sos
    m = _m(fx, "a")
    with pytest.raises(ValueError, match="e_idx must index"):
        sos.GSB(m["E"], m["dip"], [1.0], [1.0], 0.0, [0], [1, 6], m["gamma"])
    with pytest.raises(ValueError, match="f_idx must index"):
        sos.ESA(m["E"], m["dip"], [1.0], [1.0], 0.0, [0], [1], [-1], m["gamma"])
    with pytest.raises(ValueError, match="do not agree"):
        sos.SE(m["E"], m["dip"][:5, :5], [1.0], [1.0], 0.0, [0], [1], m["gamma"])
    with pytest.raises(ValueError, match="at least one"):
        sos.SE(m["E"], m["dip"], [], [1.0], 0.0, [0], [1], m["gamma"])
    with pytest.raises(ValueError, match="gamma"):
        sos.DQC_R2(m["E"], m["dip"], omega1=[1.0], omega2=[2.0], tau3=1.0, e_idx=[1], f_idx=[4])


def test_helpers():
    from pyqed_amd import sos
    assert sos.issorted(np.array([0.0, 1.0, 1.0, 2.0])) and not sos.issorted(np.array([0.0, 2.0, 1.0]))
    x = np.linspace(-1, 1, 5)
    assert np.allclose(sos.lorentzian(x, 0.1), 0.1 / (np.pi * (0.01 + x ** 2)), rtol=1e-15)
    assert sos.au2mev == 27.2116e3


def test_gpu_edge_sizes_follow_the_kernels_constants():
    """tests/test_sos_signals_gpu.py places its edge sizes around the constants of csrc/sos_signals_tiles.hpp."""
    import os
    import re
    import test_sos_signals_gpu as tg
    from conftest import ROOT
    txt = open(os.path.join(ROOT, "pyqed_amd", "csrc", "sos_signals_tiles.hpp")).read()
    consts = {k: int(v) for k, v in re.findall(r"constexpr int (SOS_[A-Z]+) = (\d+);", txt)}
    assert consts == {k: getattr(tg, k) for k in ("SOS_THREADS", "SOS_QCHUNK", "SOS_TILE", "SOS_PCHUNK")}


# ------------------------------------------------------------------------------------------------ the C entries
def test_c_entries_check_their_arguments_before_any_hip_call():
    """As test_abi.test_version_and_error_string: QD_EINVAL on null pointers and negative sizes, without a GPU."""
    from pyqed_amd import _lib
    lib = _lib.load()
    one = 0x1000   # a non-null address no check dereferences
    ps = lambda *a: lib.qd_sos_polesum(*a)
    assert ps(one, one, one, 2, 2, one, 3, one, 3, 0, 0, None, 3, 1, 0, None) == _lib.QD_EINVAL
    assert "null pointer" in _lib.last_error()
    assert ps(one, one, None, 2, 2, one, 3, one, 3, 0, 0, one, 3, 1, 0, None) == _lib.QD_EINVAL
    assert ps(None, one, one, 2, 2, one, 3, one, 3, 0, 0, one, 3, 1, 0, None) == _lib.QD_EINVAL
    assert "null pole table" in _lib.last_error()
    assert ps(one, one, one, 2, 2, None, 3, one, 3, 0, 0, one, 3, 1, 0, None) == _lib.QD_EINVAL
    assert "null grid" in _lib.last_error()
    assert ps(one, one, one, 2, 2, None, 3, None, 3, 2, 1, one, 3, 1, 0, None) == _lib.QD_EINVAL   # diagonal needs y
    assert ps(one, one, one, -1, 2, one, 3, one, 3, 0, 0, one, 3, 1, 0, None) == _lib.QD_EINVAL
    assert "bad sizes" in _lib.last_error()
    assert ps(one, one, one, 2, -1, one, 3, one, 3, 0, 0, one, 3, 1, 0, None) == _lib.QD_EINVAL
    assert ps(one, one, one, 2, 2, one, 0, one, 3, 0, 0, one, 3, 1, 0, None) == _lib.QD_EINVAL
    assert ps(one, one, one, 2, 2, one, 3, one, -3, 0, 0, one, 3, 1, 0, None) == _lib.QD_EINVAL
    assert ps(one, one, one, 2, 2, one, 3, one, 3, 3, 0, one, 3, 1, 0, None) == _lib.QD_EINVAL
    assert "xkind" in _lib.last_error()
    assert ps(one, one, one, 2, 2, one, 3, one, 3, 0, 2, one, 3, 1, 0, None) == _lib.QD_EINVAL
    assert ps(one, one, one, 2, 2, one, 3, one, 4, 0, 0, one, 3, 1, 0, None) == _lib.QD_EINVAL   # rows overlap
    assert "strides" in _lib.last_error()
    assert ps(one, one, one, 2, 2, one, 3, one, 4, 0, 0, one, 2, 2, 0, None) == _lib.QD_EINVAL
    assert ps(one, one, one, 1 << 20, 1 << 20, one, 3, one, 4, 0, 0, one, 4, 1, 0, None) == _lib.QD_EINVAL
    assert "2^31" in _lib.last_error()

    pw = lambda *a: lib.qd_sos_pathway(*a)
    ok = [0, one, one, one, 6, 0.0, one, 1, one, 3, one, 2, 0.0, one, 4, one, 5, one, 0, None]

    def bad(pos, val):
        a = list(ok)
        a[pos] = val
        return pw(*a)
    for pos in (1, 2, 3, 13, 15, 17):
        assert bad(pos, None) == _lib.QD_EINVAL
        assert "null pointer" in _lib.last_error()
    for pos in (6, 8, 10):
        assert bad(pos, None) == _lib.QD_EINVAL
        assert "null index list" in _lib.last_error()
    for pos, val in ((4, 0), (4, -6), (7, -1), (9, -1), (11, -1), (14, 0), (16, -2), (9, 7)):
        assert bad(pos, val) == _lib.QD_EINVAL
        assert "bad sizes" in _lib.last_error()
    for val in (-1, 10):
        assert bad(0, val) == _lib.QD_EINVAL
        assert "unknown pathway" in _lib.last_error()

    tp = lambda *a: lib.qd_sos_tpa(*a)
    ok = [one, one, one, 6, one, 3, one, 2, one, 4, one, 5, 1, one, None]

    def badt(pos, val):
        a = list(ok)
        a[pos] = val
        return tp(*a)
    for pos in (0, 1, 2, 8, 13):
        assert badt(pos, None) == _lib.QD_EINVAL
        assert "null pointer" in _lib.last_error()
    for pos in (4, 6):
        assert badt(pos, None) == _lib.QD_EINVAL
        assert "null index list" in _lib.last_error()
    for pos, val in ((3, 0), (5, -1), (7, -1), (9, 0), (11, -1), (10, None)):   # w1 == NULL needs n1 == 1
        assert badt(pos, val) == _lib.QD_EINVAL
        assert "bad sizes" in _lib.last_error()
