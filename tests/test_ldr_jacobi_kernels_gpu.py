"""qd_ldr_jacobi_run member by member on white noise against the extended-precision restatement
(tests/ldr_jacobi_models.py jacobi_factorised in np.clongdouble): a general real F and an independent general real Fb,
a general complex phase table of the grid's shape, general complex plain-axis matrices, orthonormal complex states;
every probed length up to 129 (ldr_models.PROBE_LENGTHS; tests/test_ldr_jacobi_plan_host.py holds them against the
plan's tile constants) on the transformed axis and on each plain axis in turn in one to three dimensions, every
(M, ns) class on both the fused and the split path where fusable, B = 1 and 3, nout = 1 and 2, two long axes (257 on
the transformed and on the plain axis), fused against split, a row-independent table against qd_ldr_run (the plain
kernel, which this feature leaves as it is), a graph replay bit for bit, psi read only, nt < nout.

Bound: 1e-10 relative per member, the project's standing bound for fp64 GPU paths against reference data.  Largest
member error seen on MI355X over every case of this file (three steps, states of norm one): 8.4e-16 on the fused path
and 9.2e-16 on the split path up to 129 points, 1.2e-15 at the 257-point axes (both fused).  Fused against split on the
same input came out bit for bit equal (0.0 in every case; 1e-14 is asserted), and a row-independent table against
qd_ldr_run stayed below 7.8e-16 (1e-14 asserted).
"""
import numpy as np
import pytest

from conftest import took
from ldr_jacobi_models import EXTENDED_OK, jacobi_factorised, member_errors, random_case
from ldr_models import PROBE_LENGTHS

pytestmark = pytest.mark.gpu

TOL = 1e-10
PAIRS = [(1, 1), (2, 2), (3, 2), (5, 3), (16, 3), (17, 2), (32, 32), (9, 4)]
FUSED_M = {1, 2, 3, 5, 16}
REF_DTYPE = np.clongdouble if EXTENDED_OK else np.complex128


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=complex))).to(torch.device("cuda", 0))


def _r(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=float))).to(torch.device("cuda", 0))


def run_case(c, nt, nout, path="auto"):
    from pyqed_amd import ldr_jacobi_run
    took("ldr")
    snap = ldr_jacobi_run(_t(c["psi"]), c["U"], c["apes"], c["F"], c["Fb"], c["ph"], c["expK"], c["dt"], nt, nout,
                          path=path)
    hit = took("ldr_")[1]
    return snap.cpu().numpy(), hit


def oracle(c, nt):
    return jacobi_factorised(c["psi"], c["U"], c["expV"], c["expVh"], c["F"], c["Fb"], c["ph"], c["expK"], nt, 1,
                             REF_DTYPE).astype(complex)


def check_case(c, path="auto"):
    """nout = 1 and 2 over three steps against the oracle, member by member; the path the plan states."""
    ref = oracle(c, 3)
    want = "ldr_jacobi_split" if path == "split" or c["M"] not in FUSED_M else "ldr_jacobi_fused"
    for nout, sel in ((1, [0, 1, 2]), (2, [1])):
        got, hit = run_case(c, 3, nout, path)
        assert hit == [want], (hit, want)
        assert got.shape == ref[:, sel].shape
        err = member_errors(got, ref[:, sel])
        print(f"dims={c['dims']} M={c['M']} ns={c['ns']} B={len(c['psi'])} nout={nout} {want}: worst {err.max():.2e}")
        assert err.max() < TOL, (c["dims"], c["M"], c["ns"], nout, err)


def placements(n):
    """n alone, on the plain axis 0, on the transformed axis, and the same in three dimensions with n on plain axis 1
    as well."""
    return [(n,), (n, 4), (3, n), (n, 3, 4), (3, n, 5), (3, 4, n)]


@pytest.mark.parametrize("n", [n for n in PROBE_LENGTHS if n <= 129])
def test_axis_length_on_every_axis(n):
    """Every placement of the probed length, each with one (M, ns) class and one B, rotating so that every class and
    both B meet every placement over the lengths."""
    for k, dims in enumerate(placements(n)):
        M, ns = PAIRS[(k + n) % len(PAIRS)]
        B = 1 + 2 * ((k + n // 2) % 2)
        check_case(random_case(1000 * n + k, dims, M, ns, B))


@pytest.mark.parametrize("dims,M,ns,B", [
    # what the rotation leaves out: the widest split class just past a row tile on the transformed axis, a whole row
    # tile there on the fused path with both B, and the member offset of the table at B = 3 beside a long outer block
    ((3, 65), 32, 32, 1), ((3, 4, 65), 32, 32, 3), ((65, 3), 32, 32, 3), ((3, 64), 2, 2, 1), ((3, 4, 64), 5, 3, 3),
    ((64,), 16, 3, 3), ((3, 129), 17, 2, 3), ((129, 3), 3, 2, 1), ((33, 17), 9, 4, 3),
    # the two long cases: 9 K-tiles and 5 row tiles on the transformed and on the plain axis
    ((3, 257), 2, 2, 1), ((257, 3), 3, 2, 3)])
def test_named_combinations_and_long_axes(dims, M, ns, B):
    assert max(dims) in PROBE_LENGTHS or (dims, M) == ((33, 17), 9)
    check_case(random_case(31, dims, M, ns, B))


@pytest.mark.parametrize("M,ns", PAIRS)
@pytest.mark.parametrize("B", [1, 3])
def test_state_counts_in_one_to_three_dimensions(M, ns, B):
    """Every (M, ns) class on the plan's path, and on the split path too where the plan fuses."""
    for k, dims in enumerate(((17,), (5, 33), (3, 4, 17), (33, 2, 3))):
        c = random_case(77 + k, dims, M, ns, B)
        check_case(c)
        if M in FUSED_M and k % 2 == B // 2:
            check_case(c, "split")


@pytest.mark.parametrize("M,ns", [(1, 1), (2, 2), (3, 2), (5, 3), (16, 3), (7, 7), (12, 4)])
def test_fused_and_split_agree(M, ns):
    """The same input through both forms: the rotations and the table are the same products, so they agree to
    rounding.  Bound, by the argument of test_ldr_kernels_gpu.test_fused_and_split_agree: an element passes three
    steps of at most ns + 2 n_last + sum of the plain n_d + M + 1 <= 90 roundings of 1.1e-16 each, which at random
    signs add up to about 1.8e-15 of a member's norm; 1e-14 is five times that."""
    for dims in ((33,), (17, 5), (3, 17, 4), (5, 4, 17)):
        c = random_case(5, dims, M, ns, 3)
        f, hf = run_case(c, 3, 1, "fused")
        s, hs = run_case(c, 3, 1, "split")
        assert hf == ["ldr_jacobi_fused"] and hs == ["ldr_jacobi_split"]
        d = member_errors(f, s).max()
        print(f"dims={dims} M={M} ns={ns}: fused against split {d:.2e}")
        assert d < 1e-14, (dims, d)


@pytest.mark.parametrize("dims,M,ns,path", [((33,), 3, 2, "fused"), ((5, 33), 2, 2, "fused"), ((5, 33), 17, 2, "split"),
                                            ((3, 4, 17), 5, 3, "fused"), ((3, 4, 17), 5, 3, "split")])
def test_row_independent_table_against_the_plain_kernel(dims, M, ns, path):
    """With the same table in every row the step is qd_ldr_run's with K_last = Fb diag(ph) F formed on the host.  The
    sums associate differently (two passes of n_last terms against one), so the two agree to rounding, not bitwise;
    the bound is the 1e-14 of test_fused_and_split_agree by the same count of roundings."""
    from pyqed_amd import ldr_run
    c = random_case(12, dims, M, ns, 3)
    c["ph"] = np.broadcast_to(c["ph"].reshape(-1, dims[-1])[0], dims).copy()
    got, hit = run_case(c, 3, 1, path)
    assert hit == [f"ldr_jacobi_{path}"]
    K_last = (c["Fb"] * c["ph"].reshape(-1, dims[-1])[0][None, :]) @ c["F"]
    plain = ldr_run(_t(c["psi"]), c["U"], c["apes"], c["expK"] + [K_last], c["dt"], 3, 1, path=path).cpu().numpy()
    assert took("ldr_axes_")[0]
    d = member_errors(got, plain).max()
    print(f"dims={dims} M={M} ns={ns} {path}: against qd_ldr_run {d:.2e}")
    assert d < 1e-14, (dims, d)
    assert member_errors(got, oracle(c, 3)).max() < TOL


def test_fused_refused_shapes_and_auto_choice():
    from pyqed_amd import ldr_jacobi_run
    c = random_case(3, (9, 4), 17, 2, 1)
    with pytest.raises(ValueError, match=r"qd_ldr_jacobi_run: the fused path needs \(16 / M\) \* M >= 12 columns of a "
                                         r"tile \(M = 17\)"):
        ldr_jacobi_run(_t(c["psi"]), c["U"], c["apes"], c["F"], c["Fb"], c["ph"], c["expK"], c["dt"], 1, 1,
                       path="fused")
    c = random_case(3, (9, 4), 9, 4, 1)
    assert run_case(c, 1, 1)[1] == ["ldr_jacobi_split"]
    # what the tensor level checks itself
    psi = _t(c["psi"])
    with pytest.raises(ValueError, match=r"ldr_jacobi_run: F and Fb must be \(4, 4\)"):
        ldr_jacobi_run(psi, c["U"], c["apes"], c["F"][:3], c["Fb"], c["ph"], c["expK"], c["dt"], 1)
    with pytest.raises(ValueError, match="ldr_jacobi_run: F and Fb must be real"):
        ldr_jacobi_run(psi, c["U"], c["apes"], c["F"] + 0j, c["Fb"], c["ph"], c["expK"], c["dt"], 1)
    with pytest.raises(ValueError, match=r"ldr_jacobi_run: ph must be \(9, 4\); got \(4, 9\)"):
        ldr_jacobi_run(psi, c["U"], c["apes"], c["F"], c["Fb"], c["ph"].T, c["expK"], c["dt"], 1)
    with pytest.raises(ValueError, match=r"ldr_jacobi_run: psi must be \[B, n, n, n, ns\] for 3 axes"):
        ldr_jacobi_run(psi, c["U"], c["apes"], c["F"], c["Fb"], c["ph"], c["expK"] * 2, c["dt"], 1)


def test_psi_is_read_only_and_trailing_steps_are_dropped():
    """nt = 5, nout = 2: two snapshots, after steps 2 and 4; the input is not written; nt < nout: nothing is launched
    and no path is noted."""
    import torch
    from pyqed_amd import ldr_jacobi_run
    c = random_case(9, (17, 6), 3, 2, 2)
    psi = _t(c["psi"])
    args = (c["U"], c["apes"], c["F"], c["Fb"], c["ph"], c["expK"], c["dt"])
    snap = ldr_jacobi_run(psi, *args, 5, 2)
    ref = oracle(c, 4)
    assert tuple(snap.shape) == (2, 2, 17, 6, 2)
    assert member_errors(snap.cpu().numpy(), ref[:, [1, 3]]).max() < TOL
    assert torch.equal(psi.view(torch.float64), _t(c["psi"]).view(torch.float64))
    took("ldr")
    assert tuple(ldr_jacobi_run(psi, *args, 1, 2).shape) == (2, 0, 17, 6, 2)
    assert took("ldr")[1] == []
    pop, rdm = ldr_jacobi_run(psi, *args, 1, 2, return_states=False)
    assert tuple(pop.shape) == (2, 0, 2) and tuple(rdm.shape) == (2, 0, 2, 2)


@pytest.mark.parametrize("path", ["fused", "split"])
def test_call_replays_from_a_graph(path):
    """One qd_ldr_jacobi_run call captured into a graph replays bit for bit, with an uncaptured call on other data
    between capture and replay."""
    import torch
    from pyqed_amd import ldr_jacobi_run
    dev = torch.device("cuda", 0)
    c = random_case(21, (5, 3, 33), 3, 2, 3)
    other = random_case(22, (4, 17), 5, 3, 2)
    U, eV, eVh, ph = _t(c["U"]), _t(c["expV"]), _t(c["expVh"]), _t(c["ph"])
    F, Fb = _r(c["F"]), _r(c["Fb"])
    Ks = [_t(k) for k in c["expK"]]
    kw = dict(path=path, expV=eV, expVh=eVh)
    eager = ldr_jacobi_run(_t(c["psi"]), U, None, F, Fb, ph, Ks, c["dt"], 3, 1, **kw)
    torch.cuda.synchronize()
    x = _t(c["psi"])
    gs = torch.zeros_like(eager)
    s = torch.cuda.Stream(dev)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        ldr_jacobi_run(x, U, None, F, Fb, ph, Ks, c["dt"], 3, 1, snap=gs, **kw)
    between, _ = run_case(other, 2, 1)
    gs.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(gs.view(torch.float64), eager.view(torch.float64))
    # a second replay on new data in the same buffers
    c2 = random_case(23, (5, 3, 33), 3, 2, 3)
    x.copy_(_t(c2["psi"]))
    g.replay()
    torch.cuda.synchronize()
    eager2 = ldr_jacobi_run(_t(c2["psi"]), U, None, F, Fb, ph, Ks, c["dt"], 3, 1, **kw)
    assert torch.equal(gs.view(torch.float64), eager2.view(torch.float64))
    assert member_errors(between, oracle(other, 2)).max() < TOL
