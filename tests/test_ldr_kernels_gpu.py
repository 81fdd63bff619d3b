"""qd_ldr_run member by member on white noise against the extended-precision restatement (tests/ldr_models.py
ldr_factorised in np.clongdouble): general complex axis matrices, orthonormal complex states, every axis length at
which the kernel takes another tile count (read from the plan: the K-tile, the row tile, the MFMA tile), the probed
length on the first, middle and last axis in turn, every (M, ns) class on both the fused and the split path, B = 1 and
3, one to three dimensions, nout = 1 and 2, and axes of 257 and about 1024 points.  The lengths are
ldr_models.PROBE_LENGTHS; tests/test_ldr_plan_host.py holds them against the plan's tile constants, so nothing here
needs a host compiler.

Bound: 1e-10 relative per member, the project's standing bound for fp64 GPU paths against reference data.  Largest
member error seen on MI355X over every case of this file: 2.3e-15 on the fused path, 2.2e-15 on the split path
(three steps, states of norm one, both at the 1023- and 1025-point axes; 9.8e-16 and 8.9e-16 up to 129 points); fused against split on the same input stayed below the 1e-14 asserted.
"""
import numpy as np
import pytest

from conftest import took
from ldr_models import EXTENDED_OK, PROBE_LENGTHS, ldr_factorised, member_errors, random_case

pytestmark = pytest.mark.gpu

TOL = 1e-10
PAIRS = [(1, 1), (2, 2), (3, 2), (5, 3), (16, 3), (17, 2), (32, 32)]
FUSED_M = {1, 2, 3, 5, 16}
REF_DTYPE = np.clongdouble if EXTENDED_OK else np.complex128


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=complex))).to(torch.device("cuda", 0))


def run_case(c, nt, nout, path="auto"):
    from pyqed_amd import ldr_run
    took("ldr")
    snap = ldr_run(_t(c["psi"]), c["U"], c["apes"], c["expK"], c["dt"], nt, nout, path=path)
    hit = took("ldr_axes_")[1]
    return snap.cpu().numpy(), hit


def check_case(c, path="auto"):
    """nout = 1 and 2 over three steps against the oracle, member by member; the path the plan states."""
    ref = ldr_factorised(c["psi"], c["U"], c["expV"], c["expVh"], c["expK"], 3, 1, REF_DTYPE).astype(complex)
    want = "ldr_axes_split" if path == "split" or c["M"] not in FUSED_M else "ldr_axes_fused"
    for nout, sel in ((1, [0, 1, 2]), (2, [1])):
        got, hit = run_case(c, 3, nout, path)
        assert hit == [want], (hit, want)
        assert got.shape == ref[:, sel].shape
        err = member_errors(got, ref[:, sel])
        print(f"dims={c['dims']} M={c['M']} ns={c['ns']} B={len(c['psi'])} nout={nout} {want}: worst {err.max():.2e}")
        assert err.max() < TOL, (c["dims"], c["M"], c["ns"], nout, err)


def placements(n):
    return [(n,), (n, 4), (3, n), (n, 3, 4), (3, n, 5), (3, 4, n)]


@pytest.mark.parametrize("n", [n for n in PROBE_LENGTHS if n <= 129])
def test_axis_length_on_every_axis(n):
    """Every placement of the probed length, each with one (M, ns) class and one B, rotating so that every class and
    both B meet every placement over the lengths."""
    for k, dims in enumerate(placements(n)):
        M, ns = PAIRS[(k + n) % len(PAIRS)]
        B = 1 + 2 * ((k + n) % 2)
        check_case(random_case(1000 * n + k, dims, M, ns, B))


@pytest.mark.parametrize("dims,M,ns,B", [
    # what the rotation above leaves out: the widest split class just past a row tile on the projecting axis, a whole
    # row tile on the last axis of the fused path, and both B there
    ((3, 65), 32, 32, 1), ((3, 4, 65), 32, 32, 3), ((65, 3), 32, 32, 3), ((3, 64), 2, 2, 1), ((3, 4, 64), 5, 3, 3),
    ((64,), 16, 3, 3), ((3, 129), 17, 2, 3), ((129, 3), 3, 2, 1),
    # many K-tiles and row tiles: 9 and 33 K-tiles, 5 and 17 row tiles, on the first and the last axis
    ((257, 3), 3, 2, 3), ((3, 257), 2, 2, 1), ((2, 257), 17, 2, 1), ((1023,), 2, 2, 1), ((2, 1025), 3, 2, 1),
    ((1025, 2), 5, 3, 1), ((2, 1023), 17, 2, 1)])
def test_named_combinations_and_long_axes(dims, M, ns, B):
    assert max(dims) in PROBE_LENGTHS
    check_case(random_case(31, dims, M, ns, B))


@pytest.mark.parametrize("M,ns", PAIRS)
@pytest.mark.parametrize("B", [1, 3])
def test_state_counts_in_one_to_three_dimensions(M, ns, B):
    for k, dims in enumerate(((17,), (5, 33), (3, 4, 17), (33, 2, 3))):
        check_case(random_case(77 + k, dims, M, ns, B))


@pytest.mark.parametrize("M,ns", [(1, 1), (2, 2), (3, 2), (5, 3), (16, 3), (7, 7), (12, 4)])
def test_fused_and_split_agree(M, ns):
    """The same input through both forms: the rotations are the same sums, so they agree to rounding; each against
    the oracle as well.  Bound: an element passes three steps of at most ns + sum n_d + M <= 50 roundings of 1.1e-16
    each, which at random signs add up to about 1.3e-15 of a member's norm; 1e-14 is seven times that."""
    for dims in ((33,), (17, 5), (3, 17, 4)):
        c = random_case(5, dims, M, ns, 3)
        f, hf = run_case(c, 3, 1, "fused")
        s, hs = run_case(c, 3, 1, "split")
        assert hf == ["ldr_axes_fused"] and hs == ["ldr_axes_split"]
        d = member_errors(f, s).max()
        assert d < 1e-14, (dims, d)
        check_case(c, "split")


def test_split_path_refused_shapes_and_auto_choice():
    from pyqed_amd import ldr_run
    c = random_case(3, (9, 4), 17, 2, 1)
    with pytest.raises(ValueError, match=r"the fused path needs \(16 / M\) \* M >= 12 columns of a tile \(M = 17\)"):
        ldr_run(_t(c["psi"]), c["U"], c["apes"], c["expK"], c["dt"], 1, 1, path="fused")
    c = random_case(3, (9, 4), 9, 2, 1)
    assert run_case(c, 1, 1)[1] == ["ldr_axes_split"]


def test_psi_is_read_only_and_trailing_steps_are_dropped():
    """nt = 5, nout = 2: two snapshots, after steps 2 and 4; the input is not written; nt < nout: nothing."""
    import torch
    from pyqed_amd import ldr_run
    c = random_case(9, (17, 6), 3, 2, 2)
    psi = _t(c["psi"])
    snap = ldr_run(psi, c["U"], c["apes"], c["expK"], c["dt"], 5, 2)
    ref = ldr_factorised(c["psi"], c["U"], c["expV"], c["expVh"], c["expK"], 4, 1, REF_DTYPE).astype(complex)
    assert tuple(snap.shape) == (2, 2, 17, 6, 2)
    assert member_errors(snap.cpu().numpy(), ref[:, [1, 3]]).max() < TOL
    assert torch.equal(psi.view(torch.float64), _t(c["psi"]).view(torch.float64))
    assert tuple(ldr_run(psi, c["U"], c["apes"], c["expK"], c["dt"], 1, 2).shape) == (2, 0, 17, 6, 2)


@pytest.mark.parametrize("path", ["fused", "split"])
def test_call_replays_from_a_graph(path):
    """One qd_ldr_run call captured into a graph replays bit for bit, with an uncaptured call on other data between
    capture and replay."""
    import torch
    from pyqed_amd import ldr_run
    dev = torch.device("cuda", 0)
    c = random_case(21, (33, 5, 3), 3, 2, 3)
    other = random_case(22, (17, 4), 5, 3, 2)
    U, eV, eVh = _t(c["U"]), _t(c["expV"]), _t(c["expVh"])
    Ks = [_t(k) for k in c["expK"]]
    eager = ldr_run(_t(c["psi"]), U, None, Ks, c["dt"], 3, 1, path=path, expV=eV, expVh=eVh)
    torch.cuda.synchronize()
    x = _t(c["psi"])
    gs = torch.zeros_like(eager)
    s = torch.cuda.Stream(dev)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        ldr_run(x, U, None, Ks, c["dt"], 3, 1, path=path, expV=eV, expVh=eVh, snap=gs)
    between, _ = run_case(other, 2, 1)
    gs.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(gs.view(torch.float64), eager.view(torch.float64))
    # a second replay on new data in the same buffers
    c2 = random_case(23, (33, 5, 3), 3, 2, 3)
    x.copy_(_t(c2["psi"]))
    g.replay()
    torch.cuda.synchronize()
    eager2 = ldr_run(_t(c2["psi"]), U, None, Ks, c["dt"], 3, 1, path=path, expV=eV, expVh=eVh)
    assert torch.equal(gs.view(torch.float64), eager2.view(torch.float64))
    ref = ldr_factorised(other["psi"], other["U"], other["expV"], other["expVh"], other["expK"], 2, 1)
    assert member_errors(between, ref).max() < TOL
