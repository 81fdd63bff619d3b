"""qd_tdse_rk4 and qd_tdse_driven_rk4 (pyqed_amd/csrc/tdse.hip) member by member: partial waves and blocks of the row
form, both sides of every dispatch threshold, the paddings and one 128-block plan of the GEMM form, and the driven run's
drive counts, against the extended-precision RK4 of oracle/highprec.py (tests/test_highprec_oracle_cpu.py).

Inputs everywhere: H a dense random complex matrix / sqrt(N), not Hermitian (nothing is right by conjugation or by
reading H for H^T), ne = 2 dense random complex operators, random states, dt = 0.1; plain runs take 5 steps saved
every 2 (the fifth step is no save), driven runs blocks of nout = 3.  Asserted everywhere:
max_b relerr(got[b], ref[b]) < 1e-12, separately for the final state, every snapshot and the observable block obs[b]
(every save, both operators).

Reference: extended precision for every member while N^2 B <= 3e6; above that the float64 run of the same oracle code
for every member and extended precision for members 0, B // 2 and B - 1 besides.  The float64 reference's states are
1e-16 from the extended ones; its observables, N^2-term sums of random operators, round at 2e-15 to 5e-15 themselves,
which is what the kernels' observables show against it (3e-16 to 6e-16 against extended precision)."""
import numpy as np
import pytest

from conftest import took
from oracle import highprec as hp

pytestmark = pytest.mark.gpu
BOUND = 1e-12
DT = 0.1


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda", 0))


def _inputs(N, B, nd=0, nblocks=0, seed=0):
    rng = np.random.default_rng([seed, N, B, nd])
    c = lambda *sh: rng.standard_normal(sh) + 1j * rng.standard_normal(sh)   # noqa: E731
    H = c(N, N) / np.sqrt(N)
    E = c(2, N, N)
    psi0 = c(B, N)
    psi0 /= np.linalg.norm(psi0, axis=1, keepdims=True)
    Hd = c(nd, N, N) / np.sqrt(N) if nd else None
    fv = 0.4 * c(nblocks, nd)
    return H, E, psi0, Hd, fv


def _errors(got, ref):
    psi, snap, obs = got
    rpsi, rsnap, robs = ref
    out = {"final": hp.worst_member(psi, rpsi)}
    assert (snap is None) == (rsnap is None)
    if rsnap is not None:
        assert snap.shape == rsnap.shape
        for k in range(rsnap.shape[1]):
            out[f"snap{k}"] = hp.worst_member(snap[:, k], rsnap[:, k])
    out["obs"] = hp.worst_member(obs, robs)
    return out


def _check(label, errs):
    print(f"{label}: " + ", ".join(f"{k} {e:.2e}" for k, e in errs.items()))
    bad = {k: e for k, e in errs.items() if not e < BOUND}
    assert not bad, (label, bad)


def _judge(label, got, oracle, psi0, extended_members=True):
    """got = (psi, snap, obs) of all members against oracle(psi0_subset, dtype) as the module docstring says."""
    B, N = psi0.shape
    if N * N * B <= 3e6:
        _check(label + " [extended]", _errors(got, oracle(psi0, np.clongdouble)))
        return
    _check(label + " [float64, all members]", _errors(got, oracle(psi0, np.complex128)))
    if not extended_members:
        return
    sel = sorted({0, B // 2, B - 1})
    sub = tuple(None if g is None else g[sel] for g in got)
    _check(label + f" [extended, members {sel}]", _errors(sub, oracle(psi0[sel], np.clongdouble)))


def _plain(N, B, path, nsteps=5, se=2, extended_members=True):
    from pyqed_amd.mol import tdse_rk4
    H, E, psi0, _, _ = _inputs(N, B)
    psi = _t(psi0.copy())
    took("")
    snap, obs = tdse_rk4(_t(H), psi, DT, nsteps, save_every=se, e_ops=_t(E))
    paths = took("")[1]
    assert paths[0] == path, paths
    got = (psi.cpu().numpy(), snap.cpu().numpy(), obs.cpu().numpy())
    assert got[1].shape == (B, nsteps // se, N) and got[2].shape == (B, nsteps // se + 1, 2)
    _judge(f"tdse N={N} B={B} {path}", got, lambda p, dt_: hp.tdse(H, p, DT, nsteps, se, E, dtype=dt_), psi0,
           extended_members)
    return paths


@pytest.mark.parametrize("N", [1, 3, 63, 65, 130, 257])
@pytest.mark.parametrize("B", [1, 2, 5])
def test_row_form_partial_waves_and_blocks(N, B):
    """A wave per row, four rows per block: N = 1, 3 (one partial wave, the later waves of the block return at once),
    63 and 65 (one lane short of a wave, one past it; 65 = 1 mod 4 leaves three idle waves in the last block), 130
    (2 mod 4) and 257 (1 mod 4, five trips of the lane loop, the last with one lane).  Both observable kernels decode
    (b, m) from one block index: B = 2, 5 with ne = 2.  Worst seen on an MI355X: states 2.0e-16, observables
    5.2e-16."""
    assert _plain(N, B, "tdse_rows") == ["tdse_rows"]


@pytest.mark.parametrize("N,B,path", [(512, 63, "tdse_rows"), (512, 64, "tdse_gemm"), (256, 127, "tdse_rows"),
                                      (256, 128, "tdse_gemm"), (257, 129, "tdse_gemm")])
def test_dispatch_thresholds_from_both_sides(N, B, path):
    """(B >= 64 and N >= 512) or (B >= 128 and N >= 256), one member to either side of each edge; the GEMM side pads
    the state to [128][512], [128][256] and, for (257, 129), [256][384], with 127 zero rows and columns of (-iH)^T.
    Worst seen: states 2.2e-16; observables 4.0e-16 against extended precision, 2.6e-15 against float64."""
    paths = _plain(N, B, path)
    if path == "tdse_gemm":
        assert set(paths[1:]) == {"ens_gemm64"}, paths
    else:
        assert paths == ["tdse_rows"], paths


def test_gemm_form_on_128_blocks():
    """N = 2048, B = 512: split_plan(Mp = 512, Np = 2048, tiles = 128) finds 4 x 16 = 64 128-blocks, S = min(256 / 64,
    128 / 4) = 4, 256 workgroups of 32 K-tiles each, neither under-filled nor short: 128-blocks, the smallest
    B N for which the plan says so (N = 1024 needs B = 2048).  Asserts the plain `ens_gemm128`.  float64 oracle for
    all 512 members (state, snapshots, both observables; the norm of every member with them) and no extended
    precision here: three members would take the host 5 s.  Worst seen: states 3.7e-16, observables 5.2e-15 (the
    float64 reference's own rounding, see above)."""
    paths = _plain(2048, 512, "tdse_gemm", extended_members=False)
    assert set(paths[1:]) == {"ens_gemm128"}, paths


def _driven(N, B, nd, nblocks, path, nout=3):
    from pyqed_amd.mol import tdse_driven_rk4
    H0, E, psi0, Hd, fv = _inputs(N, B, nd, nblocks)
    psi = _t(psi0.copy())
    took("")
    snap, obs = tdse_driven_rk4(_t(H0), None if Hd is None else _t(Hd), fv, psi, DT, nout, e_ops=_t(E))
    paths = took("")[1]
    assert set(p for p in paths if p.startswith("tdse")) == {path}, paths
    got = (psi.cpu().numpy(), None if snap is None else snap.cpu().numpy(), obs.cpu().numpy())
    assert got[2].shape == (B, nblocks + 1, 2)
    _judge(f"driven N={N} B={B} nd={nd} nblocks={nblocks}", got,
           lambda p, dt_: hp.tdse_driven(H0, Hd, fv, p, DT, nout, E, dtype=dt_), psi0)
    return got, psi0


def test_driven_without_a_drive():
    """nd = 0 (Hd = None, no field values): two blocks under H0 alone.  N = 65, B = 2.  Worst seen: 2.7e-16."""
    _driven(65, 2, 0, 2, "tdse_rows")


def test_driven_three_complex_drives():
    """nd = 3 with complex field values, so H(t) = H0 - sum_d f[k, d] Hd[d] is no more Hermitian than H0 and every
    f[k, d] is read from its own slot.  N = 65, B = 5, three blocks.  Worst seen: states 1.9e-16, observables
    4.0e-16."""
    _driven(65, 5, 3, 3, "tdse_rows")


def test_driven_no_block_gives_the_t0_row():
    """nblocks = 0: no step, no snapshot, obs[b, 0, m] at t0 for every member, the state untouched.  With no block there
    is no field value, so the host array is empty and its pointer null: qd_tdse_driven_rk4 refused that as a null
    pointer until this test met it (SESolver.run with a pulse and Nt // nout = 1 takes the same road)."""
    got, psi0 = _driven(65, 5, 3, 0, "tdse_rows")
    assert got[1] is None and np.array_equal(got[0], psi0)


def test_driven_gemm_form_at_its_smaller_edge():
    """(N, B) = (256, 128) with three complex drives: every block pads its own H(t) into (-iH)^T and runs the GEMM
    stages.  float64 for all members, extended precision for three.  Worst seen: states 2.6e-16; observables 5.6e-16
    against extended precision, 1.8e-15 against float64."""
    _driven(256, 128, 3, 2, "tdse_gemm")


def test_row_form_refuses_a_grid_past_65535():
    """B * ne = 65536 blocks in y is one more than the grid takes: an error, not a launch."""
    import torch
    from pyqed_amd.mol import tdse_rk4
    dev = torch.device("cuda", 0)
    B = 32768
    H = torch.ones((1, 1), dtype=torch.complex128, device=dev)
    E = torch.ones((2, 1, 1), dtype=torch.complex128, device=dev)
    psi = torch.ones((B, 1), dtype=torch.complex128, device=dev)
    with pytest.raises(ValueError, match=r"B \* ne too large"):
        tdse_rk4(H, psi, DT, 1, save_every=1, e_ops=E)
    assert torch.equal(psi, torch.ones_like(psi))
    # one fewer member fits
    psi = torch.ones((B - 1, 1), dtype=torch.complex128, device=dev)
    snap, obs = tdse_rk4(H, psi, DT, 1, save_every=1, e_ops=E)
    g = 1 + (-1j * DT) + (-1j * DT) ** 2 / 2 + (-1j * DT) ** 3 / 6 + (-1j * DT) ** 4 / 24
    assert abs(psi.cpu().numpy() - g).max() < 1e-15 and abs(obs[:, 1].cpu().numpy() - abs(g) ** 2).max() < 1e-15
