"""qd_superop_rk4 (pyqed_amd/csrc/superop.hip) member by member at the tails and paddings of both forms, against the
extended-precision RK4 of oracle/highprec.py (tests/test_highprec_oracle_cpu.py).

Inputs everywhere: L a dense random complex matrix / sqrt(N2) (no structure a transposed or conjugated read could
hide behind), dt = 0.2 (||dt L|| ~ 0.6: every Horner coefficient matters), member b scaled by 1 + b (a swap of two
members shows), W random complex (never vec(I)).  Asserted everywhere: max_b relerr(got[b], ref[b]) < 1e-12,
separately for the final state, every snapshot and the observable block obs[b] (every step, every W row).  The
reference's own rounding is 1e-16 per member in float64 and 1e-19 in extended precision; one dropped term at N2 = 515
moves a member by 1e-4."""
import numpy as np
import pytest

from conftest import took
from oracle import highprec as hp

pytestmark = pytest.mark.gpu
BOUND = 1e-12


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda", 0))


def _inputs(N2, B, ne, seed=0):
    rng = np.random.default_rng([seed, N2, B, ne])
    c = lambda *sh: rng.standard_normal(sh) + 1j * rng.standard_normal(sh)   # noqa: E731
    L = c(N2, N2) / np.sqrt(N2)
    v0 = c(B, N2) * (1.0 + np.arange(B))[:, None]
    W = c(ne, N2) if ne else None
    return L, v0, W


def _run(Ld, v0, dt, nsteps, W, save_every):
    """(v, snap, obs, paths) of one superop_rk4 call on the first len(v0) members."""
    from pyqed_amd.oqs import superop_rk4
    v = _t(v0.copy())
    took("")
    obs, snap = superop_rk4(Ld, v, dt, nsteps, None if W is None else _t(W), save_every=save_every)
    paths = took("")[1]
    return (v.cpu().numpy(), None if snap is None else snap.cpu().numpy(),
            None if obs is None else obs.cpu().numpy(), paths)


def _errors(got, ref):
    """Worst member error of the final state, of each snapshot and of the observable block."""
    v, snap, obs = got
    rv, rsnap, robs = ref
    out = {"final": hp.worst_member(v, rv)}
    assert (snap is None) == (rsnap is None) and (obs is None) == (robs is None)
    if rsnap is not None:
        assert snap.shape == rsnap.shape
        for k in range(rsnap.shape[1]):
            out[f"snap{k}"] = hp.worst_member(snap[:, k], rsnap[:, k])
    if robs is not None:
        out["obs"] = hp.worst_member(obs, robs)
    return out


def _check(label, errs):
    print(f"{label}: " + ", ".join(f"{k} {e:.2e}" for k, e in errs.items()))
    bad = {k: e for k, e in errs.items() if not e < BOUND}
    assert not bad, (label, bad)


@pytest.mark.parametrize("N2", [1, 9, 63, 65, 127, 129, 255, 257, 515])
def test_gemv_every_group_size_at_column_and_row_tails(N2):
    """The wave-per-rows form for B = 1 .. 16 at every N2 (one L, one 16-member extended-precision reference whose
    first B members serve batch B): B = 1 .. 8 launch superop_rows_kernel<NB, R, U> for every NB as a whole batch,
    B = 9 .. 16 launch it again as the tail group behind a full group of 8, at a member offset.  No N2 is a multiple of
    64: the column mask, the last partial 64 U chunk (U = 4: 256 columns, U = 2: 128) and, where N2 is odd, the row
    clamp and row guard of R = 4 and R = 2 all run.  5 steps, a snapshot every 2 (the fifth step is no save), ne = 3.
    Worst seen on an MI355X over all N2 and B: states 2.3e-16, observable block 4.3e-16 (N2 = 129)."""
    nsteps, se, ne, dt, Bmax = 5, 2, 3, 0.2, 16
    L, v0, W = _inputs(N2, Bmax, ne)
    ref = hp.superop(L, v0, dt, nsteps, W, se)
    Ld = _t(L)
    worst = {}
    for B in range(1, Bmax + 1):
        v, snap, obs, paths = _run(Ld, v0[:B], dt, nsteps, W, se)
        assert paths == ["superop_gemv"], paths
        assert snap.shape == (B, nsteps // se, N2) and obs.shape == (B, nsteps + 1, ne)
        errs = _errors((v, snap, obs), tuple(r[:B] for r in ref))
        bad = {k: e for k, e in errs.items() if not e < BOUND}
        assert not bad, (N2, B, bad)
        for k, e in errs.items():
            worst[k] = max(worst.get(k, 0.0), e)
    _check(f"gemv N2={N2} B=1..{Bmax}", worst)


def test_observables_past_64_rows_of_w():
    """ne = 70 > the 64 blocks of superop_obs_kernel's grid: rows 64 .. 69 come from the second trip of its loop over
    m.  N2 = 65, B = 3, every obs[b, step, m] against extended precision.  Worst seen: states 1.4e-16, observables
    1.9e-16."""
    N2, B, ne, nsteps, se, dt = 65, 3, 70, 5, 2, 0.2
    L, v0, W = _inputs(N2, B, ne)
    ref = hp.superop(L, v0, dt, nsteps, W, se)
    v, snap, obs, paths = _run(_t(L), v0, dt, nsteps, W, se)
    assert paths == ["superop_gemv"], paths
    assert obs.shape == (B, nsteps + 1, ne)
    _check("ne=70", _errors((v, snap, obs), ref))
    # every entry on its own as well, against the largest entry of its member
    top = np.abs(ref[2]).reshape(B, -1).max(axis=1)[:, None, None]
    assert np.all(np.abs(obs - ref[2]) < BOUND * top)


def test_gemv_many_groups_below_the_gemm_threshold():
    """B = 50 at N2 = 9 stays on the GEMV (the GEMM needs N2 >= 64): six full groups and a tail of two, one partial
    wave per group.  Extended precision, all members.  Worst seen: states 2.2e-16, observables 3.5e-16."""
    N2, B, nsteps, se, dt = 9, 50, 5, 2, 0.2
    L, v0, W = _inputs(N2, B, 3)
    ref = hp.superop(L, v0, dt, nsteps, W, se)
    v, snap, obs, paths = _run(_t(L), v0, dt, nsteps, W, se)
    assert paths == ["superop_gemv"], paths
    _check("gemv N2=9 B=50", _errors((v, snap, obs), ref))


# N2, B, nsteps, save_every, with W, engine path, reference
GEMM_CASES = [
    (64, 48, 5, 2, True, "ens_gemm64", "extended"),      # the smallest GEMM shape: N2p = 128, Bp = 64, S = 1
    (70, 50, 5, 2, True, "ens_gemm64", "extended"),      # N2p = 128 with 58 padded rows and columns of L, Bp = 64
    (70, 50, 5, 0, False, "ens_gemm64", "extended"),     # no W, no snapshot: unpacked after the last step only
    (129, 65, 5, 2, True, "ens_gemm64", "extended"),     # N2p = 256, Bp = 128: split_plan, 64-blocks, S = 4
    (1024, 128, 5, 2, True, "ens_gemm64", "float64"),    # the plan asks for 16 slabs, MAXS = 8 holds it to 8
    (4096, 128, 3, 2, True, "ens_gemm128", "float64"),   # 128-blocks, S = 8; L is 268 MB; third step is no save
]


@pytest.mark.parametrize("N2,B,nsteps,se,with_w,engine,refkind", GEMM_CASES)
def test_gemm_form_paddings_and_plans(N2, B, nsteps, se, with_w, engine, refkind):
    """The MFMA form (B >= 48 and N2 >= 64) through every branch of cgemm_splitk_slabs that it can reach; the engine
    path is asserted by its exact name, so `ens_gemm128` here is the plain kernel, not the xtab one.  Reference, all
    members in every case: extended precision up to N2 = 129; at N2 = 1024 and 4096, where extended precision would
    take minutes, the float64 run of the same oracle code (1e-16 from the extended one, test_highprec_oracle_cpu), and
    at N2 = 1024 members 0, 64 and 127 in extended precision besides.  Worst seen on an MI355X: against extended
    precision states 3.1e-16 and observables 6.8e-16 (N2 = 70); against float64 states 5.1e-16 and observables
    2.1e-15 (N2 = 4096, where the float64 reference's own 4096-term sums round at that size: the three extended members
    at N2 = 1024 give 2.5e-16 where float64 gives 1.2e-15)."""
    dt = 0.2
    L, v0, W = _inputs(N2, B, 3 if with_w else 0)
    ref = hp.superop(L, v0, dt, nsteps, W, se, dtype=np.clongdouble if refkind == "extended" else np.complex128)
    v, snap, obs, paths = _run(_t(L), v0, dt, nsteps, W, se)
    assert paths[0] == "superop_gemm" and set(paths[1:]) == {engine}, paths
    if not with_w:
        assert snap is None and obs is None
    _check(f"gemm N2={N2} B={B} se={se} W={with_w}", _errors((v, snap, obs), ref))
    if N2 == 1024:
        sel = [0, 64, 127]
        refx = hp.superop(L, v0[sel], dt, nsteps, W, se)
        _check("gemm N2=1024 members 0, 64, 127 in extended precision", _errors((v[sel], snap[sel], obs[sel]), refx))
