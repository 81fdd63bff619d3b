#!/usr/bin/env python
"""Time per RK4 step of the matrix-free LVC propagation (qd_lvc_rk4) on each path the plan admits, for nel = 3 on
16^2, 24^3, 16^4, 32^4 and 20^5 vibrational levels, the shapes next to the resident limit, and, where a dense H fits
(D <= 8192), the existing dense tdse_rk4 on the same model.  Stand-alone; bench.py is the flagship benchmark.

One JSON line per (shape, path): the median, minimum and maximum over --repeats timed windows of the time per step
(device events around one call of `steps` steps, after a warm-up call of the same shape), and the effective rate
4 * 3 * 16 B * D / t: four stages, each at least reading v and psi and writing out once.

    python tools/bench_lvc.py [--repeats 5] [--window 0.3] [--out profiles/lvc/bench_lvc.jsonl]

--driven times the laser-driven qd_lvc_driven_rk4 instead (one electronic drive, hold mode with hold = 1 and stage mode,
each admitted path) next to the undriven qd_lvc_rk4 on the same model and path, whose ratio is the line's
`vs_undriven`; --scan replaces the shape list by the models between D = 960 and 2046 in one to six modes, for the
driven resident / staged crossover.  Stage mode moves 16 state streams per step where the Horner step moves 12.

--pair times qd_lvc_pair_rk4 (one pair, one block, a record after every step) on 16^3, 24^3 and 20^5 on each admitted
path, next to two baselines on the same two states and path: qd_lvc_rk4 without observables (the propagation floor,
`vs_floor`) and qd_lvc_rk4 with its full record every step (`vs_full_record`, the only in-run reduction there was).
--pair --scan replaces the shapes by models between D = 480 and 1023 in one to six modes, for the pair resident /
staged crossover (LVC_PAIR_RESIDENT_MAX_D).  Results of these go to profiles/lvc_pair/.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(3, (16, 16)), (3, (24, 24, 24)), (3, (16, 16, 16, 16)), (3, (32, 32, 32, 32)), (3, (20, 20, 20, 20, 20)),
          # next to the resident limit (lvc_plan.hpp LVC_RESIDENT_MAX_D) in one, two, four and six modes
          (3, (682,)), (3, (26, 26)), (3, (5, 5, 5, 5)), (3, (3, 3, 3, 3, 3, 2)), (3, (37, 37))]
# resident against staged below the resident limit, one to six modes (--scan)
SCAN = [(3, (342,)), (3, (512,)), (3, (682,)), (3, (18, 19)), (3, (22, 23)), (3, (26, 26)), (3, (7, 7, 7)),
        (3, (8, 8, 8)), (3, (8, 9, 9)), (3, (4, 4, 4, 5)), (3, (5, 5, 5, 5)), (3, (3, 3, 3, 3, 3, 2)),
        (3, (3, 3, 3, 3, 4, 2))]
PAIR_SHAPES = [(3, (16, 16, 16)), (3, (24, 24, 24)), (3, (20, 20, 20, 20, 20))]
# pair resident against pair staged below the pair resident limit, one to six modes (--pair --scan)
PAIR_SCAN = [(3, (170,)), (3, (256,)), (3, (341,)), (3, (13, 13)), (3, (16, 16)), (3, (18, 18)), (3, (6, 6, 6)),
             (3, (7, 7, 6)), (3, (4, 4, 4, 4)), (3, (4, 4, 4, 5)), (3, (3, 3, 3, 3, 3)), (3, (2, 2, 2, 2, 2, 5)),
             (3, (3, 3, 3, 3, 2, 2))]
DENSE_MAX_D = 8192
MAX_STEPS = 50000


def model(nel, dims, seed=0):
    """A Hermitian model with couplings of the size of the frequencies (the timing does not depend on the values)."""
    rng = np.random.default_rng(seed)
    M = len(dims)
    omega = rng.uniform(0.05, 0.15, M)
    Hel = np.diag(np.linspace(0.0, 1.0, nel)).astype(complex)
    a = rng.standard_normal((M, nel, nel)) * 0.05
    W = ((a + a.transpose(0, 2, 1)) / 2).astype(complex)
    return omega, Hel, W


def h_bound(dims, omega, Hel, W):
    b = np.abs(Hel).sum(axis=0).max() + sum(w * (N - 1) for w, N in zip(omega, dims))
    return float(b + sum(np.abs(W[j]).sum(axis=0).max() * 2 * np.sqrt(N / 2) for j, N in enumerate(dims)))


def dense_h(nel, dims, omega, Hel, W):
    """The dense H [D, D] of the model, for the dense tdse_rk4 comparison."""
    from pyqed_amd import LVCOp
    H = LVCOp(Hel, dims).toarray()
    for j in range(len(dims)):
        H = H + LVCOp(W[j], dims, mode=j).toarray()
    levels = np.indices(dims).reshape(len(dims), -1)
    return H + np.diag(np.tile(np.asarray(omega) @ levels, nel))


def time_call(torch, fn, steps):
    """Seconds per step of fn(steps), by device events."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn(steps)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / steps


def measure(torch, fn, window, repeats):
    fn(2)                                   # warm-up: code objects, scratch
    torch.cuda.synchronize()
    t = time_call(torch, fn, 8)
    steps = int(min(max(window / max(t, 1e-9), 8), MAX_STEPS))
    ts = [time_call(torch, fn, steps) for _ in range(repeats)]
    return steps, float(np.median(ts)), float(min(ts)), float(max(ts))


def pair_lines(torch, args, lines, nel, dims, D, omega, Hd, Wd, dt, psi0, lvc_rk4, lvc_pair_rk4):
    """The --pair lines of one shape: per admitted path the pair run with one block and a record after every step, and
    qd_lvc_rk4 of the same two states on that path without observables and with its full record every step."""
    two = torch.cat([psi0, psi0.roll(1, 1)], dim=0)
    for path in ("staged", "resident"):
        pairs = two.clone().reshape(1, 2, D)
        recs = {}

        def pfn(steps, pairs=pairs, path=path, recs=recs):
            if steps not in recs:           # the record buffer is no part of the timed call
                recs[steps] = torch.empty((1, steps + 1, 1, nel, nel), dtype=torch.complex128, device=pairs.device)
            lvc_pair_rk4(pairs, nel, dims, omega, Hd, Wd, dt, steps, save_every=1, blocks=(0,), path=path,
                         rec=recs[steps])
        try:
            pfn(1)
        except ValueError:                  # the pair plan does not admit the path at this D
            continue
        a, b = two.clone(), two.clone()
        obs = {}

        def floor(steps, a=a, path=path):
            lvc_rk4(a, nel, dims, omega, Hd, Wd, dt, steps, observe=False, path=path)

        def full(steps, b=b, path=path, obs=obs):
            if steps not in obs:
                obs[steps] = torch.empty((2, steps + 1, nel * nel * (1 + len(dims)) + len(dims)),
                                         dtype=torch.complex128, device=b.device)
            lvc_rk4(b, nel, dims, omega, Hd, Wd, dt, steps, save_every=1, store=False, path=path, obs=obs[steps])
        res = {}
        for name, fn in ((f"lvc_{path}_floor", floor), (f"lvc_{path}_full_record", full), (f"lvc_pair_{path}", pfn)):
            steps, med, lo, hi = measure(torch, fn, args.window, args.repeats)
            res[name] = med
            rec = {"bench": "lvc_pair", "nel": nel, "dims": list(dims), "D": D, "path": name, "steps": steps,
                   "repeats": args.repeats, "us_per_step": med * 1e6, "us_per_step_min": lo * 1e6,
                   "us_per_step_max": hi * 1e6}
            if name.startswith("lvc_pair_"):
                rec["vs_floor"] = med / res[f"lvc_{path}_floor"]
                rec["vs_full_record"] = med / res[f"lvc_{path}_full_record"]
            line = json.dumps(rec)
            print(line, flush=True)
            lines.append(line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.3, help="seconds of work per timed call")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    ap.add_argument("--shapes", default=None, help='e.g. "16,16;24,24,24" (nel = 3)')
    ap.add_argument("--driven", action="store_true", help="time qd_lvc_driven_rk4 against qd_lvc_rk4")
    ap.add_argument("--scan", action="store_true", help="the crossover scan's shapes instead of the default list")
    ap.add_argument("--pair", action="store_true", help="time qd_lvc_pair_rk4 against qd_lvc_rk4 of the same states")
    args = ap.parse_args()
    import torch
    from pyqed_amd import _lib
    from pyqed_amd.mol import lvc_driven_rk4, lvc_pair_rk4, lvc_rk4, tdse_rk4
    if not torch.cuda.is_available():
        raise SystemExit("bench_lvc needs a GPU: no timing is taken on a CPU")
    dev = torch.device("cuda", 0)
    default = (PAIR_SCAN if args.scan else PAIR_SHAPES) if args.pair else (SCAN if args.scan else SHAPES)
    shapes = default if args.shapes is None else [(3, tuple(int(v) for v in s.split(","))) for s in
                                                 args.shapes.split(";")]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)   # noqa: E731
    lines = []
    if args.driven:
        # one electronic drive sigma_x-like on states 0 and 1; a field small against the model (the timing does not
        # depend on the values); rows enough for the longest call in stage mode
        fv = torch.full((2 * MAX_STEPS + 1, 1), 0.01, dtype=torch.complex128, device=dev)
    for nel, dims in shapes:
        D = nel * int(np.prod(dims))
        omega, Hel, W = model(nel, dims)
        dt = 0.5 / h_bound(dims, omega, Hel, W)
        Hd, Wd = t(Hel), t(W)
        psi0 = torch.zeros((1, D), dtype=torch.complex128, device=dev)
        psi0[0, (nel - 1) * (D // nel)] = 1.0
        runs = []
        if args.pair:
            pair_lines(torch, args, lines, nel, dims, D, omega, Hd, Wd, dt, psi0, lvc_rk4, lvc_pair_rk4)
            continue
        for path in ("staged", "resident"):
            psi = psi0.clone()

            def fn(steps, psi=psi, path=path):
                lvc_rk4(psi, nel, dims, omega, Hd, Wd, dt, steps, observe=False, path=path)
            try:
                fn(1)
            except ValueError:              # the plan does not admit the path at this D
                continue
            _lib.take_path()
            runs.append((f"lvc_{path}", fn))
            if args.driven:
                Ad = torch.zeros((1, nel, nel), dtype=torch.complex128, device=dev)
                Ad[0, 0, 1] = Ad[0, 1, 0] = 1.0
                for sample in ("hold", "stage"):
                    psi = psi0.clone()

                    def dfn(steps, psi=psi, path=path, sample=sample, Ad=Ad):
                        lvc_driven_rk4(psi, nel, dims, omega, Hd, Wd, Ad, [-1], fv, dt, steps, hold=1, sample=sample,
                                       observe=False, path=path)
                    runs.append((f"lvc_driven_{path}_{sample}", dfn))
        if D <= DENSE_MAX_D and not args.driven:
            H = t(dense_h(nel, dims, omega, Hel, W))
            psi = psi0.clone()
            runs.append(("tdse_rk4_dense", lambda steps, psi=psi, H=H: tdse_rk4(H, psi, dt, steps)))
        undriven = {}
        for name, fn in runs:
            steps, med, lo, hi = measure(torch, fn, args.window, args.repeats)
            streams = 16 if name.endswith("_stage") else 12
            rec = {"bench": "lvc", "nel": nel, "dims": list(dims), "D": D, "vector_MiB": D * 16 / 2 ** 20,
                   "path": name, "steps": steps, "repeats": args.repeats, "us_per_step": med * 1e6,
                   "us_per_step_min": lo * 1e6, "us_per_step_max": hi * 1e6,
                   "effective_TBps": streams * 16 * D / med / 1e12}
            if name.startswith("lvc_driven_"):
                rec["vs_undriven"] = med / undriven[name.split("_")[2]]
            elif name.startswith("lvc_"):
                undriven[name.split("_")[1]] = med
            line = json.dumps(rec)
            print(line, flush=True)
            lines.append(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
