"""SESolver.correlation_3op_2t (qd_tdse_pair_corr) grid points per second, beside its yardstick and around the
pair dispatch threshold.  One JSON line per measurement.

  python tools/tdse_corr_bench.py                  N = 256 and 1024, Nt = Ntau = 256, then the threshold sweep
  python tools/tdse_corr_bench.py --cpu-reference  the reference's own correlation_3op_2t on the CPU
                                                   (N = 256, Nt = Ntau = 16; build container only)

Yardstick: the plain tdse_rk4 of 2 Nt states for Ntau - 1 steps with no observable, i.e. the propagation the
correlation cannot avoid.  By operation count the GEMM path adds one B-row GEMM per step to four 2B-row ones:
9/8 of the yardstick's time, plus the reduction kernel.

Threshold sweep: time per state-step of qd_tdse_pair_corr at batch sizes on both sides of the row -> GEMM
dispatch.  The row path's time is linear in B and the GEMM path's is a step function of ceil(2B / 128), so the
crossover is where the row path's per-state cost times 2B reaches the GEMM path's time for one 128-row block.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def problem(N, B, seed=7):
    rng = np.random.default_rng(seed)
    gin = lambda: (rng.standard_normal((N, N)) + 1j * rng.standard_normal((N, N))) / np.sqrt(N)  # noqa: E731
    H = gin()
    H = (H + H.conj().T) / 2
    ops = [gin() for _ in range(3)]
    psi = rng.standard_normal((B, N)) + 1j * rng.standard_normal((B, N))
    psi /= np.linalg.norm(psi, axis=1, keepdims=True)
    return H, ops, psi


def cpu_reference(N, Nt, Ntau, dt):
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import ref_shim
    ref_shim.install()
    from pyqed.mol import SESolver
    H, ops, psi = problem(N, 1)
    t0 = time.perf_counter()
    SESolver(H).correlation_3op_2t(psi[0], ops, dt, Nt, Ntau)
    el = time.perf_counter() - t0
    print(json.dumps({"what": "reference_cpu_correlation_3op_2t", "N": N, "Nt": Nt, "Ntau": Ntau,
                      "seconds": round(el, 3), "grid_points_per_s": round(Nt * Ntau / el, 1)}), flush=True)


def timed(fn, reps):
    """Median wall time of fn() over reps runs, each ended by a device synchronise; one warm-up run first."""
    import torch
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), float(min(ts)), float(max(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="256,1024")
    ap.add_argument("--nt", type=int, default=256)
    ap.add_argument("--ntau", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--dt", type=float, default=0.005)
    ap.add_argument("--no-sweep", action="store_true")
    ap.add_argument("--cpu-reference", action="store_true")
    args = ap.parse_args()
    if args.cpu_reference:
        cpu_reference(256, 16, 16, args.dt)
        return
    import torch
    from pyqed_amd import _lib
    from pyqed_amd.mol import SESolver, tdse_pair_corr, tdse_rk4
    dev = torch.device("cuda", 0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    Nt, Ntau = args.nt, args.ntau
    for N in [int(v) for v in args.sizes.split(",")]:
        H, ops, psi = problem(N, 2 * Nt)
        sol = SESolver(H)
        _lib.take_path()
        full = timed(lambda: sol.correlation_3op_2t(psi[0], ops, args.dt, Nt, Ntau), args.reps)
        paths = sorted(set(_lib.take_path().split()))
        Hd, Ad, Bd, Cd, pd = t(H), t(ops[0]), t(ops[1]), t(ops[2]), t(psi)
        pair = timed(lambda: tdse_pair_corr(Hd, Ad, Bd, Cd, pd[:Nt], args.dt, Ntau), args.reps)
        work = pd.clone()
        yard = timed(lambda: tdse_rk4(Hd, work, args.dt, Ntau - 1), args.reps)
        print(json.dumps({"what": "correlation_3op_2t", "N": N, "Nt": Nt, "Ntau": Ntau, "paths": paths,
                          "method_s": round(full[0], 5), "method_min_max_s": [round(full[1], 5), round(full[2], 5)],
                          "grid_points_per_s": round(Nt * Ntau / full[0], 1),
                          "pair_corr_s": round(pair[0], 5), "pair_min_max_s": [round(pair[1], 5), round(pair[2], 5)],
                          "yardstick_rk4_s": round(yard[0], 5),
                          "yardstick_min_max_s": [round(yard[1], 5), round(yard[2], 5)],
                          "pair_over_yardstick": round(pair[0] / yard[0], 3)}), flush=True)
    if args.no_sweep:
        return
    ntau = 65
    for N, Bs in ((256, (32, 64, 87, 88, 128)), (512, (16, 31, 32, 64)), (1024, (8, 15, 16, 32)),
                  (2048, (4, 8, 9, 16))):
        H, ops, psi = problem(N, max(Bs))
        Hd, Ad, Bd, Cd, pd = t(H), t(ops[0]), t(ops[1]), t(ops[2]), t(psi)
        for B in Bs:
            _lib.take_path()
            el = timed(lambda: tdse_pair_corr(Hd, Ad, Bd, Cd, pd[:B], args.dt, ntau), args.reps)
            path = sorted(set(_lib.take_path().split()))
            print(json.dumps({"what": "pair_sweep", "N": N, "B": B, "states": 2 * B, "ntau": ntau, "path": path,
                              "seconds": round(el[0], 6), "min_max_s": [round(el[1], 6), round(el[2], 6)],
                              "us_per_step": round(el[0] / (ntau - 1) * 1e6, 2),
                              "us_per_state_step": round(el[0] / (ntau - 1) / (2 * B) * 1e6, 4)}), flush=True)


if __name__ == "__main__":
    main()
