#!/usr/bin/env python
"""Time per step of the matrix-free Jacobi-coordinate LDR propagation (qd_ldr_jacobi_run) against two yardsticks, in
one process and in alternation, at 63 x 63 (M = ns = 2), 127 x 127 (M = 6, ns = 3) and 255 x 255 (M = ns = 2) for
B = 1 and 16.  Neither yardstick is code under test:

  torch_rows    the reference's arithmetic restated in torch: the same expand / project, the per-row dense expTy
                [nx, ny, ny] applied by a batched matmul with the source row's matrix, expKx by an einsum
  ldr_kernels   the plain qd_ldr_run step of the same shape (one fixed matrix per axis): equal by flop count

Stand-alone; bench.py is the flagship benchmark.  One JSON line per (shape, B, path): the median, minimum and maximum
over --regions timed regions of the time per step (device events around one call of `steps` steps, after a warm-up of
the same shape; the regions of the paths of a shape alternate), and for the Jacobi path `faster`: whether its median
beats torch_rows' by more than the two spreads (max - min) combined, and `vs_plain`: its median over the plain step's,
with the two spreads over the plain median beside it.

    python tools/bench_ldr_jacobi.py [--regions 5] [--window 0.3] [--out profiles/ldr_jacobi/bench_ldr_jacobi.jsonl]

--trace runs 20 steps of every shape on the Jacobi path only, for a kernel trace taken by a profiler around this
process; --passes FILE.csv reads such a trace and prints one JSON line per (shape, B, pass): the median kernel time
against the pass' own bounds, 4 n flop per complex element of chi for the real passes and 8 n for the plain one at the
FP64 matrix peak, and 32 B per element at the HBM peak.
"""
from __future__ import annotations

import argparse
import csv
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_ldr import (NSUB, PEAK_F64_MATRIX, PEAK_HBM, RT, SUB, TPB, TRACE_STEPS, emit,  # noqa: E402
                       measure_alternating, model)

#          dims          M  ns
SHAPES = [((63, 63), 2, 2), ((127, 127), 6, 3), ((255, 255), 2, 2)]
BATCHES = (1, 16)
DOMAINS = ((0.5, 3.5), (0.0, np.pi))


def jacobi_factors(dims, dt):
    """S, the phase table and the per-row matrices of T = p_r^2 / 2 mu + p_theta^2 / 2 I(r), I = 2 r^2, and expTx."""
    from pyqed_amd import sine_dvr
    dx, dy = sine_dvr(*DOMAINS[0], dims[0], mass=1.3), sine_dvr(*DOMAINS[1], dims[1])
    S = dy.fbr2dvr()
    ph = np.exp(-1j * dt * dy.levels()[None, :] / (2.0 * dx.x ** 2)[:, None])
    return S, ph, dx.expT(dt)


def torch_rows_fn(torch, U, eV, eVh, Kx, rows, psi0):
    """The reference's step (ldr.py:1961, 1979) without the dense A: expand, the source row's matrix along y as a
    batched matmul, expKx along x, project."""
    Uc = U.conj().resolve_conj()

    def fn(steps):
        psi = psi0 * eVh
        for _ in range(steps):
            chi = torch.einsum("...mb,z...b->z...m", U, psi)
            chi = torch.matmul(rows, chi)                    # [nx, ny, ny] @ [B, nx, ny, M]
            chi = torch.einsum("ik,zk...->zi...", Kx, chi)
            psi = eV * torch.einsum("...ma,z...m->z...a", Uc, chi)
        return psi
    return fn


def passes_of(dims, M, B):
    """(pass name, kernel, template arguments, n, flop per element and n, grid in workgroups) of the fused path, as
    ldr_jacobi_plan plans it."""
    npts, n = int(np.prod(dims)), dims[-1]
    C = B * npts * M // n
    out = [("forward", "ldr_real_axis_kernel", "true,true,false", n, 4, (-(-C // (NSUB * SUB)), -(-n // RT)))]
    for d in range(len(dims) - 1):
        Cd = B * npts * M // dims[d]
        out.append((f"plain{d}", "ldr_axis_kernel", "false,false", dims[d], 8,
                    (-(-Cd // (NSUB * SUB)), -(-dims[d] // RT))))
    cu = (SUB // M) * M
    out.append(("back", "ldr_real_axis_kernel", "false,false,true", n, 4, (-(-C // (NSUB * cu)), -(-n // RT))))
    return out


def summarise_passes(path, out):
    by = {}
    for r in csv.DictReader(open(path)):
        name = r["Kernel_Name"]
        if "ldr_real_axis_kernel<" not in name and "ldr_axis_kernel<" not in name:
            continue
        kern = "ldr_real_axis_kernel" if "ldr_real_axis_kernel<" in name else "ldr_axis_kernel"
        targs = name.split("<")[1].split(">")[0].replace(" ", "")
        key = (kern, targs, int(r["Grid_Size_X"]), int(r["Grid_Size_Y"]))
        by.setdefault(key, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-9)
    lines = []
    for dims, M, ns in SHAPES:
        for B in BATCHES:
            for name, kern, targs, n, fl, grid in passes_of(dims, M, B):
                # grid sizes count work-items in a trace (workgroups, should a profiler report those)
                ts = by.get((kern, targs, grid[0] * TPB, grid[1])) or by.get((kern, targs, grid[0], grid[1]))
                if not ts:
                    continue
                elems = B * int(np.prod(dims)) * M
                t = float(np.median(ts))
                t_mfma, t_hbm = fl * n * elems / PEAK_F64_MATRIX, 32.0 * elems / PEAK_HBM
                lines.append(json.dumps({
                    "bench": "ldr_jacobi_pass", "dims": list(dims), "M": M, "ns": ns, "B": B, "pass": name,
                    "kernel": f"{kern}<{targs}>", "n": n, "flop_per_element": fl * n, "dispatches": len(ts),
                    "us": t * 1e6, "us_min": min(ts) * 1e6, "us_max": max(ts) * 1e6,
                    "bound": "mfma" if t_mfma > t_hbm else "hbm", "us_bound": max(t_mfma, t_hbm) * 1e6,
                    "fraction_of_bound": max(t_mfma, t_hbm) / t}))
    emit(lines, out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.3, help="seconds of work per timed region")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    ap.add_argument("--trace", action="store_true", help="Jacobi path only, a fixed number of steps per shape")
    ap.add_argument("--passes", default=None, help="summarise a kernel-trace CSV per pass instead of running")
    args = ap.parse_args()
    if args.passes:
        return summarise_passes(args.passes, args.out)
    import torch
    from pyqed_amd import ldr_jacobi_run, ldr_run
    if not torch.cuda.is_available():
        raise SystemExit("bench_ldr_jacobi needs a GPU: no timing is taken on a CPU")
    dev = torch.device("cuda", 0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=complex))).to(dev)   # noqa: E731
    dt = 0.01
    lines = []
    for dims, M, ns in SHAPES:
        for B in BATCHES:
            Uh, apes, Kh, psih = model(dims, M, ns, B)
            Sh, phh, Kxh = jacobi_factors(dims, dt)
            U, psi, Kx, ph = t(Uh), t(psih), t(Kxh), t(phh)
            S = torch.from_numpy(np.ascontiguousarray(Sh)).to(dev)
            eV, eVh = t(np.exp(-1j * dt * apes)), t(np.exp(-0.5j * dt * apes))
            snap = torch.empty((B, 1) + tuple(dims) + (ns,), dtype=torch.complex128, device=dev)

            def jacobi(steps):
                ldr_jacobi_run(psi, U, None, S, S, ph, [Kx], dt, steps, steps, expV=eV, expVh=eVh, snap=snap)
            if args.trace:
                jacobi(2)
                torch.cuda.synchronize()
                jacobi(TRACE_STEPS)
                torch.cuda.synchronize()
                continue
            rows = t(np.einsum("am,im,mb->iab", Sh, phh, Sh))
            Ky = t(Kh[1])
            snap_p = torch.empty_like(snap)

            def plain(steps):
                ldr_run(psi, U, None, [Kx, Ky], dt, steps, steps, expV=eV, expVh=eVh, snap=snap_p)
            tfn = torch_rows_fn(torch, U, eV, eVh, Kx, rows, psi)
            # the Jacobi path and the restated reference compute the same state
            jacobi(3)
            diff = float((snap[:, 0] - tfn(3)).abs().max())
            fns = {"ldr_jacobi_kernels": jacobi, "torch_rows": tfn, "ldr_kernels": plain}
            steps, ts = measure_alternating(torch, fns, args.window, args.regions)
            spread = {k: max(v) - min(v) for k, v in ts.items()}
            med = {k: float(np.median(v)) for k, v in ts.items()}
            for name, v in ts.items():
                rec = {"bench": "ldr_jacobi", "dims": list(dims), "M": M, "ns": ns, "B": B,
                       "D": int(np.prod(dims)) * ns, "path": name, "steps": steps[name], "regions": args.regions,
                       "us_per_step": med[name] * 1e6, "us_per_step_min": min(v) * 1e6,
                       "us_per_step_max": max(v) * 1e6}
                if name == "ldr_jacobi_kernels":
                    rec["max_abs_diff_torch_rows"] = diff
                    rec["vs_torch_rows"] = med["torch_rows"] / med[name]
                    rec["faster"] = bool(med["torch_rows"] - med[name] > spread[name] + spread["torch_rows"])
                    rec["vs_plain"] = med[name] / med["ldr_kernels"]
                    rec["spreads_over_plain"] = (spread[name] + spread["ldr_kernels"]) / med["ldr_kernels"]
                lines.append(json.dumps(rec))
                print(lines[-1], flush=True)
            fns.clear()
            del rows
            torch.cuda.empty_cache()
    if args.out and lines:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
