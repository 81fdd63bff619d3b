#!/usr/bin/env python
"""Time per step of the matrix-free LDR propagation (qd_ldr_run) against a torch restatement of the same factorised
step (einsum per axis), in one process and in alternation, at 63 x 63 (M = ns = 2), 127 x 127 (M = 6, ns = 3),
255 x 255 (M = ns = 2) and 31^3 (M = ns = 2), for B = 1 and 16; at 63 x 63 x 2, B = 1 also the reference's dense form,
a 1 GB exp_T applied by a torch matmul.  Stand-alone; bench.py is the flagship benchmark.

One JSON line per (shape, B, path): the median, minimum and maximum over --regions timed regions of the time per step
(device events around one call of `steps` steps, after a warm-up of the same shape; the regions of the paths of a shape
alternate), and for the kernel path `faster`: whether its median beats the torch path's by more than the two spreads
(max - min) combined.

    python tools/bench_ldr.py [--regions 5] [--window 0.3] [--out profiles/ldr/bench_ldr.jsonl]

--trace runs 20 steps of every shape on the kernel path only, for a kernel trace taken by a profiler around this
process; --passes FILE.csv reads such a trace (one row per dispatch with Kernel_Name, Start_Timestamp, End_Timestamp,
Grid_Size_X / _Y) and prints one JSON line per (shape, B, pass): the median kernel time against the pass' own bounds,
8 n_d flop per complex element of chi at the FP64 matrix peak and 32 B per element at the HBM peak.
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

#          dims            M  ns
SHAPES = [((63, 63), 2, 2), ((127, 127), 6, 3), ((255, 255), 2, 2), ((31, 31, 31), 2, 2)]
BATCHES = (1, 16)
DENSE = ((63, 63), 2, 2)
PEAK_F64_MATRIX = 78.6e12   # flop/s, DESIGN.md section 1
PEAK_HBM = 8.0e12           # B/s (spec; about 6.3e12 is reached by a copy)
MAX_STEPS = 20000
TRACE_STEPS = 20
TPB, SUB, NSUB, RT = 256, 16, 2, 64   # ldr_plan.hpp, for matching a trace's grids to the passes


def model(dims, M, ns, B, seed=0):
    """Orthonormal complex states, unitary-sized axis matrices and surfaces of order one (the timing does not depend on
    the values)."""
    rng = np.random.default_rng(seed)
    npts = int(np.prod(dims))
    q, _ = np.linalg.qr(rng.standard_normal((npts, M, M)) + 1j * rng.standard_normal((npts, M, M)))
    U = np.ascontiguousarray(q[:, :, :ns]).reshape(tuple(dims) + (M, ns))
    apes = rng.random(tuple(dims) + (ns,))
    Ks = [np.linalg.qr(rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n)))[0] for n in dims]
    psi = rng.standard_normal((B,) + tuple(dims) + (ns,)) + 0j
    psi /= np.linalg.norm(psi.reshape(B, -1), axis=1).reshape((B,) + (1,) * (len(dims) + 1))
    return U, apes, Ks, psi


def torch_step_fn(torch, U, eV, eVh, Ks, psi0):
    """The factorised step in torch: expand, one einsum per axis, project."""
    nd = len(Ks)
    Uc = U.conj().resolve_conj()
    axis = ["ik,zk...->zi...", "jl,zil...->zij...", "ko,zijo...->zijk..."][:nd]

    def fn(steps):
        psi = psi0 * eVh
        for _ in range(steps):
            chi = torch.einsum("...mb,z...b->z...m", U, psi)
            for d in range(nd):
                chi = torch.einsum(axis[d], Ks[d], chi)
            psi = eV * torch.einsum("...ma,z...m->z...a", Uc, chi)
        return psi
    return fn


def time_call(torch, fn, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn(steps)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / steps


def measure_alternating(torch, fns, window, regions):
    """fns: {name: fn(steps)}.  Warm every path up, size its call to the window, then time the paths in turn, `regions`
    rounds."""
    steps = {}
    for name, fn in fns.items():
        fn(2)
        torch.cuda.synchronize()
        t = time_call(torch, fn, 4)
        steps[name] = int(min(max(window / max(t, 1e-9), 4), MAX_STEPS))
    ts = {name: [] for name in fns}
    for _ in range(regions):
        for name, fn in fns.items():
            ts[name].append(time_call(torch, fn, steps[name]))
    return steps, ts


def passes_of(dims, M, B):
    """(pass name, kernel template arguments, n_d, grid in workgroups) of the fused path, as ldr_plan.hpp plans it."""
    npts, out = int(np.prod(dims)), []
    for d, n in enumerate(dims):
        first, last = d == 0, d == len(dims) - 1
        cu = (SUB // M) * M if last else SUB
        C = B * npts * M // n
        out.append((("first" if first else "last" if last else "middle"), (first, last), n,
                    (-(-C // (NSUB * cu)), -(-n // RT))))
    return out


def summarise_passes(path, out):
    rows = list(csv.DictReader(open(path)))
    by = {}
    for r in rows:
        if "ldr_axis_kernel" not in r["Kernel_Name"]:
            continue
        targs = r["Kernel_Name"].split("<")[1].split(">")[0].replace(" ", "")
        key = (targs, int(r["Grid_Size_X"]), int(r["Grid_Size_Y"]))
        by.setdefault(key, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-9)
    lines = []
    for dims, M, ns in SHAPES:
        for B in BATCHES:
            for name, (first, last), n, grid in passes_of(dims, M, B):
                targs = f"{'true' if first else 'false'},{'true' if last else 'false'}"
                # grid sizes count work-items in a trace (workgroups, should a profiler report those)
                ts = by.get((targs, grid[0] * TPB, grid[1])) or by.get((targs, grid[0], grid[1]))
                if not ts:
                    continue
                elems = B * int(np.prod(dims)) * M
                t = float(np.median(ts))
                t_mfma, t_hbm = 8.0 * n * elems / PEAK_F64_MATRIX, 32.0 * elems / PEAK_HBM
                lines.append(json.dumps({
                    "bench": "ldr_pass", "dims": list(dims), "M": M, "ns": ns, "B": B, "pass": name, "n_d": n,
                    "dispatches": len(ts), "us": t * 1e6, "us_min": min(ts) * 1e6, "us_max": max(ts) * 1e6,
                    "bound": "mfma" if t_mfma > t_hbm else "hbm", "us_bound": max(t_mfma, t_hbm) * 1e6,
                    "fraction_of_bound": max(t_mfma, t_hbm) / t}))
    emit(lines, out)


def emit(lines, out):
    for line in lines:
        print(line, flush=True)
    if out and lines:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "a") as f:
            f.write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.3, help="seconds of work per timed region")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    ap.add_argument("--trace", action="store_true", help="kernel path only, a fixed number of steps per shape")
    ap.add_argument("--passes", default=None, help="summarise a kernel-trace CSV per pass instead of running")
    args = ap.parse_args()
    if args.passes:
        return summarise_passes(args.passes, args.out)
    import torch
    from pyqed_amd import ldr_run
    if not torch.cuda.is_available():
        raise SystemExit("bench_ldr needs a GPU: no timing is taken on a CPU")
    dev = torch.device("cuda", 0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=complex))).to(dev)   # noqa: E731
    dt = 0.01
    lines = []
    for dims, M, ns in SHAPES:
        for B in BATCHES:
            Uh, apes, Kh, psih = model(dims, M, ns, B)
            U, Ks, psi = t(Uh), [t(k) for k in Kh], t(psih)
            eV, eVh = t(np.exp(-1j * dt * apes)), t(np.exp(-0.5j * dt * apes))
            snap = torch.empty((B, 1) + tuple(dims) + (ns,), dtype=torch.complex128, device=dev)

            def kernel(steps):
                ldr_run(psi, U, None, Ks, dt, steps, steps, expV=eV, expVh=eVh, snap=snap)
            if args.trace:
                kernel(2)
                torch.cuda.synchronize()
                kernel(TRACE_STEPS)
                torch.cuda.synchronize()
                continue
            tfn = torch_step_fn(torch, U, eV, eVh, Ks, psi)
            # the two paths compute the same state
            kernel(3)
            diff = float((snap[:, 0] - tfn(3)).abs().max())
            fns = {"ldr_kernels": kernel, "torch_factorised": tfn}
            if (dims, M, ns) == DENSE and B == 1:
                u = U.reshape(-1, M, ns)
                A = torch.einsum("pma,qmb->paqb", u.conj(), u)
                Kf = torch.kron(Ks[0], Ks[1])
                expT = (A * Kf[:, None, :, None]).reshape(u.shape[0] * ns, -1).contiguous()
                del A, Kf

                def dense(steps, expT=expT):
                    v = (psi * eVh).reshape(B, -1).T.contiguous()
                    ev = eV.reshape(-1, 1)
                    for _ in range(steps):
                        v = ev * (expT @ v)
                    return v
                fns["torch_dense_expT"] = dense
            steps, ts = measure_alternating(torch, fns, args.window, args.regions)
            spread = {k: max(v) - min(v) for k, v in ts.items()}
            for name, v in ts.items():
                rec = {"bench": "ldr", "dims": list(dims), "M": M, "ns": ns, "B": B, "D": int(np.prod(dims)) * ns,
                       "path": name, "steps": steps[name], "regions": args.regions,
                       "us_per_step": float(np.median(v)) * 1e6, "us_per_step_min": min(v) * 1e6,
                       "us_per_step_max": max(v) * 1e6, "max_abs_diff_paths": diff}
                if name == "ldr_kernels":
                    other = ts["torch_factorised"]
                    rec["vs_torch"] = float(np.median(other) / np.median(v))
                    rec["faster"] = bool(np.median(other) - np.median(v) >
                                         spread["ldr_kernels"] + spread["torch_factorised"])
                lines.append(json.dumps(rec))
                print(lines[-1], flush=True)
            fns.clear()
            torch.cuda.empty_cache()
    if args.out and lines:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
