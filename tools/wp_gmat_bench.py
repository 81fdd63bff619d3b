"""Time per RK4 step of the curvilinear (G-matrix) wavepacket propagator, qd_wp2_gmat_rk4, beside the same
arithmetic written with torch.fft and tensor ops on the same GPU (what a user could do before the kernels existed).

    python tools/wp_gmat_bench.py --sizes 64 256 1024 200 --batches 1 64 [--out FILE] [--limit SECONDS]

Every (size, batch) configuration is measured in a child process of its own under a time limit (--limit, default
300 s); the parent never opens the GPU.  A child that fails, faults or runs out of time ends the whole run there:
nothing more is started on the device.

Per (n x n grid, batch B): HIP-event time of a region of `steps` RK4 steps, the median of --regions timed regions
after a warm-up region, with min and max as the spread; steps is chosen from one probe region so that a region lasts
about --target-ms.  One JSON line per configuration: both medians, their ratio, the bytes per point per step the
two-launch design moves (832 B: per stage the column pass reads y, D_y y (16 B each) and G (32 B) and writes u,
phi_y; the row pass reads phi_y, u, y, psi, v and writes y', D_y y') and the share of the 8 TB/s HBM peak that gives.
The torch baseline is checked against the numpy restatement of tests/gmat_models.py; it is not tuned.  At every
configuration one step of the kernels must agree with one step of the baseline to AGREE_TOL in relative L2 norm, the
suite's bound for one step on white noise (tests/test_gmat_gpu.py: 20 fft_cases.tol(n)); a miss ends the run with an
error, so a benchmark run is also a check at the benchmark's shapes.

    python tools/wp_gmat_bench.py --ns 2 3 --sizes 64 256 1024 [--batches 1]

times the coupled-surface run, qd_wp2_gmat_ms_rk4 on B members of ns states, beside its yardstick: qd_wp2_gmat_rk4 on
B ns uncoupled single-surface members of the same grid, which moves the same state without the coupling.  The design
bytes per point, stage and member are 208 ns + 16 ns (ns - 1) (the other planes of y) + 16 ns (ns - 1) (V in place of
v) against 208 ns: a predicted ratio of 1.15 at ns = 2 and 1.31 at ns = 3.  One step is checked against the torch
baseline with the potential as an einsum, to the same bound.
Needs a GPU: there is no fallback."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import fft_cases as fc  # noqa: E402
import gmat_models as gm  # noqa: E402
from pyqed_amd import _lib  # noqa: E402

BYTES_PER_POINT_STEP = 4 * (6 * 16 + 7 * 16)   # 4 stages x (column pass 96 B + row pass 112 B) = 832
HBM_PEAK = 8.0e12


def agree_tol(n):
    """One RK4 step, kernels against the torch baseline: four stages of five transform-sized errors each."""
    return 20.0 * fc.tol(n)


def ms_bytes_per_point_stage(ns):
    """Design bytes per grid point and stage over the ns planes of a member (wp_gmat.hip)."""
    return 208 * ns + 32 * ns * (ns - 1)


def torch_step(psi, dt, kx, ky, G, v):
    """One Horner RK4 step of i dpsi/dt = (K + v) psi in the separable form, eager torch.  v [n, n], or
    [ns, ns, n, n] with psi [B, ns, n, n] (coupled surfaces)."""
    def dxf(f):
        return torch.fft.ifft(kx[:, None] * torch.fft.fft(f, dim=-2), dim=-2)

    def dyf(f):
        return torch.fft.ifft(ky * torch.fft.fft(f, dim=-1), dim=-1)

    def H(y):
        a, b = dxf(y), dyf(y)
        px = G[..., 0, 0] * a + G[..., 0, 1] * b
        py = G[..., 1, 0] * a + G[..., 1, 1] * b
        vy = v * y if v.dim() == 2 else torch.einsum("abij,kbij->kaij", v, y)
        return 0.5 * (dxf(px) + dyf(py)) + vy
    y = psi
    for c in (dt / 4, dt / 3, dt / 2, dt):
        y = psi - 1j * c * H(y)
    return y


def time_regions(run, steps, regions):
    """ms per step of each of `regions` timed regions of `steps` steps, after one warm-up region."""
    run(steps)
    torch.cuda.synchronize()
    out = []
    for _ in range(regions):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run(steps)
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) / steps)
    return out


def pick_steps(run, target_ms):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    run(2)
    torch.cuda.synchronize()
    e0.record()
    run(4)
    e1.record()
    e1.synchronize()
    per = max(e0.elapsed_time(e1) / 4, 1e-3)
    return int(min(2000, max(4, target_ms / per)))


def summary(ms):
    return {"median_us": 1e3 * statistics.median(ms), "min_us": 1e3 * min(ms), "max_us": 1e3 * max(ms)}


def measure(n, B, regions, target_ms):
    """One configuration, in this process: the JSON record."""
    if not torch.cuda.is_available():
        raise SystemExit("wp_gmat_bench: needs a GPU")
    dev = torch.device("cuda", 0)
    _lib.ensure_device(dev)
    lib = _lib.load()
    t = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x, dtype=dt)).to(dev)

    # the baseline against the restatement
    m = gm.model(24, 20)
    got = torch_step(t(m["psi0"], complex), m["dt"], t(m["kx"], float), t(m["ky"], float), t(m["G"], float),
                     t(m["v"], complex)).cpu().numpy()
    ref = gm.run_ref(m["psi0"], m["dt"], 1, m["kx"], m["ky"], m["v"], m["G"])[0]
    err = float(np.linalg.norm(got - ref) / np.linalg.norm(ref))
    if not err < 1e-12:
        raise SystemExit(f"wp_gmat_bench: the torch baseline differs from the restatement, rel err {err:.3e}")

    m = gm.model(n, n)
    G, v, kx, ky = t(m["G"], float), t(m["v"], complex), t(m["kx"], float), t(m["ky"], float)
    rng = np.random.default_rng(n + B)
    psi0 = t(rng.standard_normal((B, n, n)) + 1j * rng.standard_normal((B, n, n)), complex)
    psi0 /= torch.linalg.norm(psi0)
    dt = float(m["dt"])
    state = {"k": psi0.clone(), "b": psi0.clone()}

    def run_kernel(steps):
        _lib.check(lib.qd_wp2_gmat_rk4(state["k"].data_ptr(), B, G.data_ptr(), v.data_ptr(), kx.data_ptr(),
                                       ky.data_ptr(), n, n, dt, steps, 1, None, _lib.stream_ptr(dev)),
                   "qd_wp2_gmat_rk4")

    def run_torch(steps):
        for _ in range(steps):
            state["b"] = torch_step(state["b"], dt, kx, ky, G, v)

    _lib.take_path()
    run_kernel(1)
    run_torch(1)
    torch.cuda.synchronize()
    path = _lib.take_path()
    agree = float(torch.linalg.norm(state["k"] - state["b"]) / torch.linalg.norm(state["b"]))
    if not agree <= agree_tol(n):
        raise SystemExit(f"wp_gmat_bench: {n} x {n}, B = {B} ({path}): one step of the kernels differs from the "
                         f"torch baseline by {agree:.3e}, bound {agree_tol(n):.3e}")
    ks = summary(time_regions(run_kernel, pick_steps(run_kernel, target_ms), regions))
    bs = summary(time_regions(run_torch, pick_steps(run_torch, target_ms), regions))
    pts = B * n * n
    return {"n": n, "B": B, "path": path, "kernel": ks, "torch_baseline": bs,
            "speedup_median": bs["median_us"] / ks["median_us"], "one_step_rel_diff": agree,
            "one_step_bound": agree_tol(n), "design_bytes_per_point_step": BYTES_PER_POINT_STEP,
            "hbm_peak_fraction": BYTES_PER_POINT_STEP * pts / (ks["median_us"] * 1e-6) / HBM_PEAK}


def measure_ms(n, ns, B, regions, target_ms):
    """One coupled-surface configuration, in this process: qd_wp2_gmat_ms_rk4 on B members of ns states beside
    qd_wp2_gmat_rk4 on B ns uncoupled members."""
    import gmat_ms_models as gms
    if not torch.cuda.is_available():
        raise SystemExit("wp_gmat_bench: needs a GPU")
    dev = torch.device("cuda", 0)
    _lib.ensure_device(dev)
    lib = _lib.load()
    t = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x, dtype=dt)).to(dev)
    m = gms.model_ms(n, n, ns)
    G, kx, ky = t(m["G"], float), t(m["kx"], float), t(m["ky"], float)
    V, v = t(m["V"].transpose(2, 3, 0, 1), complex), t(m["v"], complex)   # planes [ns][ns][n][n]
    rng = np.random.default_rng(n + B + ns)
    psi0 = t(rng.standard_normal((B, ns, n, n)) + 1j * rng.standard_normal((B, ns, n, n)), complex)
    psi0 /= torch.linalg.norm(psi0)
    dt = float(m["dt"])
    state = {"ms": psi0.clone(), "one": psi0.clone()}

    def run_ms(steps):
        _lib.check(lib.qd_wp2_gmat_ms_rk4(state["ms"].data_ptr(), B, ns, G.data_ptr(), V.data_ptr(), kx.data_ptr(),
                                          ky.data_ptr(), n, n, dt, steps, 1, None, _lib.stream_ptr(dev)),
                   "qd_wp2_gmat_ms_rk4")

    def run_one(steps):
        _lib.check(lib.qd_wp2_gmat_rk4(state["one"].data_ptr(), B * ns, G.data_ptr(), v.data_ptr(), kx.data_ptr(),
                                       ky.data_ptr(), n, n, dt, steps, 1, None, _lib.stream_ptr(dev)),
                   "qd_wp2_gmat_rk4")

    _lib.take_path()
    run_ms(1)
    want = torch_step(psi0, dt, kx, ky, G, V)
    torch.cuda.synchronize()
    path = _lib.take_path()
    agree = float(torch.linalg.norm(state["ms"] - want) / torch.linalg.norm(want))
    if not agree <= agree_tol(n):
        raise SystemExit(f"wp_gmat_bench: {n} x {n}, ns = {ns}, B = {B} ({path}): one step of the kernels differs from "
                         f"the torch baseline by {agree:.3e}, bound {agree_tol(n):.3e}")
    ms = summary(time_regions(run_ms, pick_steps(run_ms, target_ms), regions))
    one = summary(time_regions(run_one, pick_steps(run_one, target_ms), regions))
    per_step = 4 * ms_bytes_per_point_stage(ns)
    return {"n": n, "ns": ns, "B": B, "path": path, "multi_state": ms, "uncoupled_members": one,
            "ratio_median": ms["median_us"] / one["median_us"],
            "predicted_ratio": ms_bytes_per_point_stage(ns) / (208.0 * ns), "one_step_rel_diff": agree,
            "one_step_bound": agree_tol(n), "design_bytes_per_point_step": per_step,
            "hbm_peak_fraction": per_step * B * n * n / (ms["median_us"] * 1e-6) / HBM_PEAK}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[64, 256, 1024, 200])
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 64])
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--target-ms", type=float, default=200.0)
    ap.add_argument("--limit", type=float, default=300.0, help="seconds a configuration's child process may take")
    ap.add_argument("--out", default=None)
    ap.add_argument("--ns", type=int, nargs="+", default=None,
                    help="time the coupled-surface run on this many states beside B ns uncoupled members "
                         "(default sizes 64 256 1024, batch 1)")
    ap.add_argument("--one", action="store_true", help="measure the single given configuration in this process")
    a = ap.parse_args()
    if a.one:
        rec = measure_ms(a.sizes[0], a.ns[0], a.batches[0], a.regions, a.target_ms) if a.ns else \
            measure(a.sizes[0], a.batches[0], a.regions, a.target_ms)
        print(json.dumps(rec), flush=True)
        return
    if a.ns and "--sizes" not in sys.argv:
        a.sizes = [64, 256, 1024]
    if a.ns and "--batches" not in sys.argv:
        a.batches = [1]

    lines = []
    for n in a.sizes:
        for B, ns in [(B, ns) for ns in (a.ns or [None]) for B in a.batches]:
            what = f"{n} x {n}, B = {B}" + (f", ns = {ns}" if ns else "")
            cmd = [sys.executable, os.path.abspath(__file__), "--one", "--sizes", str(n), "--batches", str(B),
                   "--regions", str(a.regions), "--target-ms", str(a.target_ms)] + (["--ns", str(ns)] if ns else [])
            try:
                r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=a.limit)
            except subprocess.TimeoutExpired:
                raise SystemExit(f"wp_gmat_bench: {what} ran past {a.limit:.0f} s; stopping")
            if r.returncode != 0:
                raise SystemExit(f"wp_gmat_bench: {what} ended with status {r.returncode}; stopping")
            rec = json.loads(r.stdout.strip().splitlines()[-1])
            print(json.dumps(rec), flush=True)
            lines.append(rec)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
