"""Time per RK4 step of the three-dimensional curvilinear (3 x 3 G-matrix) propagator, qd_wp3_gmat_rk4 /
qd_wp3_gmat_ms_rk4, beside the same step written with torch.fft and tensor ops on the same GPU (what a user could do
before the kernels existed; it is not tuned).

    python tools/wp_gmat3_bench.py [--sizes 32 64 128] [--ns 1 2] [--out FILE] [--limit SECONDS]

Every (n^3 grid, ns) configuration, B = 1, is measured in a child process of its own under a time limit (--limit,
default 300 s); the parent never opens the GPU.  A child that fails, faults or runs out of time ends the whole run
there: nothing more is started on the device.

Per configuration: HIP-event time of a region of `steps` RK4 steps, the median of --regions timed regions after a
warm-up region, with min and max as the spread; steps is chosen from one probe region so that a region lasts about
--target-ms.  One JSON line per configuration: both medians, their ratio, the bytes per point and step the four-pass
design moves and the share of the 8 TB/s HBM peak that gives.  Per stage and plane point (wp_gmat3.hip):
    X   reads y, D_y y, D_z y (48 B) and G (72 B), writes u, phi_y, phi_z (48 B)             168 B
    Y   reads phi_y and u, writes u                                                            48 B
    Z   reads phi_z, u, y, psi, v, writes y' and D_z y'                                       112 B
    Y'  reads y', writes D_y y'                                                                32 B
360 B, and on ns coupled surfaces 32 (ns - 1) more in Z (the other planes of y and of V).
The torch yardstick is checked against the numpy restatement of tests/gmat3_models.py first, and at every
configuration one step of the kernels must agree with one step of the yardstick to the suite's bound for a one-step
run on white noise (tests/test_gmat3_gpu.py: 24 fft_cases.tol(n)); a miss ends the run with an error, so a benchmark
run is also a check at the benchmark's shapes.
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
import gmat3_models as g3  # noqa: E402
from pyqed_amd import _lib  # noqa: E402

HBM_PEAK = 8.0e12


def agree_tol(n):
    """One RK4 step, kernels against the torch yardstick: the suite's run bound at nt = 1."""
    return 24.0 * fc.tol(n)


def bytes_per_point_step(ns):
    """Design bytes per grid point and step over the ns planes of a member."""
    return 4 * (360 * ns + 32 * ns * (ns - 1))


def torch_step(psi, dt, ks, G, V):
    """One Horner RK4 step of psi [B, ns, nx, ny, nz] on V [ns, ns, nx, ny, nz] in the separable form, eager torch."""
    shapes = [(-1, 1, 1), (-1, 1), (-1,)]
    kk = [k.reshape(s) for k, s in zip(ks, shapes)]

    def d(f, a):
        return torch.fft.ifft(kk[a] * torch.fft.fft(f, dim=a - 3), dim=a - 3)

    def H(y):
        g = [d(y, a) for a in range(3)]
        phi = [G[..., r, 0] * g[0] + G[..., r, 1] * g[1] + G[..., r, 2] * g[2] for r in range(3)]
        return 0.5 * (d(phi[0], 0) + d(phi[1], 1) + d(phi[2], 2)) + torch.einsum("abxyz,kbxyz->kaxyz", V, y)
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


def measure(n, ns, regions, target_ms):
    """One configuration, in this process: the JSON record."""
    if not torch.cuda.is_available():
        raise SystemExit("wp_gmat3_bench: needs a GPU")
    dev = torch.device("cuda", 0)
    _lib.ensure_device(dev)
    lib = _lib.load()
    t = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x, dtype=dt)).to(dev)
    planes = lambda m: (t(np.moveaxis(m["V"], (-2, -1), (0, 1)), complex),
                        np.moveaxis(m["psi0"].reshape(m["G"].shape[:3] + (-1,)), -1, 0)[None])

    # the yardstick against the restatement
    for cs in (1, 2):
        m = g3.model3(12, 10, 7, ns=cs)
        V, p0 = planes(m)
        got = torch_step(t(p0, complex), m["dt"], [t(k, float) for k in m["ks"]], t(m["G"], float), V).cpu().numpy()[0]
        ref = g3.run_ref(m["psi0"], m["dt"], 1, m["ks"], m["V"] if cs > 1 else m["v"], m["G"])[0]
        ref = np.moveaxis(ref.reshape(got.shape[1:] + (-1,)), -1, 0)
        err = float(np.linalg.norm(got - ref) / np.linalg.norm(ref))
        if not err < 1e-12:
            raise SystemExit(f"wp_gmat3_bench: the torch yardstick (ns = {cs}) differs from the restatement, "
                             f"rel err {err:.3e}")

    m = g3.model3(n, n, n, ns=ns)
    G, ks = t(m["G"], float), [t(k, float) for k in m["ks"]]
    V, _ = planes(m)
    rng = np.random.default_rng(n + ns)
    psi0 = t(rng.standard_normal((1, ns, n, n, n)) + 1j * rng.standard_normal((1, ns, n, n, n)), complex)
    psi0 /= torch.linalg.norm(psi0)
    dt = float(m["dt"])
    state = {"k": psi0.clone(), "b": psi0.clone()}

    def run_kernel(steps):
        if ns == 1:
            _lib.check(lib.qd_wp3_gmat_rk4(state["k"].data_ptr(), 1, G.data_ptr(), V.data_ptr(),
                                           *(k.data_ptr() for k in ks), n, n, n, dt, steps, 1, None,
                                           _lib.stream_ptr(dev)), "qd_wp3_gmat_rk4")
        else:
            _lib.check(lib.qd_wp3_gmat_ms_rk4(state["k"].data_ptr(), 1, ns, G.data_ptr(), V.data_ptr(),
                                              *(k.data_ptr() for k in ks), n, n, n, dt, steps, 1, None,
                                              _lib.stream_ptr(dev)), "qd_wp3_gmat_ms_rk4")

    def run_torch(steps):
        for _ in range(steps):
            state["b"] = torch_step(state["b"], dt, ks, G, V)

    _lib.take_path()
    run_kernel(1)
    run_torch(1)
    torch.cuda.synchronize()
    path = _lib.take_path()
    agree = float(torch.linalg.norm(state["k"] - state["b"]) / torch.linalg.norm(state["b"]))
    if not agree <= agree_tol(n):
        raise SystemExit(f"wp_gmat3_bench: {n}^3, ns = {ns} ({path}): one step of the kernels differs from the torch "
                         f"yardstick by {agree:.3e}, bound {agree_tol(n):.3e}")
    kr = summary(time_regions(run_kernel, pick_steps(run_kernel, target_ms), regions))
    br = summary(time_regions(run_torch, pick_steps(run_torch, target_ms), regions))
    per_step = bytes_per_point_step(ns)
    return {"n": n, "ns": ns, "B": 1, "path": path, "kernel": kr, "torch_yardstick": br,
            "speedup_median": br["median_us"] / kr["median_us"], "one_step_rel_diff": agree,
            "one_step_bound": agree_tol(n), "design_bytes_per_point_step": per_step,
            "hbm_peak_fraction": per_step * n ** 3 / (kr["median_us"] * 1e-6) / HBM_PEAK}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[32, 64, 128])
    ap.add_argument("--ns", type=int, nargs="+", default=[1, 2])
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--target-ms", type=float, default=200.0)
    ap.add_argument("--limit", type=float, default=300.0, help="seconds a configuration's child process may take")
    ap.add_argument("--out", default=None)
    ap.add_argument("--one", action="store_true", help="measure the single given configuration in this process")
    a = ap.parse_args()
    if a.one:
        print(json.dumps(measure(a.sizes[0], a.ns[0], a.regions, a.target_ms)), flush=True)
        return

    lines = []
    for n in a.sizes:
        for ns in a.ns:
            what = f"{n}^3, ns = {ns}"
            cmd = [sys.executable, os.path.abspath(__file__), "--one", "--sizes", str(n), "--ns", str(ns),
                   "--regions", str(a.regions), "--target-ms", str(a.target_ms)]
            try:
                r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=a.limit)
            except subprocess.TimeoutExpired:
                raise SystemExit(f"wp_gmat3_bench: {what} ran past {a.limit:.0f} s; stopping")
            if r.returncode != 0:
                raise SystemExit(f"wp_gmat3_bench: {what} ended with status {r.returncode}; stopping")
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
