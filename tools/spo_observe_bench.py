#!/usr/bin/env python
"""Cost of recording SPO2 observables inside the run (SPO observables) at the bench shape 256 x 256 x 2.

  (a) per-step time of the plain qd_spo2_run with snap = NULL, on this build and, with --parent-lib, on a libqdyn.so
      built from the parent commit (the run loop is shared with the observed entry point);
  (b) per-step time of qd_spo2_run_observed without snapshots at nout = 10 and nout = 1, diabatic and adiabatic;
  (c) the route without it: snapshots of every recorded step, copied to the host and reduced in numpy.

Device events around --steps steps per sample after a warm-up call; the variants are interleaved sample by sample and
the median, minimum and maximum over --repeats samples are reported, one JSON object per line.

    python tools/spo_observe_bench.py [--parent-lib PATH] [--steps 2000] [--repeats 7] [--out FILE]
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def model(n):
    x = np.linspace(-6, 6, n)
    X, Y = np.meshgrid(x, x, indexing="ij")
    surfaces = [0.5 * ((X + 1) ** 2 + Y ** 2), 0.5 * ((X - 1) ** 2 + Y ** 2) + 0.1]
    psi0 = np.zeros((n, n, 2), complex)
    psi0[:, :, 0] = np.exp(-((X + 1.5) ** 2 + Y ** 2) / 2 + 0.5j * X) / np.sqrt(np.pi)
    return x, surfaces, [[[0, 1], 0.2 * X]], psi0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parent-lib", default=None, help="libqdyn.so of the parent commit for (a)")
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--host-steps", type=int, default=200, help="recorded steps of the host route (c)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    from pyqed_amd import SPO2, _lib
    from pyqed_amd.wpd import _dev_c128, _dev_f64
    if not torch.cuda.is_available():
        raise SystemExit("spo_observe_bench: needs the GPU (no timing without one)")
    dev = torch.device("cuda", 0)
    _lib.ensure_device(dev)
    lib = _lib.load()
    n, ns = args.n, 2
    x, surfaces, couplings, psi0 = model(n)
    sol = SPO2(x, x, mass=[1.0, 1.0], nstates=ns)
    sol.set_DPES(surfaces, couplings)
    sol.build(0.05)
    _, eVh = sol._point_ops_dev(dev)
    eK = _dev_c128(sol.exp_K, dev)
    d2a = _dev_c128(sol.d2a, dev)
    xd = _dev_f64(x, dev)
    w = float((x[1] - x[0]) ** 2)
    st = _lib.stream_ptr(dev)
    psi_init = _dev_c128(psi0, dev)

    parent = None
    if args.parent_lib:
        parent = ctypes.CDLL(os.path.abspath(args.parent_lib))
        for name in ("qd_init", "qd_spo2_run"):
            fn = getattr(parent, name)
            fn.restype, fn.argtypes = _lib.SIGNATURES[name]
        _lib.check(parent.qd_init(0), "parent qd_init")

    def plain(which):
        def call(psi, steps):
            rc = which.qd_spo2_run(psi.data_ptr(), eVh.data_ptr(), eK.data_ptr(), n, n, ns, steps, steps, None, st)
            assert rc == 0, rc
        return call

    def observed(nout, basis):
        def call(psi, steps):
            nrec = max(steps // nout, 1)
            rdm = torch.empty((nrec, ns, ns), dtype=torch.complex128, device=dev)
            mom = torch.empty((nrec, 2, ns), dtype=torch.float64, device=dev)
            rc = lib.qd_spo2_run_observed(psi.data_ptr(), 1, eVh.data_ptr(), eK.data_ptr(), None, n, n, ns, steps, nout,
                                          None, _lib.ptr(basis), xd.data_ptr(), xd.data_ptr(), w, rdm.data_ptr(),
                                          mom.data_ptr(), st)
            _lib.check(rc, "qd_spo2_run_observed")
            call.keep = (rdm, mom)   # alive until the events have been read
        return call

    variants = {"plain_branch": plain(lib)}
    if parent is not None:
        variants["plain_parent"] = plain(parent)
    variants.update({"observed_nout10_diabatic": observed(10, None), "observed_nout1_diabatic": observed(1, None),
                     "observed_nout10_adiabatic": observed(10, d2a), "observed_nout1_adiabatic": observed(1, d2a)})

    def sample(call):
        psi = psi_init.clone()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call(psi, args.steps)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / args.steps   # us per step

    for call in variants.values():   # warm-up: code objects, scratch slabs
        call(psi_init.clone(), 20)
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(args.repeats):
        for k, call in variants.items():
            times[k].append(sample(call))
    lines = []
    for k, v in times.items():
        lines.append({"what": k, "n": n, "ns": ns, "steps": args.steps, "repeats": args.repeats,
                      "us_per_step_median": float(np.median(v)), "us_per_step_min": float(min(v)),
                      "us_per_step_max": float(max(v))})

    # (c) snapshots of every step, copied to the host, populations and <x>, <y> in numpy (the route of
    # run(return_states=True) + ResultSPO2.get_population / position)
    hs = args.host_steps
    snap = torch.empty((hs, n, n, ns), dtype=torch.complex128, device=dev)
    for rep in range(2):   # the second pass is the warm one
        psi = psi_init.clone()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rc = lib.qd_spo2_run(psi.data_ptr(), eVh.data_ptr(), eK.data_ptr(), n, n, ns, hs, 1, snap.data_ptr(), st)
        assert rc == 0, rc
        host = snap.cpu().numpy()
        t1 = time.perf_counter()
        dens = np.abs(host) ** 2
        pop = dens.sum(axis=(1, 2)) * w
        xa = np.einsum('kijn,i->k', dens, x) * w
        ya = np.einsum('kijn,j->k', dens, x) * w
        t2 = time.perf_counter()
    lines.append({"what": "host_route_nout1", "n": n, "ns": ns, "recorded_steps": hs,
                  "us_per_step_run_and_copy": (t1 - t0) * 1e6 / hs, "us_per_step_numpy": (t2 - t1) * 1e6 / hs,
                  "snapshot_MiB": snap.numel() * 16 / 2 ** 20})
    text = "\n".join(json.dumps(l) for l in lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
