"""Times the sum-over-states echo GSB + SE + ESA two ways on the same inputs: through the factorised pathways
(qd_sos_pathway, csrc/sos_signals.hip) and through the per-point kernel qd_photon_echo (csrc/sos.hip), and, alone,
TPA2D (qd_sos_tpa) and the t3 echo (SE_T3 + ESA_T3 accumulated, as sos.photon_echo_t3 calls them).

    python tools/bench_sos.py [--states 16 64 128] [--grid 256] [--out profiles/sos/bench_sos.json]

Method: inputs live on the device; a region is `calls` back-to-back library calls between two device events; every shape
is warmed up first; the two echo paths alternate region by region; the median over the regions is reported with their
minimum and maximum.  `calls` is chosen per shape and path so that a region lasts about --region-ms.  The outputs of the
two echo paths are compared at every size timed.  Operation counts come from the shapes (count_* below), not from a
measurement.  Needs the GPU: there is no fallback."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pyqed_amd import _lib  # noqa: E402

GSB, SE, ESA, SE_T3, ESA_T3 = 0, 1, 2, 3, 4


def model(N, seed=0):
    rng = np.random.default_rng(seed)
    E = np.concatenate([[0.0], np.sort(rng.uniform(0.8, 2.6, N - 1))])
    d = rng.standard_normal((N, N)) + 1j * rng.standard_normal((N, N))
    return E.astype(complex), (d + d.conj().T) / 2, rng.uniform(0.02, 0.2, N)


def count_per_point(ng, ne, nf):
    """Complex divisions per grid point of qd_photon_echo: one Green's function per (b), per (b, d) of GSB and per
    (b, c, d) of SE and ESA."""
    return ne + ne * ne + ne * ne * (ng + nf)


def count_factorised(ng, ne, nf, n1, n3):
    """(reciprocals of the inner passes, reciprocals of the outer passes, complex multiply-adds of the outer passes,
    exponentials of the build passes) of GSB + SE + ESA through qd_sos_pathway."""
    inner = (ne * ne + ne * ne * ng + ne * nf) * n3
    tiles_y = -(-n3 // 16)
    outer_recip = 3 * ne * n1 * tiles_y
    outer_mac = 3 * ne * n1 * n3
    build_exp = ne * ne * ng + ne * nf * ne
    return inner, outer_recip, outer_mac, build_exp


def regions(fn, stream_sync, target_ms, nreg, max_calls=4096):
    """Median / min / max milliseconds per call over nreg regions of `calls` calls; the first region is a warm-up."""
    ev = lambda: torch.cuda.Event(enable_timing=True)

    def region(calls):
        a, b = ev(), ev()
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        stream_sync()
        return a.elapsed_time(b) / calls
    fn()
    stream_sync()
    one = region(1)
    calls = int(min(max_calls, max(1, round(target_ms / max(one, 1e-3)))))
    region(calls)
    return calls, [region(calls) for _ in range(nreg)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--states", type=int, nargs="+", default=[16, 64, 128])
    ap.add_argument("--grid", type=int, default=256)
    ap.add_argument("--regions", type=int, default=7)
    ap.add_argument("--region-ms", type=float, default=100.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_sos needs the GPU; there is no CPU fallback")
    dev = torch.device("cuda", 0)
    _lib.ensure_device(dev)
    lib = _lib.load()
    sync = torch.cuda.synchronize
    st = _lib.stream_ptr(dev)
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=dt))).to(dev)
    n = args.grid
    rows = []
    for N in args.states:
        E, dip, gamma = model(N)
        Et, Dt, Gt = up(E, complex), up(dip, complex), up(gamma, float)
        g, e, f = [0], list(range(N)), list(range(N))   # Mol.photon_echo's defaults
        gi, ei, fi = up(g, np.int32), up(e, np.int32), up(f, np.int32)
        w1 = np.linspace(-2.8, -0.6, n)
        w3 = np.linspace(0.6, 2.8, n)
        pump, x1, x3 = up(-w1, float), up(w1, float), up(w3, float)
        t2 = 1.3
        S_old = torch.empty((n, n), dtype=torch.complex128, device=dev)
        S_new = torch.empty((n, n), dtype=torch.complex128, device=dev)

        def old():
            _lib.check(lib.qd_photon_echo(Et.data_ptr(), Dt.data_ptr(), Gt.data_ptr(), N, gi.data_ptr(), 1,
                                          ei.data_ptr(), N, fi.data_ptr(), N, pump.data_ptr(), n, x3.data_ptr(), n, t2,
                                          S_old.data_ptr(), st), "qd_photon_echo")

        def pathway(p, out, acc, deph=0.0):
            _lib.check(lib.qd_sos_pathway(p, Et.data_ptr(), Dt.data_ptr(), Gt.data_ptr(), N, deph, gi.data_ptr(), 1,
                                          ei.data_ptr(), N, fi.data_ptr(), N, t2, x1.data_ptr(), n, x3.data_ptr(), n,
                                          out.data_ptr(), acc, st), "qd_sos_pathway")

        def new():
            pathway(GSB, S_new, 0)
            pathway(SE, S_new, 1)
            pathway(ESA, S_new, 1)

        def echo_t3():
            pathway(SE_T3, S_t3, 0, 0.03)
            pathway(ESA_T3, S_t3, 1, 0.03)
        S_t3 = torch.empty((n, n), dtype=torch.complex128, device=dev)
        Er = up(E.real, float)
        tpa_out = torch.empty((n, n), dtype=torch.float64, device=dev)

        def tpa():
            _lib.check(lib.qd_sos_tpa(Er.data_ptr(), Dt.data_ptr(), Gt.data_ptr(), N, ei.data_ptr(), N, fi.data_ptr(), N,
                                      x3.data_ptr(), n, x3.data_ptr(), n, 1, tpa_out.data_ptr(), st), "qd_sos_tpa")
        # alternate the two echo paths region by region
        c_old, _ = regions(old, sync, args.region_ms, 0)
        c_new, _ = regions(new, sync, args.region_ms, 0)
        t_old, t_new = [], []
        for _ in range(args.regions):
            t_old += _timed(old, c_old, sync)
            t_new += _timed(new, c_new, sync)
        a, b = S_old.cpu().numpy(), S_new.cpu().numpy()
        diff = float(np.linalg.norm(b - a) / np.linalg.norm(a))
        c_t3, t_t3 = regions(echo_t3, sync, args.region_ms, args.regions)
        c_tpa, t_tpa = regions(tpa, sync, args.region_ms, args.regions)
        inner, orec, omac, bexp = count_factorised(1, N, N, n, n)
        row = {
            "states": N, "grid": [n, n], "g_e_f": [1, N, N],
            "photon_echo_kernel_ms": _stats(t_old, c_old), "factorised_ms": _stats(t_new, c_new),
            "speedup_median": statistics.median(t_old) / statistics.median(t_new),
            "relerr_factorised_vs_kernel": diff,
            "count_divisions_per_point_kernel": count_per_point(1, N, N),
            "count_divisions_kernel": count_per_point(1, N, N) * n * n,
            "count_factorised": {"inner_reciprocals": inner, "outer_reciprocals": orec, "outer_macs": omac,
                                 "build_exponentials": bexp},
            "photon_echo_t3_ms": _stats(t_t3, c_t3), "tpa2d_ms": _stats(t_tpa, c_tpa),
            "count_tpa_divisions": 2 * N * N * n * n,
        }
        rows.append(row)
        print(json.dumps(row), flush=True)
    out = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "regions": args.regions,
           "region_ms_target": args.region_ms, "results": rows}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)
        print("wrote", args.out)


def _timed(fn, calls, sync):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    sync()
    return [a.elapsed_time(b) / calls]


def _stats(ts, calls):
    return {"median": statistics.median(ts), "min": min(ts), "max": max(ts), "calls_per_region": calls,
            "regions": len(ts)}


if __name__ == "__main__":
    main()
