"""bench.py's stdout contract, on CPU: the compact JSON line built from a recorded full-bench detail file
(profiles/r04/bench_r04f_detail.json, the driver's own command on one MI355X) carries every key the driver parses,
the headline's roofline and cpu_baseline, the 2DES half of BASELINE's metric, and stays short enough for the
driver's stdout tail."""
import json
import os
import sys

from conftest import ROOT

sys.path.insert(0, ROOT)


def test_dump_outputs_full_batch_and_seeded_sample(tmp_path):
    """bench.dump_outputs: float64 (re, im) of the states; a batch over DUMP_MAX_BYTES is cut to the same seeded
    sample of its matrices on every call, whose indices are written beside it."""
    import numpy as np
    import torch
    import bench
    N = 32
    keep = bench.DUMP_MAX_BYTES // (N * N * 16)
    rng = np.random.default_rng(0)
    for B in (3, keep + 5):
        rho = rng.standard_normal((B, N, N)) + 1j * rng.standard_normal((B, N, N))
        for d in ("a", "b"):
            bench.dump_outputs(torch.from_numpy(rho), str(tmp_path / f"{B}{d}"))
        x, idx = np.load(tmp_path / f"{B}a" / "rho.npy"), np.load(tmp_path / f"{B}a" / "rho_index.npy")
        assert x.dtype == np.float64 and idx.dtype == np.float64
        assert x.shape == (min(B, keep), N, N, 2) and x.nbytes <= bench.DUMP_MAX_BYTES <= 64e6
        assert np.array_equal(idx, np.arange(B)) if B <= keep else len(np.unique(idx)) == keep
        assert np.array_equal(x[..., 0] + 1j * x[..., 1], rho[idx.astype(int)])
        assert np.array_equal(idx, np.load(tmp_path / f"{B}b" / "rho_index.npy"))
        assert np.array_equal(x, np.load(tmp_path / f"{B}b" / "rho.npy"))


def test_compact_line_keys_and_length():
    import bench
    out = json.load(open(os.path.join(ROOT, "profiles", "r04", "bench_r04f_detail.json")))
    line = bench.compact_line(out, "gpurun_out/bench_detail.json")
    s = json.dumps(line)
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline", "twodes"):
        assert k in line, k
    assert line["metric"] == json.load(open(os.path.join(ROOT, "BASELINE.json")))["metric"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert k in line["roofline"], k
    for k in ("value", "unit", "cores", "kind", "sample"):
        assert k in line["cpu_baseline"], k
    tw = line["twodes"]
    assert tw["value"] > 0 and "roofline" in tw and "shard_1of8" in tw and "cpu_baseline" in tw
    assert line["higher_is_better"] is True and line["scaling"] == "weak"
    assert len(s) < 3500, len(s)
