"""bench.py --dump-outputs DIR: what the last timed evaluation returned, as DIR/<name>.npy, the same from run to run for the same arguments
(the timed region starts from a fixed noise counter, whatever the adaptive warm-up ran), so that two builds can be compared output for output."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_outputs_dtypes_and_the_size_limit(tmp_path):
    sys.path.insert(0, ROOT)
    import bench
    big = np.arange(1000, dtype=np.float32).reshape(10, 100)
    bench.dump_outputs(str(tmp_path / "a"), {"x": np.array([1.5]), "y": np.arange(4, dtype=np.int32), "big": big}, limit=3 * 400)
    assert np.load(tmp_path / "a" / "x.npy").dtype == np.float64 and np.load(tmp_path / "a" / "y.npy").dtype == np.float64
    s = np.load(tmp_path / "a" / "big.npy")
    assert s.dtype == np.float32 and s.shape == (100,) and np.all(np.diff(s) > 0) and np.all(np.isin(s, big))   # 400 bytes: a sample
    bench.dump_outputs(str(tmp_path / "b"), {"x": np.array([1.5]), "y": np.arange(4, dtype=np.int32), "big": big}, limit=3 * 400)
    assert np.array_equal(s, np.load(tmp_path / "b" / "big.npy"))                                           # the same sample every run
    bench.dump_outputs(str(tmp_path / "c"), {"big": big})
    assert np.array_equal(np.load(tmp_path / "c" / "big.npy"), big)                                         # within the limit: whole


def _bench(out, *extra):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--warmup", "3", "--config", "1", "--no-cpu-baseline",
           "--no-train-leg", "--median-iters", "0", "--dump-outputs", str(out), *extra]
    p = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    res = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][0])
    return res, {n: np.load(os.path.join(out, n + ".npy")) for n in ("elbo", "log_p")}


@pytest.mark.gpu
def test_bench_dumps_the_last_timed_step(gpu_device, tmp_path):
    """13 steps as graph replays of 4 plus one single launch, and 13 eager launches: the same last evaluation (the 13th of the timed region)."""
    r1, d1 = _bench(tmp_path / "graph", "--steps", "13")
    r2, d2 = _bench(tmp_path / "eager", "--steps", "13", "--no-graph")
    r3, d3 = _bench(tmp_path / "twelve", "--steps", "12")
    for r, steps in ((r1, 13), (r2, 13), (r3, 12)):
        assert r["steps"] == steps and r["ms_per_step"] > 0.0
    assert "hipGraph replay" in r1["config"]["launch"] and r2["config"]["launch"] == "eager"
    for d, r in ((d1, r1), (d2, r2), (d3, r3)):
        assert d["elbo"].dtype == np.float64 and d["elbo"].shape == (1,) and float(d["elbo"][0]) == r["elbo"]
        assert d["log_p"].dtype == np.float32 and d["log_p"].shape == (1024,) and np.all(np.isfinite(d["log_p"]))
    assert np.array_equal(d1["elbo"], d2["elbo"]) and np.array_equal(d1["log_p"], d2["log_p"])
    assert not np.array_equal(d1["log_p"], d3["log_p"])                 # the 12th evaluation drew other noise
