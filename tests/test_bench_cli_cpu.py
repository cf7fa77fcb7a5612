"""CPU: bench.py's command line -- a plain run times the headline only (the other legs and the CPU baselines
need --full), and --dump-outputs writes a bounded, fixed set of float64 arrays."""
import os
import subprocess
import sys

import numpy as np

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_refuses_what_only_full_measures():
    for extra in (["--legs", "c5"], ["--cpu-seconds", "3"]):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "1", "--warmup", "0"] + extra,
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 2 and "--full" in r.stderr, r.stderr[-2000:]


def test_dump_outputs_small_arrays_are_written_whole(tmp_path):
    lam, vel = np.arange(30, dtype=np.float64) * 0.5, np.ones((4, 6), np.float32)
    bench.dump_outputs(str(tmp_path), {"lambda": lam, "velocity": vel})
    a, v = np.load(tmp_path / "lambda.npy"), np.load(tmp_path / "velocity.npy")
    assert a.dtype == np.float64 and np.array_equal(a, lam)
    assert v.dtype == np.float64 and v.shape == (4, 6) and np.array_equal(v, vel)


def test_dump_outputs_large_arrays_are_a_fixed_bounded_sample(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BYTES_MAX", 8000)
    lam, vel = np.arange(3000, dtype=np.float64), -np.arange(600 * 6, dtype=np.float64).reshape(600, 6)
    got = []
    for run in ("a", "b"):
        bench.dump_outputs(str(tmp_path / run), {"lambda": lam, "velocity": vel})
        got.append([np.load(tmp_path / run / (n + ".npy")) for n in ("lambda", "velocity")])
    (a, v), (a2, v2) = got
    assert 8 * (a.size + v.size) <= 8000
    assert a.size > 0 and v.size > 0
    assert np.array_equal(a, a2) and np.array_equal(v, v2)            # the same sample every run
    assert np.all(np.diff(a) > 0) and np.all(np.isin(a, lam))        # sorted elements of the real output
    assert np.all(np.diff(v) < 0) and np.all(np.isin(v, vel))
