"""bench.py --dump-outputs: what the last timed step computed, written as .npy for build-to-build comparison."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _env():
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env["BAS_BENCH_MAX_CORES"] = "2"
    return env


def _bench(*extra):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--no-traffic", "--no-cpu-baseline", *extra],
                       capture_output=True, text=True, timeout=600, env=_env(), cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip().startswith("{")]
    assert len(lines) == 1, r.stdout[-3000:]
    return json.loads(lines[0])


def test_dump_outputs_types_and_seeded_sample(tmp_path, monkeypatch):
    """float32 is kept, other types become float64; past the limit an array becomes a fixed seeded sample with its
    positions beside it, and the files stay within the limit."""
    y = np.arange(2 * 5000, dtype=np.float32).reshape(2, 5000)
    peak = np.array([3], dtype=np.int64)
    w = bench.dump_outputs(str(tmp_path / "a"), {"y": y, "peak": peak})
    assert w == {"y.npy": [2, 5000], "peak.npy": [1]}
    assert np.load(tmp_path / "a" / "y.npy").dtype == np.float32
    assert np.array_equal(np.load(tmp_path / "a" / "y.npy"), y)
    assert np.load(tmp_path / "a" / "peak.npy").dtype == np.float64

    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 4096 + 2 * 12000)
    for d in ("b", "c"):
        w = bench.dump_outputs(str(tmp_path / d), {"y": y, "peak": peak})
        assert w["y.npy"] == [1000] and w["y_sample_index.npy"] == [1000] and w["peak.npy"] == [1]
    total = sum(os.path.getsize(tmp_path / "b" / f) for f in os.listdir(tmp_path / "b"))
    assert total <= bench.DUMP_LIMIT_BYTES
    pos = np.load(tmp_path / "b" / "y_sample_index.npy")
    assert pos.dtype == np.float64 and np.all(np.diff(pos) > 0)
    assert np.array_equal(np.load(tmp_path / "b" / "y.npy"), y.reshape(-1)[pos.astype(np.int64)])
    for f in ("y.npy", "y_sample_index.npy"):
        assert np.array_equal(np.load(tmp_path / "b" / f), np.load(tmp_path / "c" / f))


@pytest.mark.gpu
def test_bench_dump_outputs_scene_and_stream(tmp_path):
    """Scene mode: y [2, T_out] float32 after the peak rule and the peak, bit-identical from run to run (seeded
    inputs); --steps is the number of timed steps.  Stream mode: the last block (B, 2) and the running peak."""
    runs = []
    for d in ("a", "b"):
        out = _bench("--sources", "4", "--seconds", "0.5", "--steps", "3", "--warmup", "1", "--settle-ms", "0",
                     "--dump-outputs", str(tmp_path / d))
        assert out["steps"] == 3 and out["ms_per_step"] > 0
        t_out = out["config"]["out_samples"]
        assert out["dumped_outputs"] == {"y.npy": [2, t_out], "peak.npy": [1]}
        y, peak = np.load(tmp_path / d / "y.npy"), np.load(tmp_path / d / "peak.npy")
        assert y.dtype == np.float32 and y.shape == (2, t_out) and np.isfinite(y).all() and np.abs(y).max() > 0
        if peak[0] > 1.0:                                    # the peak rule: the mix is divided by its peak
            assert np.abs(y).max() <= 1.0 + 1e-6
        runs.append((y, peak))
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1])

    out = _bench("--mode", "stream", "--sources", "8", "--fs", "48000", "--block", "16384", "--steps", "2", "--warmup", "1",
                 "--dump-outputs", str(tmp_path / "s"))
    assert out["steps"] == 2 and out["ms_per_step"] > 0
    y = np.load(tmp_path / "s" / "y.npy")
    assert y.dtype == np.float32 and y.shape == tuple(out["out_block_shape"]) and np.isfinite(y).all()
    assert np.load(tmp_path / "s" / "peak.npy")[0] >= np.abs(y).max()
