"""GPU: bench.py end to end at a small scale -- a plain run (the headline alone) with --dump-outputs, whose dumped
bytes must be the plaintext of the streams it names, and a --full run with every leg that moved behind --full."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench
import corpus

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(args, tmp_path, timeout):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--scale", "0.01",
                        "--detail-out", str(tmp_path / "detail.json")] + args,
                       cwd=str(tmp_path), capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.gpu
def test_plain_bench_dumps_the_decoded_bytes(tmp_path):
    out = tmp_path / "dump"
    line = _bench(["--steps", "3", "--warmup", "1", "--dump-outputs", str(out)], tmp_path, 600)
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in line, k
    assert line["steps"] == 3 and line["ms_per_step"] > 0 and line["value"] > 0
    assert line["cpu_baseline"] is None and "configs" not in line and "host_to_host" not in line
    spec = bench.CONFIGS["cfg3"]
    n = max(8, int(spec["streams"] * 0.01))
    status, out_len = np.load(out / "status.npy"), np.load(out / "out_len.npy")
    assert status.dtype == np.float64 and status.shape == (n,) and not status.any()
    assert (out_len == spec["size"]).all()
    sample = np.load(out / "decoded_sample.npy")
    ids = np.load(out / "decoded_sample_streams.npy")
    assert sample.dtype == np.float32 and sample.shape == (min(n, bench.DUMP_STREAMS), spec["size"])
    for row, i in enumerate(ids.astype(int)):   # stream i of the seeded batch is corpus.plain(family, 1 + i, size)
        want = np.frombuffer(corpus.plain(spec["family"], 1 + i, spec["size"]), dtype=np.uint8)
        assert np.array_equal(sample[row], want.astype(np.float32)), i


@pytest.mark.gpu
def test_full_bench_runs_the_side_legs(tmp_path):
    line = _bench(["--full", "--steps", "2", "--warmup", "1", "--configs", "cfg2-T,cfg4-R", "--side-steps", "1",
                   "--cpu-target-s", "0.2", "--side-cpu-target-s", "0.2"], tmp_path, 900)
    assert line["config"]["bit_exact"] == "all"
    assert [c["name"] for c in line["configs"]] == ["cfg2-T", "cfg4-R"]
    assert line["cpu_baseline"]["value"] > 0 and all(c["cpu"] > 0 for c in line["configs"])
    assert "cfg3" in line["host_to_host"] and line["xz_1024_blocks_host_to_host"] > 0
    assert [p[0] for p in line["scaling_projection"]["points"]] == [2, 4, 8]
    assert "latency_bound_GBps" in line["roofline"]
