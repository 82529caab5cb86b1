"""The plain command line of the multi-GPU bench on the ONE-GPU box: `python bench.py --gpus 2 ...` with no launcher around it and no WORLD_SIZE in the
environment -- what the driver types.  The process must start its own ranks before anything touches the GPU, run the whole N > 1 control flow (shard
layout, part flags, size exchange, ordered gather, read-back of the gathered archive) and print rank 0's JSON line; PNA_BENCH_REHEARSAL=1 puts both
ranks on cuda:0 and the exchange on gloo (RCCL refuses two ranks on one device) -- timings of such a run mean nothing.

This module sorts first on purpose: its test starts child processes, and it does so before any test of this pytest process has initialised the GPU."""
import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT


@pytest.mark.gpu
@pytest.mark.timeout(900)
def test_plain_command_line_two_rank_rehearsal_on_one_gpu():
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "LOCAL_WORLD_SIZE", "GROUP_RANK")}
    env["PNA_BENCH_REHEARSAL"] = "1"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--files", "64", "--steps", "2", "--warmup", "1"],
                       env=env, capture_output=True, text=True, timeout=800)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    d = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{\"metric\"")][-1])
    assert d["n_gpus"] == 2 and d["config"]["entries"] == 64 and d["config"]["entries_per_gpu"] == 32 and d["config"]["gather_pieces"] == 2
    assert d["verified"] is True and d["gathered_archive_verified"] is True
    assert d["scaling"] == "strong" and d["value"] > 0


def _bench_dump(out_dir, *extra, env=None):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--files", "64", "--no-cpu-baseline", "--no-end-to-end",
                        "--dump-outputs", str(out_dir)] + list(extra), env=env, capture_output=True, text=True, timeout=800)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    d = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{\"metric\"")][-1])
    import numpy as np
    arrays = {f[:-4]: np.load(os.path.join(out_dir, f)) for f in sorted(os.listdir(out_dir))}
    assert d["dumped_outputs"]["files"] == [n + ".npy" for n in arrays]
    assert all(a.dtype in (np.float32, np.float64) for a in arrays.values())
    assert sum(os.path.getsize(os.path.join(out_dir, f)) for f in os.listdir(out_dir)) <= 64 << 20
    return d, arrays


@pytest.mark.gpu
@pytest.mark.timeout(900)
def test_dump_outputs_repeat_across_runs(tmp_path):
    """--dump-outputs: the same arguments give the same inputs, so two runs (whatever --steps / --warmup) dump the same arrays; the
    per-MiB checksums cover the whole archive."""
    import numpy as np
    d1, a1 = _bench_dump(tmp_path / "a", "--gpus", "1", "--steps", "1", "--warmup", "0")
    d2, a2 = _bench_dump(tmp_path / "b", "--gpus", "1", "--steps", "2", "--warmup", "1")
    assert d1["steps"] == 1 and d2["steps"] == 2 and d1["verified"] is True
    assert sorted(a1) == sorted(a2) == ["output_block_sums", "output_bytes", "output_sample", "output_sample_pos"]
    for k in a1:
        assert np.array_equal(a1[k], a2[k]), k
    n = int(a1["output_bytes"][0])
    assert abs(n - 64 * (1 << 20) / d1["ratio"]) < 0.01 * n
    assert a1["output_block_sums"].size == -(-n // (1 << 20)) and a1["output_sample"].size == min(n, 1 << 21)


@pytest.mark.gpu
@pytest.mark.timeout(900)
def test_dump_outputs_of_the_gathered_archive(tmp_path):
    """N > 1 (rehearsal on one GPU): rank 0 dumps the archive gathered from both ranks' pieces."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "LOCAL_WORLD_SIZE", "GROUP_RANK")}
    env["PNA_BENCH_REHEARSAL"] = "1"
    d, a = _bench_dump(tmp_path / "g", "--gpus", "2", "--steps", "1", "--warmup", "0", "--no-gather-compare", env=env)
    assert d["gathered_archive_verified"] is True
    n = int(a["output_bytes"][0])
    assert abs(n - 64 * (1 << 20) / d["ratio"]) < 0.01 * n
