"""bench.py --dump-outputs on the host: what dump_outputs() writes for given output tensors (no GPU: CPU tensors)."""
import os
import subprocess
import sys

import numpy as np
import torch

import bench


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_is_exact_and_seeded(tmp_path):
    g = torch.Generator().manual_seed(5)
    parts = [torch.randint(0, 256, (3 * (1 << 20) + 123,), dtype=torch.uint8, generator=g), torch.randint(0, 256, (5000,), dtype=torch.uint8, generator=g)]
    r = bench.dump_outputs(str(tmp_path / "a"), torch, parts, list(range(0, 40, 4)))
    bench.dump_outputs(str(tmp_path / "b"), torch, parts, list(range(0, 40, 4)))
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert r["files"] == [k + ".npy" for k in a] and r["bytes"] <= 64 << 20
    assert all(np.array_equal(a[k], b[k]) for k in a)
    full = np.concatenate([p.numpy() for p in parts])
    assert a["output_bytes"].tolist() == [full.size]
    pos = a["output_sample_pos"].astype(np.int64)
    assert pos.size == 1 << 21 and np.all(np.diff(pos) >= 0) and np.array_equal(a["output_sample"], full[pos].astype(np.float32))
    w = np.arange(1, (1 << 20) + 1, dtype=np.int64)
    p0 = parts[0].numpy().astype(np.int64)
    want = [(p0[i:i + (1 << 20)] * w[:p0[i:i + (1 << 20)].size]).sum() for i in range(0, p0.size, 1 << 20)]
    want.append((parts[1].numpy().astype(np.int64) * w[:5000]).sum())
    assert a["output_block_sums"].tolist() == want
    assert a["entry_offsets"].tolist() == list(range(0, 40, 4))
    assert {k: v.dtype for k, v in a.items()} == {"entry_offsets": np.float64, "output_block_sums": np.float64, "output_bytes": np.float64,
                                                  "output_sample": np.float32, "output_sample_pos": np.float64}


def test_small_output_is_dumped_whole(tmp_path):
    x = torch.arange(1000, dtype=torch.int64).to(torch.uint8)
    bench.dump_outputs(str(tmp_path), torch, [x])
    a = _load(tmp_path)
    assert np.array_equal(a["output_sample"], x.numpy().astype(np.float32)) and np.array_equal(a["output_sample_pos"], np.arange(1000.0))


def test_steps_must_be_positive():
    r = subprocess.run([sys.executable, bench.__file__, "--steps", "0"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--steps must be at least 1" in r.stderr
