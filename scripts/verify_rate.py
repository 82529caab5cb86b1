"""Rate of `pna verify` (pna_gpu_verify_archive_host) against extract on the same archive, on the GPU box: python scripts/verify_rate.py [files]
A files x 1 MiB zstd-3 archive built from host memory (10 000 by default); extract, verify and verify --fast each timed once after a warm-up.
Prints GiB/s of ARCHIVE bytes (what verify reads), and one JSON line."""
import ctypes, importlib, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
pna = importlib.import_module("portable-network-archive_amd")
n, L = int(sys.argv[1]) if len(sys.argv) > 1 else 10000, 1 << 20
ctx = pna.Context(0)
src = torch.empty(L * 256 + 8192, dtype=torch.uint8, device="cuda")
ctx.corpus_fill_device(0, 0, 256, L, L, src.data_ptr())
host = src[:256 * L].cpu().numpy().tobytes()
ents = [memoryview(host)[(i % 256) * L:(i % 256 + 1) * L] for i in range(n)]
names = [f"enwik/part{i:07d}.txt" for i in range(n)]
arc = pna.create_archive(ctx, names, [bytes(e) for e in ents], algo=pna.ALGO_ZSTD, level=3)
del ents
seen = [0]
def cb(_u, idx, name, kind, data, ln):
    seen[0] += ln
    return 0
fn = pna.ENTRY_FN(cb)
def extract():
    rc = ctx._L.pna_gpu_extract_archive_host(ctx._h, arc, len(arc), None, 0, fn, None)
    assert rc == 0
def verify(fast):
    recs, s = pna.verify_archive(ctx, arc, fast=fast)
    assert s["rc"] == 0 and s["ok"] == n, s
res = {"files": n, "archive_mib": round(len(arc) / 2**20, 1)}
for name, f in (("extract", extract), ("verify", lambda: verify(False)), ("verify_fast", lambda: verify(True))):
    f()                                                                  # warm-up
    t0 = time.perf_counter(); f(); dt = time.perf_counter() - t0
    res[name + "_gib_s"] = round(len(arc) / dt / 2**30, 2)
    print(f"{name:12s} {n} x 1 MiB, {len(arc) / 2**20:.0f} MiB archive in host memory: {dt * 1e3:.1f} ms = {len(arc) / dt / 2**30:.2f} GiB/s of archive bytes")
print(json.dumps(res))
