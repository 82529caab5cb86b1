"""Rates of k_pick and of pna_gpu_extract_select_host on the GPU box: python scripts/pick_rate.py [files] [small_pieces] [runs]
  1. k_pick over files x 1 MiB pieces (10 000 by default), source and destination both 16-aligned;
  2. the same with every source at offset 7 mod 16;
  3. small_pieces x 4 KiB (262 144 by default);
  4. a hipMemcpyAsync device-to-device copy of ONE contiguous buffer of the same total bytes as 1., in the same process;
  5. selecting 1 % of the entries of a files x 1 MiB zstd-3 archive through extract_select, to host and to device, against extract_archive of the
     whole archive: wall time and uploaded bytes.
k_pick's time is its HIP-event time (pna_gpu_debug_extract_stats), the copy's a HIP-event pair around it; medians of `runs` (5) after a warm-up.
Writes profiles/pick_rate.txt and prints one JSON line."""
import importlib, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
pna = importlib.import_module("portable-network-archive_amd")
n = int(sys.argv[1]) if len(sys.argv) > 1 else 10000
n_small = int(sys.argv[2]) if len(sys.argv) > 2 else 262144
runs = int(sys.argv[3]) if len(sys.argv) > 3 else 5
L, LS = 1 << 20, 4096
ctx = pna.Context(0)
lines, res = [], {}


def say(s):
    print(s, flush=True)
    lines.append(s)


def pick_case(label, key, count, size, src_mod):
    stride = size + 256                                                          # pieces apart on both sides, as entries in a window buffer are
    src = torch.empty(count * stride + 4096, dtype=torch.uint8, device="cuda")
    dst = torch.empty(count * stride + 4096, dtype=torch.uint8, device="cuda")
    src.random_(0, 256)
    so = [256 + i * stride + src_mod for i in range(count)]
    dd = [dst.data_ptr() + 256 + i * stride for i in range(count)]
    ln = [size] * count
    ms = []
    for r in range(runs + 1):
        pna.pick_device(ctx, src, so, dd, ln)
        ms.append(pna.extract_stats(ctx)[4])
    t = statistics.median(ms[1:])
    k = count // 2
    assert torch.equal(dst[256 + k * stride:256 + k * stride + size], src[so[k]:so[k] + size])
    gib = count * size / 2**30
    res[key] = {"pieces": count, "piece_bytes": size, "source_offset_mod_16": src_mod, "k_pick_ms": round(t, 3), "gib_s": round(gib / (t * 1e-3), 1)}
    say(f"{label}: k_pick {t:.3f} ms for {gib:.2f} GiB = {gib / (t * 1e-3):.1f} GiB/s copied (read + written: twice that)")
    del src, dst
    torch.cuda.empty_cache()
    return gib / (t * 1e-3)


r_aligned = pick_case(f"{n} x 1 MiB pieces, source and destination 16-aligned", "aligned_1mib", n, L, 0)
pick_case(f"{n} x 1 MiB pieces, every source at offset 7 mod 16", "misaligned_1mib", n, L, 7)
pick_case(f"{n_small} x 4 KiB pieces, 16-aligned", "aligned_4kib", n_small, LS, 0)

# the runtime's own device-to-device copy of one contiguous buffer of n MiB
a = torch.empty(n * L, dtype=torch.uint8, device="cuda").random_(0, 256)
b = torch.empty(n * L, dtype=torch.uint8, device="cuda")
ms = []
for r in range(runs + 1):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); b.copy_(a, non_blocking=True); e1.record(); torch.cuda.synchronize()      # (Tensor.copy_ between two device tensors is hipMemcpyAsync device-to-device)
    ms.append(e0.elapsed_time(e1))
t = statistics.median(ms[1:])
r_copy = n * L / 2**30 / (t * 1e-3)
res["memcpy_d2d"] = {"bytes": n * L, "ms": round(t, 3), "gib_s": round(r_copy, 1)}
res["k_pick_over_memcpy"] = round(r_aligned / r_copy, 3)
say(f"hipMemcpyAsync device-to-device, one buffer of {n} MiB: {t:.3f} ms = {r_copy:.1f} GiB/s; k_pick on aligned 1 MiB pieces reaches {r_aligned / r_copy:.2f} x that")
del a, b
torch.cuda.empty_cache()

# 1 % of an archive through extract_select against extract_archive of all of it
src = torch.empty(L * 256 + 8192, dtype=torch.uint8, device="cuda")
ctx.corpus_fill_device(0, 0, 256, L, L, src.data_ptr())
host = src[:256 * L].cpu().numpy()
del src
names = [f"enwik/part{i:07d}.txt" for i in range(n)]
arc = pna.create_archive(ctx, names, [host[(i % 256) * L:(i % 256 + 1) * L].tobytes() for i in range(n)], algo=pna.ALGO_ZSTD, level=3)
want = set(range(0, n, 100))
dev = torch.empty(len(want) * L, dtype=torch.uint8, device="cuda")


def timed(f):
    f()
    ts = []
    for _ in range(runs):
        t0 = time.perf_counter(); f(); ts.append(time.perf_counter() - t0)
    return statistics.median(ts)


def to_host():
    recs, s = pna.extract_select(ctx, arc, lambda i, *a: "host" if i in want else None)
    assert s["to_host"] == len(want) and recs[1][4] == host[(100 % 256) * L:(100 % 256 + 1) * L].tobytes()


def to_device():
    recs, s = pna.extract_select(ctx, arc, lambda i, *a: dev[(i // 100) * L:(i // 100 + 1) * L] if i in want else None)
    assert s["to_device"] == len(want)


t_host = timed(to_host); up_host = pna.extract_stats(ctx)[0]
t_dev = timed(to_device); up_dev = pna.extract_stats(ctx)[0]
assert dev[L:2 * L].cpu().numpy().tobytes() == host[(100 % 256) * L:(100 % 256 + 1) * L].tobytes()
t_all = timed(lambda: pna.extract_archive(ctx, arc))
res["select_1_percent"] = {"entries": n, "selected": len(want), "archive_mib": round(len(arc) / 2**20, 1), "to_host_ms": round(t_host * 1e3, 1),
                           "to_device_ms": round(t_dev * 1e3, 1), "uploaded_mib_host": round(up_host / 2**20, 1), "uploaded_mib_device": round(up_dev / 2**20, 1),
                           "extract_archive_ms": round(t_all * 1e3, 1)}
say(f"{n} x 1 MiB zstd-3 archive of {len(arc) / 2**20:.0f} MiB, {len(want)} entries selected: extract_select to host {t_host * 1e3:.1f} ms "
    f"({up_host / 2**20:.1f} MiB uploaded), to device {t_dev * 1e3:.1f} ms ({up_dev / 2**20:.1f} MiB uploaded); extract_archive of every entry {t_all * 1e3:.1f} ms "
    f"({len(arc) / 2**20:.0f} MiB uploaded)")
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
with open(os.path.join(ROOT, "profiles", "pick_rate.txt"), "w") as f:
    f.write("\n".join(lines) + "\n" + json.dumps(res) + "\n")
print(json.dumps(res))
