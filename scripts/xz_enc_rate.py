"""Rates of the xz (LZMA2) encoder on the GPU box: python scripts/xz_enc_rate.py [runs] [n_big] [n_small] [cpu_entries]
  (a) n_big (2 048) x 1 MiB corpus text entries at xz level 6 through compress_batch_device (option xz_encode): the call, the chunk coder k_lzma2enc alone
      (pna_gpu_last_timing: ms_lit -- the xz path records its coder there, its CRC64 kernel in ms_stats, sizes + scan in ms_seq), the ratio; against
      lzma.compress(preset=6) -- liblzma, the reference's encoder -- on 16 threads in this process over the first cpu_entries (64) entries, and against this
      library's zstd at the same LZ set (zstd level 6);
  (b) n_small (16 384) x 16 KiB entries, the same way;
  (c) decompress_batch_device of (a)'s output: every entry is one block per MiB here, so one wave per entry as for liblzma's single-block streams;
  (latency) one entry of 1 MiB with the blocks latency mode chooses, and with option blk_log = 16.
Each after a warm-up, `runs` (6) timed runs: median and min - max.  Writes profiles/xz_enc_rate.txt and prints one JSON line."""
import concurrent.futures, importlib, json, lzma, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
pna = importlib.import_module("portable-network-archive_amd")
runs = int(sys.argv[1]) if len(sys.argv) > 1 else 6
n_big = int(sys.argv[2]) if len(sys.argv) > 2 else 2048
n_small = int(sys.argv[3]) if len(sys.argv) > 3 else 16384
cpu_entries = int(sys.argv[4]) if len(sys.argv) > 4 else 64
THREADS = 16
ctx = pna.Context(0)
ctx.set_option("xz_encode", 1)
pool = concurrent.futures.ThreadPoolExecutor(THREADS)
lines, res = [], {}


def say(s):
    print(s, flush=True)
    lines.append(s)


def spread(xs):
    return {"median": round(statistics.median(xs), 2), "min": round(min(xs), 2), "max": round(max(xs), 2)}


def fmt(d):
    return f"{d['median']:.1f} ms ({d['min']:.1f} - {d['max']:.1f})"


def encode_case(key, label, n, L):
    src = torch.empty(n * L + 8192, dtype=torch.uint8, device="cuda")
    ctx.corpus_fill_device(0, 0, n, L, L, src.data_ptr())
    offs, lens = [i * L for i in range(n)], [L] * n
    cap = n * pna.bound(pna.ALGO_XZ, L) + 64
    dst = torch.empty(cap, dtype=torch.uint8, device="cuda")
    out = {}
    for name, algo in (("zstd", pna.ALGO_ZSTD), ("xz", pna.ALGO_XZ)):               # (xz last: its streams stay in dst for the checks and for (c))
        wall, coder, lz = [], [], []
        for r in range(runs + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            doff = ctx.compress_batch_device(src.data_ptr(), offs, lens, dst.data_ptr(), cap, algo=algo, level=6)
            wall.append((time.perf_counter() - t0) * 1e3)
            t = ctx.timing()
            coder.append(t.ms_lit); lz.append(t.ms_lz)
        out[name] = {"wall_ms": spread(wall[1:]), "coder_ms": spread(coder[1:]), "lz_ms": spread(lz[1:]), "ratio": round(n * L / doff[n], 4), "blk_log": ctx.timing().blk_log}
        if algo == pna.ALGO_XZ:
            xoff = doff
            streams = dst[:doff[n]].cpu().numpy().tobytes()
    k = min(cpu_entries, n)
    plains = [src[i * L:(i + 1) * L].cpu().numpy().tobytes() for i in range(k)]
    for i in (0, k // 2, k - 1):
        assert lzma.decompress(streams[xoff[i]:xoff[i + 1]], format=lzma.FORMAT_XZ) == plains[i]
    cpu = []
    for r in range(runs + 1):
        t0 = time.perf_counter()
        outs = list(pool.map(lambda b: lzma.compress(b, format=lzma.FORMAT_XZ, preset=6), plains))
        cpu.append((time.perf_counter() - t0) * 1e3)
    c = spread(cpu[1:])
    mib = n * L / 2**20
    x, z = out["xz"], out["zstd"]
    res[key] = {"entries": n, "entry_bytes": L, "runs": runs, "xz": x, "zstd_level_6": z,
                "liblzma_16_threads": {"entries": k, "wall_ms": c, "ratio": round(k * L / sum(map(len, outs)), 4), "mib_s": round(k * L / 2**20 / (c["median"] * 1e-3), 1)},
                "xz_call_mib_s": round(mib / (x["wall_ms"]["median"] * 1e-3), 1), "xz_coder_mib_s": round(mib / (x["coder_ms"]["median"] * 1e-3), 1),
                "zstd_call_mib_s": round(mib / (z["wall_ms"]["median"] * 1e-3), 1)}
    q = res[key]
    say(f"{label}: xz level 6 (blocks of {1 << x['blk_log']} bytes) call {fmt(x['wall_ms'])} = {q['xz_call_mib_s']:.0f} MiB/s, of which k_lzma2enc {fmt(x['coder_ms'])} = "
        f"{q['xz_coder_mib_s']:.0f} MiB/s and the LZ stage {fmt(x['lz_ms'])}; ratio {x['ratio']:.3f}")
    say(f"    liblzma preset 6 on {THREADS} threads over the first {k} entries: {fmt(c)} = {q['liblzma_16_threads']['mib_s']:.1f} MiB/s, ratio {q['liblzma_16_threads']['ratio']:.3f}; "
        f"device call / liblzma speed {q['xz_call_mib_s'] / q['liblzma_16_threads']['mib_s']:.1f} x")
    say(f"    this library's zstd level 6 (the same LZ set) on the same batch: call {fmt(z['wall_ms'])} = {q['zstd_call_mib_s']:.0f} MiB/s, ratio {z['ratio']:.3f}")
    return src, dst, xoff


src, dst, xoff = encode_case("a_big", f"(a) {n_big} x 1 MiB", n_big, 1 << 20)
# (c) the read side over (a)'s output
L, n = 1 << 20, n_big
back = torch.empty(n * L + 64, dtype=torch.uint8, device="cuda")
wall, ev = [], []
for r in range(runs + 1):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ctx.decompress_batch_device(dst.data_ptr(), xoff[:n], [xoff[i + 1] - xoff[i] for i in range(n)], back.data_ptr(), [i * L for i in range(n)], [L] * n, algo=pna.ALGO_XZ)
    wall.append((time.perf_counter() - t0) * 1e3); ev.append(ctx.timing().ms_lz)
assert torch.equal(back[:n * L], src[:n * L])
w, e = spread(wall[1:]), spread(ev[1:])
res["c_decode_of_a"] = {"entries": n, "runs": runs, "wall_ms": w, "xz_kernels_ms": e, "mib_s": round(n / (w["median"] * 1e-3), 1)}
say(f"(c) decompress_batch_device of (a)'s {n} streams (one block each): call {fmt(w)}, of which xz kernels {fmt(e)} = {n / (w['median'] * 1e-3):.0f} MiB/s decoded")
del src, dst, back
torch.cuda.empty_cache()
encode_case("b_small", f"(b) {n_small} x 16 KiB", n_small, 16384)
# latency mode: one entry of 1 MiB, the blocks the library chooses there (16 KiB) against 64 KiB blocks -- the call is as long as its longest chunk's chain
L = 1 << 20
src = torch.empty(L + 8192, dtype=torch.uint8, device="cuda")
ctx.corpus_fill_device(0, 0, 1, L, L, src.data_ptr())
cap = pna.bound(pna.ALGO_XZ, L) + 64
dst = torch.empty(cap, dtype=torch.uint8, device="cuda")
res["latency_one_mib"] = {}
for blk_log in (0, 16):
    ctx.set_option("blk_log", blk_log)
    wall = []
    for r in range(runs + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        doff = ctx.compress_batch_device(src.data_ptr(), [0], [L], dst.data_ptr(), cap, algo=pna.ALGO_XZ, level=6)
        wall.append((time.perf_counter() - t0) * 1e3)
    w, got = spread(wall[1:]), ctx.timing().blk_log
    assert lzma.decompress(dst[:doff[1]].cpu().numpy().tobytes(), format=lzma.FORMAT_XZ) == src[:L].cpu().numpy().tobytes()
    res["latency_one_mib"]["chosen" if blk_log == 0 else "blk_log_16"] = {"blk_log": got, "wall_ms": w, "ratio": round(L / doff[1], 4)}
    say(f"(latency) 1 x 1 MiB, {'the blocks latency mode chooses' if blk_log == 0 else 'option blk_log 16'} ({1 << got} bytes): call {fmt(w)}, ratio {L / doff[1]:.3f}")
ctx.set_option("blk_log", 0)
say("(d) one form of the coder's chain was built (through LDS, one round trip per coding decision): no second timing")
say("not measured: multi-GPU paths, levels other than 6 for speed, end to end from pageable host memory")
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
with open(os.path.join(ROOT, "profiles", "xz_enc_rate.txt"), "w") as f:
    f.write("\n".join(lines) + "\n" + json.dumps(res) + "\n")
print(json.dumps(res))
