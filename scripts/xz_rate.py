"""Rates of the xz (LZMA2) decoder on the GPU box: python scripts/xz_rate.py [runs] [big_mib] [big_runs]
  (a) 512 x 1 MiB text entries (liblzma preset 6) through decompress_batch_device;
  (b) 16 384 x 16 KiB entries;
  (c) ONE single-block stream of big_mib (64) MiB: the serial case -- one wave decodes it;
  (d) verify_archive of an archive of (a).
Each after a warm-up, `runs` (6) timed runs ((c): big_runs, 6): median and min - max of the call's wall time and of the HIP-event time of the xz kernels
(pna_gpu_last_timing: ms_lz), against liblzma in the same process on 16 threads (lzma.decompress in a thread pool releases the GIL): the reference's own
decoder at this machine's CPU budget.  The entries are 256 distinct corpus files, each compressed once and used 2 / 64 times.
Writes profiles/xz_rate.txt and prints one JSON line."""
import concurrent.futures, importlib, json, lzma, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
pna = importlib.import_module("portable-network-archive_amd")
from oracle import pna_format as pf
runs = int(sys.argv[1]) if len(sys.argv) > 1 else 6
big_mib = int(sys.argv[2]) if len(sys.argv) > 2 else 64
big_runs = int(sys.argv[3]) if len(sys.argv) > 3 else 6
L, THREADS = 1 << 20, 16
ctx = pna.Context(0)
pool = concurrent.futures.ThreadPoolExecutor(THREADS)
lines, res = [], {}


def say(s):
    print(s, flush=True)
    lines.append(s)


def spread(xs):
    return {"median": round(statistics.median(xs), 2), "min": round(min(xs), 2), "max": round(max(xs), 2)}


def fmt(d):
    return f"{d['median']:.1f} ms ({d['min']:.1f} - {d['max']:.1f})"


src = torch.empty(L * 256 + 8192, dtype=torch.uint8, device="cuda")
ctx.corpus_fill_device(0, 0, 256, L, L, src.data_ptr())
host = src[:256 * L].cpu().numpy().tobytes()
del src
xz6 = lambda b: lzma.compress(b, format=lzma.FORMAT_XZ, preset=6)


def batch_case(key, label, plains, streams, nruns):
    """streams[i] decodes to plains[i]; both lists may repeat objects"""
    offs, at = [], 0
    for s in streams:
        offs.append(at); at += (len(s) + 15) & ~15
    blob = bytearray(at + 16)
    for o, s in zip(offs, streams):
        blob[o:o + len(s)] = s
    d_src = torch.frombuffer(blob, dtype=torch.uint8).cuda()
    doff, at = [], 0
    for p in plains:
        doff.append(at); at += (len(p) + 15) & ~15
    d_dst = torch.empty(at + 16, dtype=torch.uint8, device="cuda")
    lens, raws = [len(s) for s in streams], [len(p) for p in plains]
    wall, ev = [], []
    for r in range(nruns + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ctx.decompress_batch_device(d_src.data_ptr(), offs, lens, d_dst.data_ptr(), doff, raws, algo=pna.ALGO_XZ)
        wall.append((time.perf_counter() - t0) * 1e3); ev.append(ctx.timing().ms_lz)
    for k in (0, len(plains) // 2, len(plains) - 1):
        assert d_dst[doff[k]:doff[k] + raws[k]].cpu().numpy().tobytes() == plains[k]
    cpu = []
    for r in range(nruns + 1):
        t0 = time.perf_counter()
        outs = list(pool.map(lzma.decompress, streams))
        cpu.append((time.perf_counter() - t0) * 1e3)
    assert outs[-1] == plains[-1]
    mib = sum(raws) / 2**20
    w, e, c = spread(wall[1:]), spread(ev[1:]), spread(cpu[1:])
    res[key] = {"streams": len(streams), "decoded_mib": round(mib, 1), "compressed_mib": round(sum(lens) / 2**20, 1), "runs": nruns, "device_wall_ms": w,
                "xz_kernels_ms": e, "liblzma_16_threads_ms": c, "device_mib_s": round(mib / (w["median"] * 1e-3), 1),
                "liblzma_mib_s": round(mib / (c["median"] * 1e-3), 1), "device_over_liblzma": round(c["median"] / w["median"], 3)}
    say(f"{label}: device call {fmt(w)}, of which xz kernels {fmt(e)} = {mib / (w['median'] * 1e-3):.0f} MiB/s decoded; liblzma on {THREADS} threads {fmt(c)} = "
        f"{mib / (c['median'] * 1e-3):.0f} MiB/s; device / liblzma speed {c['median'] / w['median']:.2f} x  [{nruns} runs after a warm-up]")
    del d_src, d_dst
    torch.cuda.empty_cache()


files = [host[i * L:(i + 1) * L] for i in range(256)]
t0 = time.perf_counter()
big_plain = host[:big_mib * L]
f_big = pool.submit(xz6, big_plain)                                              # (the single-block stream: compressed meanwhile)
xz_files = list(pool.map(xz6, files))
small = [f[:16384] for f in files]
xz_small = list(pool.map(xz6, small))
say(f"inputs: 256 corpus files of 1 MiB -> {sum(map(len, xz_files)) / 2**20:.1f} MiB of .xz (preset 6, CRC64), their first 16 KiB -> "
    f"{sum(map(len, xz_small)) / 2**10:.0f} KiB; compressed here in {time.perf_counter() - t0:.1f} s")
batch_case("a_512_x_1mib", "(a) 512 x 1 MiB", files * 2, xz_files * 2, runs)
batch_case("b_16384_x_16kib", "(b) 16 384 x 16 KiB", small * 64, xz_small * 64, runs)
batch_case("c_one_block", f"(c) one single-block stream of {big_mib} MiB", [big_plain], [f_big.result()], big_runs)

# (d) verify of an archive of (a): fSIZ present, one FDAT chunk per entry
arc = bytearray(pf.write_archive_header())
for i in range(512):
    arc += pf.write_normal_entry(pf.file_entry_header(pna.ALGO_XZ, f"enwik/part{i:04d}.txt"), [xz_files[i % 256]], L)
arc += pf.finalize_archive()
arc = bytes(arc)
wall = []
for r in range(runs + 1):
    t0 = time.perf_counter()
    recs, s = pna.verify_archive(ctx, arc)
    wall.append((time.perf_counter() - t0) * 1e3)
    assert s["rc"] == 0 and len(recs) == 512 and all(r[2] == pna.VERIFY_OK and r[4] == L for r in recs)
w = spread(wall[1:])
res["d_verify_archive"] = {"entries": 512, "archive_mib": round(len(arc) / 2**20, 1), "runs": runs, "wall_ms": w, "decoded_mib_s": round(512 / (w["median"] * 1e-3), 1)}
say(f"(d) verify_archive of 512 x 1 MiB xz entries ({len(arc) / 2**20:.0f} MiB of archive in pageable host memory): {fmt(w)} = {512 / (w['median'] * 1e-3):.0f} MiB/s of decoded bytes")
say("not measured: multi-GPU paths, end-to-end extract from pageable memory, the presets' effect on decode speed")
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
with open(os.path.join(ROOT, "profiles", "xz_rate.txt"), "w") as f:
    f.write("\n".join(lines) + "\n" + json.dumps(res) + "\n")
print(json.dumps(res))
