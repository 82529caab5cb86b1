"""Rate of `pna diff` (pna_gpu_diff_archive_host) on the GPU box: python scripts/diff_rate.py [files] [small_files] [runs]
  1. files x 1 MiB zstd-3 (10 000 by default), every file equal: diff_archive against the only way to do the same job without it -- extract_archive
     into host memory, then numpy.array_equal per entry on 16 threads --, both in this process, median of `runs` (5) timed runs after a warm-up;
  2. the same archive with 1 % of the files differing in one byte;
  3. small_files x 4 KiB deflate (262 144 by default), every file equal.
Prints MiB/s of decoded bytes compared, k_diff's own time from HIP events (pna_gpu_debug_diff_stats), and one JSON line.  The files' bytes lie in
ordinary (pageable) host memory, as an mmap'ed file's would."""
import importlib, json, os, statistics, sys, time
from concurrent.futures import ThreadPoolExecutor
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
pna = importlib.import_module("portable-network-archive_amd")
n = int(sys.argv[1]) if len(sys.argv) > 1 else 10000
n_small = int(sys.argv[2]) if len(sys.argv) > 2 else 262144
runs = int(sys.argv[3]) if len(sys.argv) > 3 else 5
L, LS = 1 << 20, 4096
ctx = pna.Context(0)
src = torch.empty(L * 256 + 8192, dtype=torch.uint8, device="cuda")
ctx.corpus_fill_device(0, 0, 256, L, L, src.data_ptr())
host = src[:256 * L].cpu().numpy()
del src


def timed(f):
    f()                                                                      # warm-up
    ts = []
    for _ in range(runs):
        t0 = time.perf_counter(); f(); ts.append(time.perf_counter() - t0)
    return statistics.median(ts)


def case(label, names, entry_of, file_of, algo, expect_differ, baseline):
    """entry_of(i) / file_of(i) -> numpy view of the bytes entry i is created from / of the file it is compared with"""
    arc = pna.create_archive(ctx, names, [entry_of(i).tobytes() for i in range(len(names))], algo=algo, level=3)
    total = sum(len(file_of(i)) for i in range(len(names)))
    index = {nm: i for i, nm in enumerate(names)}

    def source(idx, path, kind, stored):
        v = file_of(idx)
        return pna.DIFF_FS_FILE, (v.ctypes.data, len(v))

    def diff():
        recs, s = pna.diff_archive(ctx, arc, source)
        assert s["rc"] == 0 and s["differ"] == expect_differ and s["same"] == len(names) - expect_differ, s
    t_diff = timed(diff)
    streams, nbytes, ms_k = pna.diff_stats(ctx)
    out = {"case": label, "files": len(names), "archive_mib": round(len(arc) / 2**20, 1), "decoded_mib": round(total / 2**20, 1),
           "diff_ms": round(t_diff * 1e3, 1), "diff_mib_s": round(total / t_diff / 2**20), "k_diff_ms": round(ms_k, 2),
           "k_diff_gib_s_per_side": round(nbytes / (ms_k * 1e-3) / 2**30, 1) if ms_k else None}
    print(f"{label}: diff_archive {t_diff * 1e3:.1f} ms = {total / t_diff / 2**20:.0f} MiB/s of decoded bytes compared; k_diff {ms_k:.2f} ms over {nbytes / 2**20:.0f} MiB")
    if baseline:
        pool = ThreadPoolExecutor(16)

        def extract_and_compare():
            ents = pna.extract_archive(ctx, arc)
            same = sum(pool.map(lambda e: bool(np.array_equal(np.frombuffer(e[2], np.uint8), file_of(index[e[0]]))), ents, chunksize=64))
            assert same == len(names) - expect_differ
        t_base = timed(extract_and_compare)
        pool.shutdown()
        out.update({"extract_compare_ms": round(t_base * 1e3, 1), "extract_compare_mib_s": round(total / t_base / 2**20), "diff_over_extract_compare": round(t_base / t_diff, 2)})
        print(f"{label}: extract_archive + numpy.array_equal on 16 threads {t_base * 1e3:.1f} ms = {total / t_base / 2**20:.0f} MiB/s; diff_archive is {t_base / t_diff:.2f} x as fast")
    return out


res = []
names = [f"enwik/part{i:07d}.txt" for i in range(n)]
orig = lambda i: host[(i % 256) * L:(i % 256 + 1) * L]
res.append(case(f"{n} x 1 MiB zstd-3, all equal", names, orig, orig, pna.ALGO_ZSTD, 0, True))
changed = {}
for i in range(0, n, 100):                                                   # 1 %: one byte, somewhere in the file
    v = host[(i % 256) * L:(i % 256 + 1) * L].copy(); v[(i * 7919) % L] ^= 0x5A; changed[i] = v
res.append(case(f"{n} x 1 MiB zstd-3, 1 % differ", names, orig, lambda i: changed.get(i, orig(i)), pna.ALGO_ZSTD, len(changed), False))
snames = [f"small/{i % 512}/f{i:07d}" for i in range(n_small)]
small = lambda i: host[(i % 65536) * LS:(i % 65536 + 1) * LS]
res.append(case(f"{n_small} x 4 KiB deflate, all equal", snames, small, small, pna.ALGO_DEFLATE, 0, False))
print(json.dumps(res))
