"""Cost of measuring open streams (pna_gpu_open_size_device) next to the extract of a solid archive: one line per codec with the measurement's
time per GiB of decoded content and the solid extract's time for the same stream (pna_gpu_extract_archive_host, the measurement included)."""
import argparse
import ctypes
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    import numpy as np
    import torch
    pna = __import__("portable-network-archive_amd")
    from oracle import pna_format as pf
    ctx = pna.Context(0)
    n, L = a.mib, 1 << 20
    src = torch.empty(n * L + 8192, dtype=torch.uint8, device="cuda")
    ctx.corpus_fill_device(0, 0, n, L, L, src.data_ptr())
    host = src[:n * L].cpu().numpy()
    names = [f"c/{i:05d}.txt" for i in range(n)]
    views = [host[i * L:(i + 1) * L] for i in range(n)]
    for algo, label in ((pna.ALGO_ZSTD, "zstd"), (pna.ALGO_DEFLATE, "deflate")):
        parts = []

        def _sink(_u, buf, k):
            parts.append(np.ctypeslib.as_array(ctypes.cast(buf, ctypes.POINTER(ctypes.c_ubyte)), shape=(k,)).copy())
            return 0
        scb = pna.SINK_FN(_sink)
        a_names = (ctypes.c_char_p * n)(*[s.encode() for s in names])
        a_src = (ctypes.c_void_p * n)(*[v.ctypes.data for v in views])
        a_len = (ctypes.c_size_t * n)(*[len(v) for v in views])
        ctx._check(ctx._L.pna_gpu_create_solid_archive_host(ctx._h, algo, pna.LEVEL_DEFAULT, n, a_names, a_src, a_len, scb, None))
        arc = np.concatenate(parts).tobytes()
        body = pf.read_archive(arc)[1][0].data
        plain = len(body)
        d = torch.frombuffer(bytearray(body + bytes(64)), dtype=torch.uint8).cuda()
        torch.cuda.synchronize()
        ms, size, exact = [], 0, False
        for _ in range(a.reps + 1):
            t0 = time.perf_counter()
            size, exact = ctx.open_size_device(d.data_ptr(), 0, len(body), algo=algo)
            ms.append((time.perf_counter() - t0) * 1e3)
        ms = sorted(ms[1:])
        xs = []
        cb = pna.ENTRY_FN(lambda *_: 0)
        for _ in range(a.reps + 1):
            t0 = time.perf_counter()
            ctx._check(ctx._L.pna_gpu_extract_archive_host(ctx._h, arc, len(arc), None, 0, cb, None))
            xs.append((time.perf_counter() - t0) * 1e3)
        xs = sorted(xs[1:])
        gib = n * L / (1 << 30)
        print(json.dumps({"codec": label, "decoded_mib": n, "stream_bytes": plain, "measured": size, "exact": exact,
                          "measure_ms_median": round(ms[len(ms) // 2], 2), "measure_ms_per_gib": round(ms[len(ms) // 2] / gib, 2),
                          "extract_ms_median": round(xs[len(xs) // 2], 1)}), flush=True)
        del d
    ctx.close()


if __name__ == "__main__":
    main()
