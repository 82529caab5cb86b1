"""What option mtile costs and what it buys: python scripts/mtile_rate.py [--files N] [--ab-lib OTHER_LIBPNA_GPU_SO] > profiles/mtile_rate.txt

For mtile = 0 / 2048 / 1024 / 512 / 256:
  * speed on the headline shape (N x 1 MiB of the synthetic corpus resident in HBM, zstd 3; deflate 6 on 2 048 x 1 MiB): the match kernel, the LZ stage and
    the whole step from pna_gpu_last_timing and the wall clock, and the ratio on that corpus;
  * ratio on real data: this repository's own documents, sources, its built library and the raw golden files, one entry each.
--ab-lib: the default path (mtile = 0) of this build against another build of the library (the parent commit's), alternating, one fresh process per
measurement (PNA_GPU_LIB picks the library).  Reads nothing outside the repository but that library."""
import argparse
import glob
import importlib
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
MTILES = (0, 2048, 1024, 512, 256)
L = 1 << 20


def speed(pna, ctx, torch, n, algo, level, steps=3):
    """steps x one device batch of n x 1 MiB; the best step's figures"""
    src = torch.empty(n * L + 8192, dtype=torch.uint8, device="cuda")
    dst = torch.empty(n * (L + 1024), dtype=torch.uint8, device="cuda")
    ctx.corpus_fill_device(0, 0, n, L, L, src.data_ptr())
    offs, lens, best = [i * L for i in range(n + 1)], [L] * n, None
    for s in range(steps + 1):                   # (the first one warms up: workspaces)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = ctx.compress_batch_device(src.data_ptr(), offs, lens, dst.data_ptr(), dst.numel(), algo=algo, level=level)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        tm = ctx.timing()
        r = {"step_ms": round(ms, 2), "ms_lz_match": round(tm.ms_lz_match, 2), "ms_lz": round(tm.ms_lz, 2), "mib_s": round(n / ms * 1e3),
             "ratio": round(n * L / max(out[-1], 1), 4)}
        if s and (best is None or r["step_ms"] < best["step_ms"]):
            best = r
    del src, dst
    torch.cuda.empty_cache()
    return best


def real_set():
    names = ["DESIGN.md", "LAB_LOG.md", "portable-network-archive_amd/csrc/k_zdec.hip", "portable-network-archive_amd/csrc/pna_host.cpp",
             "portable-network-archive_amd/libpna_gpu.so"]
    names += sorted(os.path.relpath(p, ROOT) for p in glob.glob(os.path.join(ROOT, "tests", "golden", "raw", "**", "*"), recursive=True) if os.path.isfile(p))
    return names, [open(os.path.join(ROOT, n), "rb").read() for n in names]


def child(args):
    import torch
    pna = importlib.import_module("portable-network-archive_amd")
    with pna.Context(0) as ctx:
        print(json.dumps(speed(pna, ctx, torch, args.files, pna.ALGO_ZSTD, 3, steps=args.steps)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=10000)
    ap.add_argument("--deflate-files", type=int, default=2048)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--ab-lib", default=None)
    ap.add_argument("--ab-rounds", type=int, default=6)
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child(args)
    import torch
    pna = importlib.import_module("portable-network-archive_amd")
    from oracle import codec
    names, ents = real_set()
    total = sum(len(e) for e in ents)
    print(f"# option mtile on {torch.cuda.get_device_name(0)}: {args.files} x 1 MiB zstd 3, {args.deflate_files} x 1 MiB deflate 6 (best of {args.steps} steps), "
          f"real-data set of {len(ents)} files / {total} bytes")
    with pna.Context(0) as ctx:
        for algo, level, n, tag in ((pna.ALGO_ZSTD, 3, args.files, "zstd 3"), (pna.ALGO_DEFLATE, 6, args.deflate_files, "deflate 6")):
            base = None
            for mt in MTILES:
                ctx.set_option("mtile", mt)
                r = speed(pna, ctx, torch, n, algo, level, steps=args.steps)
                base = base or r
                outs = ctx.compress_batch(ents, algo=algo, level=level)
                print(f"{tag:9s} mtile {mt:4d}: k_lzm {r['ms_lz_match']:8.2f} ms ({r['ms_lz_match'] / base['ms_lz_match']:.2f}x)  LZ {r['ms_lz']:8.2f} ms  step {r['step_ms']:8.2f} ms "
                      f"({r['step_ms'] / base['step_ms']:.2f}x)  {r['mib_s']:7d} MiB/s  ratio synthetic {r['ratio']:.4f}  real {total / sum(len(o) for o in outs):.4f}")
                if mt in (0, 256) and algo == pna.ALGO_ZSTD:
                    for nm, e, o in zip(names, ents, outs):
                        assert codec.zstd_decompress(o, len(e)) == e, nm
                        print(f"    {nm:60s} {len(e):9d} -> {len(o):9d}")
        ctx.set_option("mtile", 0)
    if args.ab_lib:
        print(f"# default path (mtile = 0), this build against {os.path.basename(os.path.dirname(os.path.abspath(args.ab_lib)))}/{os.path.basename(args.ab_lib)}, alternating, a process each")
        series = {"other": [], "this": []}
        for _ in range(args.ab_rounds):
            for who in ("other", "this"):
                env = dict(os.environ)
                if who == "other":
                    env["PNA_GPU_LIB"] = os.path.abspath(args.ab_lib)
                else:
                    env.pop("PNA_GPU_LIB", None)
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--files", str(args.files), "--steps", str(args.steps)],
                                   env=env, capture_output=True, text=True, timeout=300, check=True)
                series[who].append(json.loads(p.stdout.strip().splitlines()[-1]))
        for who in ("other", "this"):
            print(f"{who:5s} step ms {[r['step_ms'] for r in series[who]]}  k_lzm ms {[r['ms_lz_match'] for r in series[who]]}  LZ ms {[r['ms_lz'] for r in series[who]]}")
        lo, hi = min(r["step_ms"] for r in series["other"]), max(r["step_ms"] for r in series["other"])
        mine = sorted(r["step_ms"] for r in series["this"])
        med = (mine[(len(mine) - 1) // 2] + mine[len(mine) // 2]) / 2
        print(f"other's spread {lo} .. {hi} ms; this build's median {med:.2f} ms, {mine[0]} .. {mine[-1]}")


if __name__ == "__main__":
    main()
