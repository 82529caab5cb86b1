"""Decode rates of single zstd frames around the 4 GiB marks, this build against another one (--ab-lib: a libpna_gpu.so of the commit before; PNA_GPU_LIB picks
the library of a child process).  Writes profiles/zstd_4gib_rate.txt (--out).

  (a) this build only: ONE frame of this library (option single_frame, level 1) of 6 GiB whose every MiB is 832 KiB of random 7-bit bytes and its first
      192 KiB again -- more than 4 GiB compressed, more than 4 GiB of literals: the frame of tests/test_gpu_full_size_zstd_4gib_compressed.py;
  (b) both builds: 5 GiB of 4-bit bytes, the split adjusted: every MiB is 768 KiB of random bytes and then its last 4 KiB of them 64 times over -- a repeat
      4 KiB back, which level 1 does find (832 KiB back it does not: every byte of (a) is a literal) --: about 1.9 GiB compressed and 3.75 GiB of
      literals, below both of the old limits -- the frame the build before takes in parallel already;
  (c) both builds: 10 000 x 1 MiB of this library's zstd-3 frames (the headline shape), decoded in one call;
  (s) this build only: 64 MiB of (a)'s data as one frame on the one-workgroup kernel (zdec_serial = 1): what (a) cost per byte before.

Each build runs --rounds (2) times in a process of its own, the builds alternating, every shape warmed up once and timed --reps (3) times per process: six
timed runs per build and shape.  A build that refuses a shape is listed as that.  Times are host clocks around a call that ends in a stream synchronise.  The one-workgroup fallback is refused in (a) - (c)."""
import argparse
import importlib
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KIB, MIB, GIB = 1 << 10, 1 << 20, 1 << 30


def child(shapes, reps):
    import torch
    sys.path.insert(0, ROOT)
    pna = importlib.import_module("portable-network-archive_amd")

    def recipe(mib, seed, hi, lit_kib, near=0):
        g = torch.Generator(device="cuda")
        g.manual_seed(seed)
        d = torch.randint(0, hi, (mib, MIB), dtype=torch.uint8, device="cuda", generator=g)
        if near:                                                        # the last `near` KiB of the random part, over and over
            d[:, lit_kib * KIB:] = d[:, (lit_kib - near) * KIB:lit_kib * KIB].repeat(1, (1024 - lit_kib) // near)
        else:                                                           # the segment's first bytes again
            d[:, lit_kib * KIB:] = d[:, :(1024 - lit_kib) * KIB]
        return d.view(-1)

    def compress(ctx, src, lens, level, single):
        n = len(lens)
        so = [0]
        for k in lens:
            so.append(so[-1] + k)
        cap = n * pna.bound(pna.ALGO_ZSTD, max(lens)) + 64
        comp = torch.empty(cap, dtype=torch.uint8, device="cuda")
        ctx.set_option("single_frame", 1 if single else 0)
        offs = ctx.compress_batch_device(src.data_ptr(), so, lens, comp.data_ptr(), cap, level=level)
        ctx.set_option("single_frame", 0)
        return comp, so, offs

    def timed(ctx, comp, offs, so, lens, src, what, extra):
        n = len(lens)
        out = torch.zeros(so[-1] + 64, dtype=torch.uint8, device="cuda")
        cl = [offs[i + 1] - offs[i] for i in range(n)]
        ms = []
        for r in range(reps + 1):                                       # the first run warms up
            torch.cuda.synchronize()
            t = time.perf_counter()
            try:
                ctx.decompress_batch_device(comp.data_ptr(), offs[:n], cl, out.data_ptr(), so[:n], lens)
            except pna.PnaGpuError as e:
                print(json.dumps(dict(shape=what, refused=str(e), out_bytes=so[-1], comp_bytes=offs[n] - offs[0])), flush=True)
                return
            torch.cuda.synchronize()
            if r:
                ms.append((time.perf_counter() - t) * 1e3)
        ok = bool(torch.equal(out[:so[-1]], src[:so[-1]]))
        print(json.dumps(dict(shape=what, ms=ms, out_bytes=so[-1], comp_bytes=offs[n] - offs[0], equal=ok, **extra)), flush=True)

    for shape in shapes:
        ctx = pna.Context(0)
        ctx.set_option("zdec_fallback_max_mib", 1)
        if shape == "a":
            src = recipe(6 * 1024, 21, 128, 832)
            comp, so, offs = compress(ctx, src, [src.numel()], 1, True)
            timed(ctx, comp, offs, so, [src.numel()], src, "a", {})
        elif shape == "b":
            src = recipe(5 * 1024, 22, 16, 768, near=4)
            comp, so, offs = compress(ctx, src, [src.numel()], 1, True)
            timed(ctx, comp, offs, so, [src.numel()], src, "b", {})
        elif shape == "c":
            n, L = 10000, MIB
            src = torch.empty(n * L + 8192, dtype=torch.uint8, device="cuda")
            ctx.corpus_fill_device(0, 0, n, L, L, src.data_ptr())
            comp, so, offs = compress(ctx, src, [L] * n, 3, False)
            timed(ctx, comp, offs, so, [L] * n, src, "c", {})
        elif shape == "s":
            src = recipe(64, 21, 128, 832)
            comp, so, offs = compress(ctx, src, [src.numel()], 1, True)
            ctx.set_option("zdec_fallback_max_mib", 0)
            ctx.set_option("zdec_serial", 1)
            timed(ctx, comp, offs, so, [src.numel()], src, "s", {})
        del src, comp
        ctx.close()
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ab-lib", help="libpna_gpu.so of the build to compare with")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "zstd_4gib_rate.txt"))
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--child", help="(internal) the shapes one process measures")
    args = ap.parse_args()
    if args.child:
        return child(args.child.split(","), args.reps)
    runs = {}                                                           # (build, shape) -> list of records
    for rnd in range(args.rounds):
        for build in (["before"] if args.ab_lib else []) + ["this"]:
            env = dict(os.environ)
            env.pop("PNA_GPU_LIB", None)
            if build == "before":
                env["PNA_GPU_LIB"] = os.path.abspath(args.ab_lib)
            shapes = "b,c" if build == "before" else "a,b,c,s"
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", shapes, "--reps", str(args.reps)], env=env, stdout=subprocess.PIPE, text=True, timeout=900)
            if p.returncode:
                raise SystemExit(f"the {build} build's process failed ({p.returncode}):\n{p.stdout[-2000:]}")
            for ln in p.stdout.splitlines():
                if ln.startswith("{"):
                    rec = json.loads(ln)
                    runs.setdefault((build, rec["shape"]), []).append(rec)
    lines = ["shape build runs median_ms min_ms max_ms GiB/s_of_output(median) compressed_bytes output_bytes equal"]
    for (build, shape), recs in sorted(runs.items(), key=lambda kv: (kv[0][1], kv[0][0])):
        if any("refused" in r for r in recs):
            lines.append(f"{shape} {build} refused: {[r['refused'] for r in recs if 'refused' in r][0]} (compressed {recs[0]['comp_bytes']} B)")
            continue
        ms = [m for r in recs for m in r["ms"]]
        med = statistics.median(ms)
        lines.append(f"{shape} {build} {len(ms)} {med:.1f} {min(ms):.1f} {max(ms):.1f} {recs[0]['out_bytes'] / GIB / (med / 1e3):.2f} "
                     f"{recs[0]['comp_bytes']} {recs[0]['out_bytes']} {all(r['equal'] for r in recs)}")
        lines.append(f"    runs (ms): {' '.join(f'{m:.1f}' for m in ms)}")
    text = "\n".join([ln.strip() for ln in __doc__.strip().splitlines()[:1]] + lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
