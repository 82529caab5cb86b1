"""The host create pipelines, this build against another one (the procedure of profiles/decode_stages_rate.txt): the two libraries alternate on one GPU, a
process per run, the figure of each process's third iteration; the child's median must lie inside the parent's own min-max spread, and that spread be at
most 5 % of its median (else the figure is repeated with more runs).
  python scripts/host_pipeline_rate.py --ab-lib PARENT/libpna_gpu.so [--runs 5] [--figures small host batch solid stream bench] [--out FILE]
Figures: small  bench.py --algo deflate, 10^6 x 4 KiB: `end_to_end` ms and the third `[pna create] planning took` line under PNA_TRACE=1;
         host   scripts/host_rate.py 10000 (bench.py's end-to-end leg on its own: 10 000 x 1 MiB from pageable memory);
         batch  scripts/batch_rate.py 512 1 (pna_gpu_compress_batch from pageable memory, default batch_piece_mib);
         solid  scripts/solid_host_rate.py 2048 zstd (pna_gpu_create_solid_archive_host from pageable memory);
         stream Context.bench_stream_threads, 16 writers over 2 048 x 1 MiB (this script with --stream-once);
         bench  bench.py at its defaults, once per build: ms_per_step and value_end_to_end.
PNA_GPU_LIB picks the library of a run.  Reads nothing outside the repository but that library."""
import argparse, importlib, os, re, statistics, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def stream_once():
    sys.path.insert(0, ROOT)
    import torch
    pna = importlib.import_module("portable-network-archive_amd")
    n, L = 2048, 1 << 20
    ctx = pna.Context(0)
    src = torch.empty(n * L + 8192, dtype=torch.uint8, device="cuda")
    ctx.corpus_fill_device(0, 0, n, L, L, src.data_ptr())
    host = src[:n * L].cpu().numpy().tobytes()
    entries = [host[i * L:(i + 1) * L] for i in range(n)]
    del src
    for it in range(3):
        secs, out = ctx.bench_stream_threads(entries, threads=16)
        print(f"stream 16 writers, {n} x 1 MiB: {secs * 1e3:.1f} ms = {n * L / secs / 2**30:.2f} GiB/s of input, ratio {n * L / out:.3f}", flush=True)
    ctx.close()


SMALL = ["bench.py", "--algo", "deflate", "--files", "1000000", "--file-mib", "0.00390625", "--kind", "1", "--no-cpu-baseline", "--no-verify"]
FIGURES = {      # name -> (command, environment, [(label, regex over the whole output, which match)])
    "small": ([sys.executable] + SMALL, {"PNA_TRACE": "1"}, [("end_to_end ms", r'"end_to_end": \{"value": [0-9.]+, "unit": "MiB/s", "ms": ([0-9.]+)', 0),
                                                             ("planning ms", r"\[pna create\] planning took ([0-9.]+) ms", 2)]),
    "host": ([sys.executable, "scripts/host_rate.py", "10000"], {}, [("create ms", r"rc 0 ([0-9.]+) ms", 2)]),
    "batch": ([sys.executable, "scripts/batch_rate.py", "512", "1"], {}, [("call ms", r"call \d: rc 0 ([0-9.]+) ms", 2)]),
    "solid": ([sys.executable, "scripts/solid_host_rate.py", "2048", "zstd", "reps=3"], {}, [("create ms", r"rc 0 ([0-9.]+) ms", 2)]),
    "stream": ([sys.executable, "scripts/host_pipeline_rate.py", "--stream-once"], {}, [("16 writers ms", r"MiB: ([0-9.]+) ms", 2)]),
    "bench": ([sys.executable, "bench.py", "--gpus", "1"], {}, [("ms_per_step", r'"ms_per_step": ([0-9.]+)', 0), ("end_to_end MiB/s", r'"value_end_to_end": ([0-9.]+)', 0)]),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ab-lib"); ap.add_argument("--runs", type=int, default=5); ap.add_argument("--out", default=None)
    ap.add_argument("--figures", nargs="+", default=["small", "batch", "solid", "stream", "bench"]); ap.add_argument("--stream-once", action="store_true")
    args = ap.parse_args()
    if args.stream_once:
        return stream_once()
    log, got = [], {}
    for fig in args.figures:
        cmd, extra, wanted = FIGURES[fig]
        for run in range(1 if fig == "bench" else args.runs):
            for build in ("parent", "child"):
                env = dict(os.environ, **extra)
                env.pop("PNA_GPU_LIB", None)
                if build == "parent":
                    env["PNA_GPU_LIB"] = os.path.abspath(args.ab_lib)
                r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
                text = r.stdout + r.stderr
                if r.returncode:                                  # a failing run ends the measurement: nothing more is started on the device
                    print(text[-3000:]); sys.exit(f"{fig}: {build} run {run + 1} exited with {r.returncode}")
                keep = [ln[:600] for ln in text.splitlines() if re.search(r"planning took|^call |rc 0 |^stream 16|^\{\"metric", ln)]
                log.append(f"== {build} run {run + 1} {fig}\n" + "\n".join(keep))
                for label, rx, which in wanted:
                    got.setdefault((fig, label), {}).setdefault(build, []).append(float(re.findall(rx, text)[which]))
                print(log[-1], flush=True)
    summary = []
    for (fig, label), v in got.items():
        p, c = v["parent"], v["child"]
        if len(p) == 1:
            summary.append(f"{fig}: {label}: parent {p[0]}, child {c[0]} (once per build)")
            continue
        pm, cm = statistics.median(p), statistics.median(c)
        summary.append(f"{fig}: {label} (3rd iteration)\n  parent runs {p}  median {pm:g}  min-max {min(p):g}-{max(p):g} (spread {100 * (max(p) - min(p)) / pm:.1f} % of the median)\n"
                       f"  child  runs {c}  median {cm:g}  min-max {min(c):g}-{max(c):g}  -> child median {'inside' if min(p) <= cm <= max(p) else 'below (faster than)' if cm < min(p) else 'ABOVE (slower than)'} the parent's spread")
    report = "\n".join(summary) + "\n\n---- every run's output\n" + "\n".join(log) + "\n"
    print(report)
    if args.out:
        with open(args.out, "w") as f:
            f.write(report)


if __name__ == "__main__":
    main()
