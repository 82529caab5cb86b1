"""Stored entries on the device (PNA_ALGO_STORE: k_store / k_store_fold), on the GPU box: python scripts/store_rate.py [files] [runs] [--parent DIR] [--out FILE] [--no-large]
  (a) fused against unfused: files x 1 MiB (10 000 by default), HBM-resident, unencrypted, through create_archive_device -- the fused k_store + k_store_fold
      against the unfused form of the same build (option store_unfused: k_store's copy-only form + k_frame), alternating; wall time of the call, the
      k_store launches' HIP-event time, GB/s of payload read + written;
  (b) one entry of 4 GiB - 16 bytes (one chunk, 4 096 pieces: the many-pieces fold) in both forms;
  (c) 262 144 x 4 KiB unencrypted;
  (d) the same files x 1 MiB with AES-CTR, stored against the deflate-0 call that a caller had to use before;
  (e) with --parent DIR (a built checkout of the parent commit): bench.py --gpus 1 --steps 3 --warmup 1 --no-cpu-baseline --no-end-to-end --no-verify,
      `runs` times from DIR and `runs` times from this tree, alternating, a process each.
`runs` (6) timed runs after a warm-up; median and min - max.  Writes FILE (default: profiles/store_rate.txt) and prints one JSON line."""
import importlib, json, os, statistics, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
pna = importlib.import_module("portable-network-archive_amd")
args = [a for a in sys.argv[1:]]
parent = None
if "--parent" in args:
    i = args.index("--parent"); parent = args[i + 1]; del args[i:i + 2]
out_path = os.path.join(ROOT, "profiles", "store_rate.txt")
if "--out" in args:
    i = args.index("--out"); out_path = os.path.abspath(args[i + 1]); del args[i:i + 2]
large = "--no-large" not in args
args = [a for a in args if a != "--no-large"]
n = int(args[0]) if len(args) > 0 else 10000
runs = int(args[1]) if len(args) > 1 else 6
L = 1 << 20
HBM_PEAK_GBS = 8000.0                                                   # the MI355X's data-sheet HBM3E peak, 8 TB/s: the yardstick of the '% of peak' figures, not a measurement
lines, res = [], {}


def say(s):
    print(s, flush=True)
    lines.append(s)


def spread(xs):
    return f"median {statistics.median(xs):.3f} ms (min {min(xs):.3f} - max {max(xs):.3f})"


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def both_forms(ctx, tag, names, offs, lens, src, what):
    """the fused and the unfused form of one unencrypted call, alternating: ({form: [call ms]}, {form: [k_store ms]})"""
    cap = pna.archive_bound(pna.ALGO_STORE, names, lens)
    dsts = {f: torch.empty(cap, dtype=torch.uint8, device="cuda") for f in ("fused", "unfused")}
    call, kern, caches, totals = {"fused": [], "unfused": []}, {"fused": [], "unfused": []}, {"fused": {}, "unfused": {}}, {}
    for r in range(runs + 1):
        for form in ("fused", "unfused"):
            ctx.set_option("store_unfused", 1 if form == "unfused" else 0)
            box = []
            ms = timed(lambda: box.append(ctx.create_archive_device(names, src.data_ptr(), offs, lens, dsts[form].data_ptr(), cap, algo=pna.ALGO_STORE, _cache=caches[form], want_offsets=False)))
            totals[form] = box[0][0]
            if r:
                call[form].append(ms); kern[form].append(pna.store_stats(ctx)[3])
    ctx.set_option("store_unfused", 0)
    # the two forms wrote the same archive (the unfused form's CRCs are k_frame's: an independent computation of every chunk CRC)
    same = totals["fused"] == totals["unfused"] and bool(torch.equal(dsts["fused"][:totals["fused"]], dsts["unfused"][:totals["unfused"]]))
    if not same:
        say(f"({tag}) THE TWO FORMS' ARCHIVES DIFFER")
        raise SystemExit(1)
    gb = 2 * sum(lens) / 1e9
    say(f"({tag}) {what}; {runs} runs after a warm-up, the two forms alternating")
    for form, k in (("fused", "k_store + k_store_fold"), ("unfused", "k_store copy-only + k_frame")):
        m = statistics.median(call[form])
        say(f"({tag}) {form:8s} ({k}): call {spread(call[form])} = {gb / (m * 1e-3):.0f} GB/s of payload read + written ({100 * gb / (m * 1e-3) / HBM_PEAK_GBS:.0f} % of the {HBM_PEAK_GBS / 1000:.0f} TB/s HBM peak); of which k_store {spread(kern[form])}")
    ok = statistics.median(call["fused"]) < min(call["unfused"])
    say(f"({tag}) the fused form's median lies {'below' if ok else 'NOT below'} the unfused form's fastest run")
    say(f"({tag}) the two forms' archives of {totals['fused']} bytes are equal byte for byte")
    res[tag] = {"call_ms": {f: [round(x, 3) for x in call[f]] for f in call}, "k_store_ms": {f: [round(x, 3) for x in kern[f]] for f in kern}, "fused_median_below_unfused_min": ok}
    del dsts


ctx = pna.Context(0)
src = torch.empty(n * L + 8192, dtype=torch.uint8, device="cuda")
ctx.corpus_fill_device(0, 0, n, L, L, src.data_ptr())
names = [f"enwik/part{i:07d}.txt" for i in range(n)]
offs, lens = [i * L for i in range(n)], [L] * n
both_forms(ctx, "a", names, offs, lens, src, f"{n} x 1 MiB, inputs in HBM, unencrypted, archive left in HBM")

# (d) AES-CTR: stored against deflate 0
key, phsf = pna.kdf_pbkdf2_sha256(b"password", bytes(range(16)), 1000)
ci = pna.Cipher(key, phsf, pna.MODE_CTR, ivs=os.urandom(16 * n))
cap = max(pna.archive_enc_bound(pna.ALGO_STORE, names, lens, ci), pna.archive_enc_bound(pna.ALGO_DEFLATE, names, lens, ci))
dst = torch.empty(cap, dtype=torch.uint8, device="cuda")
step, caches = {"store": [], "deflate0": []}, {"store": {}, "deflate0": {}}
for r in range(runs + 1):
    for which, (algo, level) in (("store", (pna.ALGO_STORE, 0)), ("deflate0", (pna.ALGO_DEFLATE, 0))):
        ms = timed(lambda: ctx.create_archive_device(names, src.data_ptr(), offs, lens, dst.data_ptr(), cap, algo=algo, level=level, cipher=ci, _cache=caches[which], want_offsets=False))
        if r:
            step[which].append(ms)
say(f"(d) {n} x 1 MiB with AES-256-CTR, inputs in HBM: stored {spread(step['store'])}; deflate 0 (what a caller had to use before) {spread(step['deflate0'])}")
res["d"] = {k: [round(x, 3) for x in v] for k, v in step.items()}
del dst, src
torch.cuda.empty_cache()

# (c) many small entries
ns, ls = 262144, 4096
src = torch.empty(ns * ls + 8192, dtype=torch.uint8, device="cuda")
ctx.corpus_fill_device(0, 0, ns, ls, ls, src.data_ptr())
both_forms(ctx, "c", [f"s/{i:06d}" for i in range(ns)], [i * ls for i in range(ns)], [ls] * ns, src, f"{ns} x 4 KiB, inputs in HBM, unencrypted")
del src
torch.cuda.empty_cache()

# (b) one large entry: the many-pieces fold
if large:
    big = (4 << 30) - 16
    src = torch.empty(big + 8192, dtype=torch.uint8, device="cuda")
    ctx.corpus_fill_device(0, 0, 4096, L, L, src.data_ptr())
    both_forms(ctx, "b", ["one/large.bin"], [0], [big], src, "one entry of 4 GiB - 16 bytes (one chunk, 4 096 pieces)")
    del src
ctx.close()
torch.cuda.empty_cache()

# (e) the default path, parent against this build
if parent:
    cmd = [sys.executable, "bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1", "--no-cpu-baseline", "--no-end-to-end", "--no-verify"]
    vals = {"parent": [], "this": []}
    for r in range(runs):
        for which, cwd in (("parent", parent), ("this", ROOT)):
            out = subprocess.run(cmd, cwd=cwd, capture_output=True, text=True, timeout=300)
            if out.returncode:
                say(f"(e) bench.py in {which} failed with status {out.returncode}: {out.stderr[-400:]}")
                raise SystemExit(1)
            line = [ln for ln in out.stdout.splitlines() if ln.startswith("{") and '"value"' in ln][-1]
            vals[which].append(json.loads(line)["value"])
            print(f"(e) run {r} {which}: {vals[which][-1]} MiB/s", flush=True)
    pm, tm = statistics.median(vals["parent"]), statistics.median(vals["this"])
    inside = min(vals["parent"]) <= tm <= max(vals["parent"])
    say("(e) bench.py --gpus 1 --steps 3 --warmup 1 --no-cpu-baseline --no-end-to-end --no-verify, MiB/s, alternating, a process each:")
    say(f"    parent     {vals['parent']}  median {pm:.1f}")
    say(f"    this build {vals['this']}  median {tm:.1f}")
    say(f"    this build's median lies {'inside' if inside else 'OUTSIDE'} the parent's min - max ({min(vals['parent'])} - {max(vals['parent'])})")
    res["bench_default_path"] = {"parent": vals["parent"], "this": vals["this"], "this_median_inside_parent_range": inside}
say("not measured: multi-GPU; end to end from pageable files; the host forms; the solid forms; CBC and GCM STREAM over stored payloads; another tile or piece size for k_store")
os.makedirs(os.path.dirname(out_path), exist_ok=True)
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n" + json.dumps(res) + "\n")
print(json.dumps(res))
