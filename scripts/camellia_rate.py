"""Camellia-256 against AES-256 in the cipher stage, on the GPU box: python scripts/camellia_rate.py [files] [runs] [--parent DIR] [--out FILE]
  (a) k_cam_ctr against k_aes_ctr over the same bytes with the same units: the compressed payloads of a files x 1 MiB (10 000 by default) zstd-3 archive,
      where they stand in the archive image in HBM, through pna_gpu_cipher_apply_device -- the kernel's HIP-event time (pna_gpu_last_timing: ms_cipher);
  (b) the create step (pna_gpu_create_archive_enc_device, inputs in HBM, archive left in HBM) with AES-CTR and with Camellia-CTR: wall time of the call
      and the cipher stage's share of it;
  (c) with --parent DIR (a built checkout of the parent commit): bench.py --gpus 1 --steps 3 --warmup 1 --no-cpu-baseline --no-end-to-end --no-verify,
      `runs` times from DIR and `runs` times from this tree, alternating, each in a process of its own -- both lists, and whether this build's median
      lies inside the parent's min - max.
`runs` (6) timed runs after a warm-up; median and min - max.  Writes FILE (default: profiles/camellia_rate.txt) and prints one JSON line."""
import importlib, json, os, statistics, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
pna = importlib.import_module("portable-network-archive_amd")
args = [a for a in sys.argv[1:]]
parent = None
if "--parent" in args:
    i = args.index("--parent"); parent = args[i + 1]; del args[i:i + 2]
out_path = os.path.join(ROOT, "profiles", "camellia_rate.txt")
if "--out" in args:
    i = args.index("--out"); out_path = os.path.abspath(args[i + 1]); del args[i:i + 2]
n = int(args[0]) if len(args) > 0 else 10000
runs = int(args[1]) if len(args) > 1 else 6
L = 1 << 20
lines, res = [], {}


def say(s):
    print(s, flush=True)
    lines.append(s)


def spread(xs):
    return f"median {statistics.median(xs):.2f} ms (min {min(xs):.2f} - max {max(xs):.2f})"


ctx = pna.Context(0)
ctx.set_option("camellia", 1)
src = torch.empty(n * L + 8192, dtype=torch.uint8, device="cuda")
ctx.corpus_fill_device(0, 0, n, L, L, src.data_ptr())
names = [f"enwik/part{i:07d}.txt" for i in range(n)]
offs, lens = [i * L for i in range(n)], [L] * n
key, phsf = pna.kdf_pbkdf2_sha256(b"password", bytes(range(16)), 1000)
ivs = os.urandom(16 * n)
ciphers = {"aes": pna.Cipher(key, phsf, pna.MODE_CTR, ivs=ivs), "camellia": pna.Cipher(key, phsf, pna.MODE_CTR, encryption=pna.ENC_CAMELLIA, ivs=ivs)}
cap = pna.archive_enc_bound(pna.ALGO_ZSTD, names, lens, ciphers["aes"])
dst = torch.empty(cap, dtype=torch.uint8, device="cuda")

# (b) the create step
create = {}
caches = {w: {} for w in ciphers}                                       # the argument arrays of the binding, built once per cipher
for r in range(runs + 1):
    for which, ci in ciphers.items():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        total, eoff = ctx.create_archive_device(names, src.data_ptr(), offs, lens, dst.data_ptr(), cap, algo=pna.ALGO_ZSTD, level=3, cipher=ci, _cache=caches[which])
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        if r:
            create.setdefault(which, []).append((ms, ctx.timing().ms_cipher))
say(f"{n} x 1 MiB enwik-style text, zstd-3, inputs in HBM, archive of {total / 2**20:.0f} MiB left in HBM; {runs} runs after a warm-up, the two ciphers alternating")
for which in ciphers:
    say(f"(b) create with {which}-ctr: call {spread([m for m, _ in create[which]])}, of which the cipher stage {spread([c for _, c in create[which]])}")
res["create_ms"] = {w: [round(m, 2) for m, _ in create[w]] for w in ciphers}
res["create_cipher_stage_ms"] = {w: [round(c, 3) for _, c in create[w]] for w in ciphers}

# (a) the CTR kernels alone over the payloads of that archive (the last one written: Camellia's -- any bytes do, the ranges are what counts)
arc_eoff = list(eoff)
head = dst[:min(total, 4096)].cpu().numpy().tobytes()
# every entry is FHED | fSIZ | PHSF | FDAT(iv) | FDAT(ciphertext) | FEND; its ciphertext chunk ends 12 bytes (CRC, then FEND) before the next entry
first_len = arc_eoff[1] - arc_eoff[0]
fixed = head.index(b"FDAT", head.index(b"FDAT") + 4) + 4 - arc_eoff[0]              # bytes of an entry in front of its ciphertext
p_off = [arc_eoff[i] + fixed for i in range(n)]
p_len = [arc_eoff[i + 1] - arc_eoff[i] - fixed - 4 - 12 for i in range(n)]
assert min(p_len) > 0 and first_len > fixed
kern = {}
for r in range(runs + 1):
    for which, ci in ciphers.items():
        ctx.cipher_apply_device(ci, dst.data_ptr(), p_off, p_len)
        if r:
            kern.setdefault(which, []).append(ctx.timing().ms_cipher)
gib = sum(p_len) / 2**30
units = sum((x + (256 << 10) - 1) // (256 << 10) for x in p_len)
for which, k in (("aes", "k_aes_ctr"), ("camellia", "k_cam_ctr")):
    m = statistics.median(kern[which])
    say(f"(a) {k}: {spread(kern[which])} over {gib:.2f} GiB of payloads in {units} units = {gib / (m * 1e-3):.0f} GiB/s")
ratio = statistics.median(kern["camellia"]) / statistics.median(kern["aes"])
say(f"(a) k_cam_ctr / k_aes_ctr = {ratio:.2f} (both with four bank-replicated tables, 128 KiB of LDS, one workgroup of 1024 per CU; no other layout was tried for Camellia)")
res["ctr_kernel_ms"] = {w: [round(x, 3) for x in kern[w]] for w in ciphers}
res["ctr_payload_gib"] = round(gib, 3)
res["cam_over_aes"] = round(ratio, 3)
del src, dst
ctx.close()
torch.cuda.empty_cache()

# (c) the default path, parent against this build
if parent:
    cmd = [sys.executable, "bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1", "--no-cpu-baseline", "--no-end-to-end", "--no-verify"]
    vals = {"parent": [], "this": []}
    for r in range(runs):
        for which, cwd in (("parent", parent), ("this", ROOT)):
            out = subprocess.run(cmd, cwd=cwd, capture_output=True, text=True, timeout=300)
            if out.returncode:
                say(f"(c) bench.py in {which} failed with status {out.returncode}: {out.stderr[-400:]}")
                raise SystemExit(1)
            line = [ln for ln in out.stdout.splitlines() if ln.startswith("{") and '"value"' in ln][-1]
            vals[which].append(json.loads(line)["value"])
            print(f"(c) run {r} {which}: {vals[which][-1]} MiB/s", flush=True)
    pm, tm = statistics.median(vals["parent"]), statistics.median(vals["this"])
    inside = min(vals["parent"]) <= tm <= max(vals["parent"])
    say(f"(c) bench.py --gpus 1 --steps 3 --warmup 1 --no-cpu-baseline --no-end-to-end --no-verify, MiB/s, alternating, a process each:")
    say(f"    parent     {vals['parent']}  median {pm:.1f}")
    say(f"    this build {vals['this']}  median {tm:.1f}")
    say(f"    this build's median lies {'inside' if inside else 'OUTSIDE'} the parent's min - max ({min(vals['parent'])} - {max(vals['parent'])})")
    res["bench_default_path"] = {"parent": vals["parent"], "this": vals["this"], "this_median_inside_parent_range": inside}
say("not measured: another table layout for k_cam_ctr; the CBC kernels; GCM STREAM with Camellia (k_cam_ctr plus the GHASH kernels it shares with AES); the read side")
os.makedirs(os.path.dirname(out_path), exist_ok=True)
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n" + json.dumps(res) + "\n")
print(json.dumps(res))
