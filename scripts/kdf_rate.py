"""Key derivation on the device against the host, on the GPU box: python scripts/kdf_rate.py [--runs R] [--sizes a,b,..] [--pbkdf2-sizes a,b,..]
                                                           [--e2e ENTRIES] [--off-runs K] [--parent DIR] [--out FILE]
  (a) pna_gpu_kdf_batch at the reference's default Argon2id parameters (m=19456, t=2, p=1), n jobs per call: wall time of the call (it drains its
      stream: seeds, fill, H' included), the kernels' HIP-event time and the rounds of the block memory (pna_gpu_debug_kdf_stats);
  (b) the same for PBKDF2-HMAC-SHA256 with 600 000 rounds;
  (c) the host: pna_kdf_argon2 / pna_kdf_pbkdf2_sha256 on one thread, and in a pool of 16 threads of this process (ctypes releases the GIL) -- the fair
      host alternative; then for every n who wins, by how much, and the smallest measured n from which the device wins (the crossover);
  (d) extract_archive and verify_archive of an ENTRIES x 64 KiB (2 048) AES-CTR zstd archive with one salt per entry at the default parameters, option
      kdf_device off against 1.  Off is ENTRIES serial host derivations per call: it is timed K times (2), without a warm-up -- it is host-bound.  The
      same entries under ONE salt, and the 2 048-job batch alone, bracket what the cipher stage's one launch per PHSF group costs;
  (e) with --parent DIR (a built checkout of the parent commit): bench.py --gpus 1 --steps 3 --warmup 1 --no-cpu-baseline --no-end-to-end --no-verify,
      R times from DIR and R times from this tree, alternating, each in a process of its own.
R (6) timed runs after a warm-up; median and min - max.  Writes FILE (default: profiles/kdf_rate.txt) and prints one JSON line."""
import base64, ctypes, importlib, json, os, statistics, subprocess, sys, time
from concurrent.futures import ThreadPoolExecutor
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
pna = importlib.import_module("portable-network-archive_amd")
from oracle import codec

args = sys.argv[1:]


def opt(name, default):
    if name in args:
        i = args.index(name); v = args[i + 1]; del args[i:i + 2]
        return v
    return default


runs = int(opt("--runs", 6))
sizes = [int(x) for x in opt("--sizes", "1,4,16,64,256,1024,4096").split(",")]
psizes = [int(x) for x in opt("--pbkdf2-sizes", "1,16,64,256,1024,4096").split(",")]
e2e = int(opt("--e2e", 2048))
off_runs = int(opt("--off-runs", 2))
parent = opt("--parent", None)
out_path = os.path.abspath(opt("--out", os.path.join(ROOT, "profiles", "kdf_rate.txt")))
PW, THREADS = b"password", 16
lines, res = [], {}


def say(s):
    print(s, flush=True)
    lines.append(s)


def spread(xs, unit="ms"):
    return f"median {statistics.median(xs):.2f} {unit} (min {min(xs):.2f} - max {max(xs):.2f})"


def salt(i):
    return (i + 1).to_bytes(8, "little") * 2


def wall(fn):
    t0 = time.perf_counter()
    r = fn()
    return (time.perf_counter() - t0) * 1e3, r


ctx = pna.Context(0)
L = pna.load_library()
argon_job = lambda i: {"kind": pna.KDF_ARGON2ID_JOB, "t_cost": 2, "m_cost_kib": 19456, "lanes": 1, "salt": salt(i)}
pbk_job = lambda i: {"kind": pna.KDF_PBKDF2_SHA256_JOB, "rounds": 600000, "salt": salt(i)}


def host_one(kind, i):
    key = ctypes.create_string_buffer(32)
    s = salt(i)
    if kind == "argon2id":
        rc = L.pna_kdf_argon2(2, PW, len(PW), s, len(s), 2, 19456, 1, key, 32)
    else:
        rc = L.pna_kdf_pbkdf2_sha256(PW, len(PW), s, len(s), 600000, key, 32, None, 0)
    assert rc == 0
    return key.raw


# (a), (b) the device
dev = {}
for kind, mk, ns in (("argon2id", argon_job, sizes), ("pbkdf2", pbk_job, psizes)):
    say(f"pna_gpu_kdf_batch, {'argon2id m=19456,t=2,p=1' if kind == 'argon2id' else 'pbkdf2-sha256 with 600 000 rounds'}; {runs} runs after a warm-up")
    for n in ns:
        jobs = [mk(i) for i in range(n)]
        ws, ks, first = [], [], None
        for r in range(runs + 1):
            ms, (keys, st) = wall(lambda: pna.kdf_batch(ctx, PW, jobs))
            d, h, rounds, kms = pna.kdf_stats(ctx)
            assert (d, h) == (n, 0) and st == [0] * n
            if r == 0:
                assert keys[0] == host_one(kind, 0) and (n == 1 or keys[-1] == host_one(kind, n - 1))      # the same keys as the host's
            else:
                ws.append(ms); ks.append(kms)
        dev[(kind, n)] = ws
        m = statistics.median(ws)
        say(f"  n = {n:5d}: call {spread(ws)}, kernels {spread(ks)}, {rounds} round(s) of the block memory: {n / (m * 1e-3):.0f} keys/s")
    res["device_call_ms_" + kind] = {str(n): [round(x, 2) for x in dev[(kind, n)]] for n in ns}

# (c) the host
host = {}
for kind, pool_jobs in (("argon2id", 64), ("pbkdf2", 32)):
    one = [wall(lambda: host_one(kind, 0))[0] for _ in range(runs + 1)][1:]
    with ThreadPoolExecutor(THREADS) as ex:
        pool = [wall(lambda: list(ex.map(lambda i: host_one(kind, i), range(pool_jobs))))[0] for _ in range(runs + 1)][1:]
    host[kind] = (statistics.median(one), pool_jobs / (statistics.median(pool) * 1e-3))
    say(f"host, {kind}: one derivation on one thread {spread(one)}; {pool_jobs} derivations in a pool of {THREADS} threads {spread(pool)} = {host[kind][1]:.0f} keys/s")
    res["host_one_ms_" + kind] = [round(x, 2) for x in one]
    res["host_pool16_ms_" + kind] = {"jobs": pool_jobs, "ms": [round(x, 2) for x in pool]}
for kind, ns in (("argon2id", sizes), ("pbkdf2", psizes)):
    t1, rate = host[kind]
    cross = None
    for n in ns:
        d = statistics.median(dev[(kind, n)])
        h1, h16 = n * t1, max(-(-n // THREADS) * t1, n / rate * 1e3)      # 16 threads: whole waves of 16 jobs, never faster than the pool's measured rate
        who = "device" if d < h16 else "host"
        if who == "device" and cross is None:
            cross = n
        if who == "host":
            cross = None
        say(f"  {kind} n = {n:5d}: device {d:9.1f} ms, host one thread {h1:10.1f} ms ({h1 / d:6.2f}x), host 16 threads {h16:9.1f} ms ({h16 / d:6.2f}x): the {who} wins")
    say(f"  {kind}: against 16 host threads the device wins from n = {cross} on (of the sizes measured)" if cross else f"  {kind}: the device wins at none of the sizes measured")
    res["crossover_" + kind] = cross

# (d) the read side, one salt per entry
if e2e:
    ents = [codec.corpus_file(i % 64, i + 1, 65536) for i in range(e2e)]
    jobs = [argon_job(i) for i in range(e2e)]
    batch_ms = [wall(lambda: pna.kdf_batch(ctx, PW, jobs))[0] for _ in range(runs + 1)][1:]
    keys, _ = pna.kdf_batch(ctx, PW, jobs)
    b64 = lambda s: base64.b64encode(s).decode().rstrip("=")
    parts = []
    for i, e in enumerate(ents):
        part = (pna.PART_HEAD if i == 0 else 0) | (pna.PART_TAIL if i == e2e - 1 else 0)
        ci = pna.Cipher(keys[i], "$argon2id$v=19$m=19456,t=2,p=1$" + b64(salt(i)), pna.MODE_CTR)
        parts.append(pna.create_archive_chunked(ctx, ["e/%05d" % i], [e], 0, cipher=ci, part=part))
    arc = b"".join(parts)
    one_salt = pna.create_archive_chunked(ctx, ["e/%05d" % i for i in range(e2e)], ents, 0, cipher=pna.Cipher(keys[0], "$argon2id$v=19$m=19456,t=2,p=1$" + b64(salt(0)), pna.MODE_CTR))
    want = [("e/%05d" % i, 0, e) for i, e in enumerate(ents)]
    say(f"read side: {e2e} x 64 KiB zstd AES-CTR entries, one salt per entry (argon2id m=19456,t=2,p=1), archive of {len(arc) / 2**20:.1f} MiB in host memory")
    t = {}
    for name, fn in (("extract_archive", lambda a: pna.extract_archive(ctx, a, PW)), ("verify_archive", lambda a: pna.verify_archive(ctx, a, PW))):
        ctx.set_option("kdf_device", 0)
        off = []
        for _ in range(off_runs):
            ms, got = wall(lambda: fn(arc))
            off.append(ms)
            assert (got == want) if name == "extract_archive" else (got[1]["ok"] == e2e)
        ctx.set_option("kdf_device", 1)
        on, single = [], []
        for r in range(runs + 1):
            ms, got = wall(lambda: fn(arc))
            assert (got == want) if name == "extract_archive" else (got[1]["ok"] == e2e)
            assert pna.kdf_stats(ctx)[:2] == (e2e, 0)
            ms1, _ = wall(lambda: fn(one_salt))
            if r:
                on.append(ms); single.append(ms1)
        ctx.set_option("kdf_device", 0)
        t[name] = (off, on, single)
        say(f"  {name}: kdf_device = 0 {spread(off)} over {off_runs} run(s), no warm-up; kdf_device = 1 {spread(on)}: {statistics.median(off) / statistics.median(on):.0f}x")
        say(f"      the same entries under one salt (one derivation, one cipher call), kdf_device = 1: {spread(single)}")
        res["e2e_" + name] = {"off_ms": [round(x, 1) for x in off], "on_ms": [round(x, 2) for x in on], "one_salt_on_ms": [round(x, 2) for x in single]}
    mb = statistics.median(batch_ms)
    say(f"  the {e2e}-job batch alone: {spread(batch_ms)}")
    ex_on, ex_one = statistics.median(t["extract_archive"][1]), statistics.median(t["extract_archive"][2])
    b1 = statistics.median(dev[("argon2id", 1)]) if ("argon2id", 1) in dev else float("nan")      # the one-salt extract's own batch: one job
    cipher = ex_on - mb - (ex_one - b1)
    say(f"  cipher stage, by difference: extract with a salt per entry {ex_on:.1f} ms - the batch {mb:.1f} ms - (the one-salt extract {ex_one:.1f} ms - its one-job batch {b1:.1f} ms) = "
        f"{cipher:.1f} ms for {e2e - 1} further cipher calls (one launch per PHSF group in decrypt_ctr_cbc); an estimate, not a kernel time")
    res["e2e_batch_ms"] = [round(x, 2) for x in batch_ms]
    res["e2e_cipher_calls_by_difference_ms"] = round(cipher, 2)
ctx.close()
torch.cuda.empty_cache()

# (e) the default create path, parent against this build
if parent:
    cmd = [sys.executable, "bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1", "--no-cpu-baseline", "--no-end-to-end", "--no-verify"]
    vals, steps = {"parent": [], "this": []}, {"parent": [], "this": []}
    for r in range(runs):
        for which, cwd in (("parent", parent), ("this", ROOT)):
            out = subprocess.run(cmd, cwd=cwd, capture_output=True, text=True, timeout=300)
            if out.returncode:
                say(f"(e) bench.py in {which} failed with status {out.returncode}: {out.stderr[-400:]}")
                raise SystemExit(1)
            j = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{") and '"value"' in ln][-1])
            vals[which].append(j["value"])
            steps[which].append(j.get("ms_per_step"))
            print(f"(e) run {r} {which}: {vals[which][-1]} MiB/s, step {steps[which][-1]}", flush=True)
    pm, tm = statistics.median(vals["parent"]), statistics.median(vals["this"])
    inside = min(vals["parent"]) <= tm <= max(vals["parent"])
    say("default create path: bench.py --gpus 1 --steps 3 --warmup 1 --no-cpu-baseline --no-end-to-end --no-verify, MiB/s, alternating, a process each:")
    say(f"    parent     {vals['parent']}  median {pm:.1f}")
    say(f"    this build {vals['this']}  median {tm:.1f}")
    if all(s is not None for s in steps["parent"] + steps["this"]):
        say(f"    step time, ms: parent {steps['parent']}, this build {steps['this']}")
    say(f"    this build's median lies {'inside' if inside else 'OUTSIDE'} the parent's min - max ({min(vals['parent'])} - {max(vals['parent'])})")
    res["bench_default_path"] = {"parent": vals["parent"], "this": vals["this"], "parent_step_ms": steps["parent"], "this_step_ms": steps["this"], "this_median_inside_parent_range": inside}
say("not measured: other mappings of a block onto wave lanes (16 or 64 wave lanes per block, permlane instead of LDS for the transpose); H0 / H' on the device; "
    "p > 1 at scale; a device with other work on it; the cipher stage's kernel time under one launch per entry (only the difference above)")
os.makedirs(os.path.dirname(out_path), exist_ok=True)
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n" + json.dumps(res) + "\n")
print(json.dumps(res))
