"""`pna create --solid` from PAGEABLE host memory, plain versus AES-256-CTR versus GCM STREAM: N x 1 MiB of the bench corpus ->
pna_gpu_create_solid_archive_enc_host -> counting sink.  Prints the input rate of each, the ratio and the page-locked staging held afterwards.
python scripts/solid_enc_host_rate.py [files] [zstd|deflate] [reps=3] [option=value ...]   (files: 8192 = 8 GiB)"""
import ctypes, importlib, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
pna = importlib.import_module("portable-network-archive_amd")
args = sys.argv[1:]
n = int(args[0]) if args and args[0].isdigit() else 8192
algo = pna.ALGO_DEFLATE if "deflate" in args else pna.ALGO_ZSTD
opts = dict(kv.split("=") for kv in args if "=" in kv)
reps = int(opts.pop("reps", 3))
L = 1 << 20
ctx = pna.Context(0)
for k, v in opts.items():
    ctx.set_option(k, int(v))
dev = torch.empty(n * L + 8192, dtype=torch.uint8, device="cuda")
ctx.corpus_fill_device(0, 0, n, L, L, dev.data_ptr())
host = dev[:n * L].cpu().numpy()
del dev
torch.cuda.empty_cache()
Lb = pna.load_library()
Lb.pna_gpu_debug_pinned_bytes.restype = ctypes.c_uint64
Lb.pna_gpu_debug_pinned_bytes.argtypes = [ctypes.c_void_p]
count = [0]


def _sink(_u, buf, k):
    count[0] += k
    return 0


cb = pna.SINK_FN(_sink)
base = host.ctypes.data
a_names = (ctypes.c_char_p * n)(*[f"solid/part{i:07d}.txt".encode() for i in range(n)])
a_src = (ctypes.c_void_p * n)(*[base + i * L for i in range(n)])
a_len = (ctypes.c_size_t * n)(*[L] * n)
key, phsf = pna.kdf_pbkdf2_sha256(b"password", bytes(range(16)), 1000)
ciphers = [("plain", None), ("ctr", pna.Cipher(key, phsf, pna.MODE_CTR, ivs=bytes(16))), ("gcm", pna.Cipher(key, phsf, pna.MODE_GCM, ivs=bytes(39)))]
for name, ci in ciphers:
    cs = ci.struct(1) if ci is not None else None
    for it in range(reps):
        count[0] = 0
        t0 = time.perf_counter()
        rc = Lb.pna_gpu_create_solid_archive_enc_host(ctx._h, algo, pna.LEVEL_DEFAULT, n, a_names, a_src, a_len, ctypes.byref(cs) if cs is not None else None, cb, None)
        t1 = time.perf_counter()
        print(f"{name} {n} x 1 MiB: rc {rc} {1e3 * (t1 - t0):.1f} ms = {n * L / (t1 - t0) / 2**20:.0f} MiB/s of input, ratio {n * L / max(count[0], 1):.3f}, "
              f"pinned {Lb.pna_gpu_debug_pinned_bytes(ctx._h) / 2**20:.0f} MiB", flush=True)
ctx.close()
