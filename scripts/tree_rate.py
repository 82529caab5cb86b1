"""What one tree call saves: python scripts/tree_rate.py [--dirs N] [--per-dir K] [--runs R] > profiles/tree_rate.txt

The workload is `pna create` of a tree of --dirs directories with --per-dir text files of 4 KiB each (default 4 096 x 16 = 65 536 files), every directory
record directly before its files, deflate 6, from host memory.
  (a) one pna_gpu_create_archive_tree_host call: directories and files in walk order;
  (b) what a host had to do without entry kinds: the archive header, then per directory its record written by the host (pna_archive_entry_record_bytes)
      and one pna_gpu_create_archive_part_host call for its run of files, then AEND -- the same bytes as (a);
  (c) the floor: the files alone in one pna_gpu_create_archive_host call.
Every leg runs once to warm up, then --runs times; median and min - max of the wall clock around the calls (argument arrays are built before the clock starts,
the sink copies into one preallocated buffer)."""
import argparse
import ctypes
import importlib
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FILE_LEN = 4096


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dirs", type=int, default=4096)
    ap.add_argument("--per-dir", type=int, default=16)
    ap.add_argument("--runs", type=int, default=6)
    args = ap.parse_args()
    import torch
    pna = importlib.import_module("portable-network-archive_amd")
    from oracle import pna_format as pf
    L = pna.load_library()
    nd, per = args.dirs, args.per_dir
    nf = nd * per
    algo, level = pna.ALGO_DEFLATE, 6
    vp, sz = ctypes.c_void_p, ctypes.c_size_t
    with pna.Context(0) as ctx:
        # the files: the synthetic text corpus, generated on the device, one host buffer
        d = torch.empty(nf * FILE_LEN + 8192, dtype=torch.uint8, device="cuda")
        ctx.corpus_fill_device(0, 0, nf, FILE_LEN, FILE_LEN, d.data_ptr())
        text = ctypes.create_string_buffer(d[:nf * FILE_LEN].cpu().numpy().tobytes(), nf * FILE_LEN)
        del d
        base = ctypes.addressof(text)
        # the tree in walk order, and the files alone
        names, src, lens, kinds = [], [], [], []
        for i in range(nd):
            names.append(b"tree/d%04d" % i); src.append(None); lens.append(0); kinds.append(pna.KIND_DIRECTORY)
            for j in range(per):
                k = i * per + j
                names.append(b"tree/d%04d/f%02d.txt" % (i, j)); src.append(base + k * FILE_LEN); lens.append(FILE_LEN); kinds.append(pna.KIND_FILE)
        n = len(names)
        a_names, a_src, a_len = (ctypes.c_char_p * n)(*names), (vp * n)(*src), (sz * n)(*lens)
        a_kind = (ctypes.c_uint8 * n)(*kinds)
        ks = pna.KindsStruct()
        ks.kind = ctypes.cast(a_kind, ctypes.POINTER(ctypes.c_uint8))
        fidx = [i for i in range(n) if kinds[i] == pna.KIND_FILE]
        f_names, f_src, f_len = (ctypes.c_char_p * nf)(*[names[i] for i in fidx]), (vp * nf)(*[src[i] for i in fidx]), (sz * nf)(*[lens[i] for i in fidx])
        dir_names = [names[i] for i in range(n) if kinds[i] == pna.KIND_DIRECTORY]
        head, tail = pf.write_archive_header(0), pf.finalize_archive()

        cap = pna.archive_tree_bound(algo, [s.decode() for s in names], lens, kinds, None)
        out = ctypes.create_string_buffer(cap)
        out_base, pos = ctypes.addressof(out), [0]

        def _sink(_u, buf, k):
            ctypes.memmove(out_base + pos[0], buf, k)
            pos[0] += k
            return 0
        cb = pna.SINK_FN(_sink)

        def put(b):
            ctypes.memmove(out_base + pos[0], b, len(b))
            pos[0] += len(b)

        tree = L.pna_gpu_create_archive_tree_host
        tree.argtypes = [vp, ctypes.c_int, ctypes.c_int, sz, vp, vp, vp, vp, vp, ctypes.c_uint32, vp, ctypes.c_uint32, pna.SINK_FN, vp]
        part = L.pna_gpu_create_archive_part_host
        part.argtypes = [vp, ctypes.c_int, ctypes.c_int, sz, vp, vp, vp, ctypes.c_uint32, pna.SINK_FN, vp]
        whole = L.pna_gpu_create_archive_host
        whole.argtypes = [vp, ctypes.c_int, ctypes.c_int, sz, vp, vp, vp, pna.SINK_FN, vp]
        record = L.pna_archive_entry_record_bytes
        record.restype = sz
        record.argtypes = [ctypes.c_int, ctypes.c_char_p, vp, sz, vp, sz, vp, sz, ctypes.c_uint32, vp, sz]
        P, S = ctypes.sizeof(vp), ctypes.sizeof(sz)

        def leg_a():
            pos[0] = 0
            rc = tree(ctx._h, algo, level, n, a_names, a_src, a_len, None, None, 0, ctypes.byref(ks), pna.PART_HEAD | pna.PART_TAIL, cb, None)
            assert rc == 0, (rc, L.pna_gpu_last_error(ctx._h))

        def leg_b():
            pos[0] = 0
            put(head)
            for i in range(nd):
                got = record(pna.KIND_DIRECTORY, dir_names[i], None, 0, None, 0, None, 0, 0, out_base + pos[0], 4096)     # the host's own directory record
                pos[0] += got
                o = i * per
                rc = part(ctx._h, algo, level, per, ctypes.byref(f_names, o * P), ctypes.byref(f_src, o * P), ctypes.byref(f_len, o * S), 0, cb, None)
                assert rc == 0, (rc, L.pna_gpu_last_error(ctx._h))
            put(tail)

        def leg_c():
            pos[0] = 0
            rc = whole(ctx._h, algo, level, nf, f_names, f_src, f_len, cb, None)
            assert rc == 0, (rc, L.pna_gpu_last_error(ctx._h))

        def measure(leg):
            leg()                                                       # warm-up: workspaces, page-locked slots
            ms = []
            for _ in range(args.runs):
                t0 = time.perf_counter()
                leg()
                ms.append((time.perf_counter() - t0) * 1e3)
            return ms, out.raw[:pos[0]]

        print(f"# pna create of a tree on {torch.cuda.get_device_name(0)}: {nd} directories x {per} text files of {FILE_LEN} bytes ({nf} files, {nf * FILE_LEN >> 20} MiB), deflate {level}, "
              f"from host memory; warm-up + {args.runs} runs, wall clock ms")
        res = {}
        for tag, leg in (("a", leg_a), ("b", leg_b), ("c", leg_c)):
            res[tag] = measure(leg)
        what = {"a": "one pna_gpu_create_archive_tree_host call", "b": f"{nd} x (host directory record + pna_gpu_create_archive_part_host of {per} files)",
                "c": "the files alone, one pna_gpu_create_archive_host call (floor)"}
        for tag in ("a", "b", "c"):
            ms, arc = res[tag]
            print(f"({tag}) {what[tag]:82s} median {statistics.median(ms):9.2f} ms   min - max {min(ms):9.2f} - {max(ms):9.2f}   archive {len(arc)} bytes   runs {[round(x, 2) for x in ms]}")
        same = res["a"][1] == res["b"][1]
        print(f"(a) and (b) wrote {'the same bytes' if same else 'DIFFERENT bytes'} with the context's default options")
        if not same:
            ctx.set_option("latency_max_mib", 0)
            leg_a(); a0 = out.raw[:pos[0]]
            leg_b(); b0 = out.raw[:pos[0]]
            print(f"with latency_max_mib = 0 (a) and (b) wrote {'the same bytes' if a0 == b0 else 'DIFFERENT bytes'}")
        items = pf.read_archive(res["a"][1])[1]
        assert len(items) == n and [it.kind for it in items] == kinds
        ma, mb, mc = (statistics.median(res[t][0]) for t in ("a", "b", "c"))
        print(f"(b) / (a) = {mb / ma:.1f}x; the {nd} directory records cost (a) - (c) = {ma - mc:.2f} ms; one fragment of (b) = {mb / nd:.3f} ms")


if __name__ == "__main__":
    main()
