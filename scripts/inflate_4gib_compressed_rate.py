"""Measure and decode time per GiB of content for zlib streams of more than 4 GiB of compressed bytes, against a 3.5 GiB stream from the same generator
(no cliff at 4 GiB: the chunk decoder reads every stream with 64-bit positions).  One JSON line per shape:
  stored    random bytes at level 0 (stored blocks only)             -- 3.5 GiB and 4.1 GiB of content
  huffman   a 7-bit alphabet under Z_HUFFMAN_ONLY (dynamic blocks)    -- 3.5 GiB and 4.8 GiB of content
  solid     pna_gpu_create_solid_archive_host (deflate) of 4.1 GiB of random entries, read back by pna_gpu_extract_archive_host
  entry     one deflate entry of the stored stream in FDAT chunks of 2^32 - 5 bytes, with and without fSIZ, read back by pna_gpu_extract_archive_host
measure_s_per_gib: pna_gpu_open_size_device; decode_s_per_gib: pna_gpu_decompress_batch_device (size known); extract_s_per_gib: the whole extract call."""
import argparse
import ctypes
import json
import os
import struct
import sys
import time
import zlib

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

MIB, GIB = 1 << 20, 1 << 30


def _random_host(torch, n, seed, mask=0xFF):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    d = torch.randint(0, mask + 1, (n,), dtype=torch.uint8, device="cuda", generator=g)
    h = d.cpu().numpy()
    del d
    torch.cuda.empty_cache()
    return h


def _zlib(np, host, level, strategy=zlib.Z_DEFAULT_STRATEGY, piece=256 * MIB):
    co = zlib.compressobj(level, zlib.DEFLATED, 15, 8, strategy)
    parts = [np.frombuffer(co.compress(host[a:a + piece]), dtype=np.uint8) for a in range(0, host.size, piece)]
    parts.append(np.frombuffer(co.flush(), dtype=np.uint8))
    return np.concatenate(parts)


def _best(reps, fn):
    t = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); t.append(time.perf_counter() - t0)
    return min(t)


def _stream_line(ctx, pna, torch, label, raw, comp, reps):
    d_src = torch.from_numpy(comp).cuda()
    out = torch.empty(raw.size + 64, dtype=torch.uint8, device="cuda")
    gib = raw.size / GIB

    def measure():
        assert ctx.open_size_device(d_src.data_ptr(), 0, comp.size, algo=pna.ALGO_DEFLATE) == (raw.size, True)

    def decode():
        ctx.decompress_batch_device(d_src.data_ptr(), [0], [comp.size], out.data_ptr(), [0], [raw.size], algo=pna.ALGO_DEFLATE)
        torch.cuda.synchronize()
    tm, td = _best(reps, measure), _best(reps, decode)
    chunked = ctx.timing().lz_match_launches
    assert torch.equal(out[:raw.size], torch.from_numpy(raw).cuda())
    print(json.dumps({"shape": label, "content_gib": round(gib, 3), "compressed_gib": round(comp.size / GIB, 3), "chunk_decoder": chunked,
                      "measure_s_per_gib": round(tm / gib, 3), "decode_s_per_gib": round(td / gib, 3)}), flush=True)
    del d_src, out
    torch.cuda.empty_cache()


def _extract_line(ctx, pna, label, arc, content, reps):
    n = [0]

    def _cb(_u, idx, name, kind, data, k):
        n[0] += k
        return 0
    cb = pna.ENTRY_FN(_cb)

    def run():
        n[0] = 0
        ctx._check(ctx._L.pna_gpu_extract_archive_host(ctx._h, arc.ctypes.data_as(ctypes.c_char_p), arc.size, None, 0, cb, None))
        assert n[0] == content
    t = _best(reps, run)
    print(json.dumps({"shape": label, "content_gib": round(content / GIB, 3), "archive_gib": round(arc.size / GIB, 3),
                      "extract_s_per_gib": round(t / (content / GIB), 3)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--shapes", default="stored,huffman,solid,entry")
    a = ap.parse_args()
    import numpy as np
    import torch
    pna = __import__("portable-network-archive_amd")
    from oracle import pna_format as pf
    ctx = pna.Context(0)
    shapes = a.shapes.split(",")
    stored_big = None
    if "stored" in shapes or "entry" in shapes:
        for size in ((7 * GIB) // 2, 4 * GIB + 100 * MIB):
            raw = _random_host(torch, size, 21)
            comp = _zlib(np, raw, 0)
            if "stored" in shapes:
                _stream_line(ctx, pna, torch, f"stored_{size / GIB:.1f}gib", raw, comp, a.reps)
            if size > 4 * GIB:
                stored_big = (raw, comp)
            del raw, comp
    if "huffman" in shapes:
        for size in ((7 * GIB) // 2, 4 * GIB + 800 * MIB):
            raw = _random_host(torch, size, 22, 0x7F)
            comp = _zlib(np, raw, 6, zlib.Z_HUFFMAN_ONLY)
            _stream_line(ctx, pna, torch, f"huffman_{size / GIB:.1f}gib", raw, comp, a.reps)
            del raw, comp
    if "solid" in shapes:
        n = 4 * GIB + 100 * MIB
        host = _random_host(torch, n, 23)
        views = [host[i:i + 512 * MIB] for i in range(0, n, 512 * MIB)]
        parts = []

        def _sink(_u, buf, k):
            parts.append(np.ctypeslib.as_array(ctypes.cast(buf, ctypes.POINTER(ctypes.c_ubyte)), shape=(k,)).copy())
            return 0
        scb = pna.SINK_FN(_sink)
        k = len(views)
        a_names = (ctypes.c_char_p * k)(*[f"r/{i:03d}".encode() for i in range(k)])
        a_src = (ctypes.c_void_p * k)(*[v.ctypes.data for v in views])
        a_len = (ctypes.c_size_t * k)(*[len(v) for v in views])
        ctx._check(ctx._L.pna_gpu_create_solid_archive_host(ctx._h, pna.ALGO_DEFLATE, pna.LEVEL_DEFAULT, k, a_names, a_src, a_len, scb, None))
        arc = np.concatenate(parts)
        del parts, views, host
        _extract_line(ctx, pna, "solid_deflate", arc, n, a.reps)
        del arc
    if "entry" in shapes and stored_big is not None:
        raw, comp = stored_big
        for fsiz in (True, False):
            parts = [np.frombuffer(pf.write_archive_header() + pf.write_chunk(b"FHED", pf.entry_header_bytes(0, pna.ALGO_DEFLATE, 0, 0, "big.bin")), dtype=np.uint8)]
            if fsiz:
                parts.append(np.frombuffer(pf.write_chunk(b"fSIZ", struct.pack(">Q", raw.size)), dtype=np.uint8))
            for o in range(0, comp.size, (1 << 32) - 5):
                body = comp[o:o + (1 << 32) - 5]
                parts += [np.frombuffer(struct.pack(">I", body.size) + b"FDAT", dtype=np.uint8), body,
                          np.frombuffer(struct.pack(">I", zlib.crc32(body, zlib.crc32(b"FDAT")) & 0xFFFFFFFF), dtype=np.uint8)]
            parts.append(np.frombuffer(pf.write_chunk(b"FEND") + pf.finalize_archive(), dtype=np.uint8))
            arc = np.concatenate(parts)
            del parts
            _extract_line(ctx, pna, "entry_fsiz" if fsiz else "entry_no_fsiz", arc, raw.size, a.reps)
            del arc
    ctx.close()


if __name__ == "__main__":
    main()
