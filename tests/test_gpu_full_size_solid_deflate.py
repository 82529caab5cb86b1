"""`pna create --solid` with Compression::Deflate at full size from PAGEABLE host memory (pna_gpu_create_solid_archive_host, run with -m gpu):
about 8 GiB of inner entries, one of them beyond 4 GiB (two FDAT chunks, FlattenWriter's cut at 2^32 - 5, lib/src/util/io.rs:60-77), streamed through
windows with at most 1.5 GiB of page-locked memory.  zlib (the C library) decodes the SDAT bodies as one stream and checks the Adler-32 chained
over the windows; 8 192 x 1 MiB equals the one-shot device archive byte for byte."""
import ctypes
import struct
import zlib

import pytest

pytestmark = pytest.mark.gpu

CH = 0xFFFFFFFB                                                     # the largest FDAT chunk FlattenWriter writes


def _need_hbm(torch, gib):
    free, _ = torch.cuda.mem_get_info()
    assert free >= gib * (1 << 30), f"the full-size case needs {gib} GiB of free HBM, found {free >> 30} GiB: an MI355X has 288 GB"


def _chunks(buf):
    """Walk a .pna image (numpy uint8 array): yields (type, payload offset, payload length, stored crc)."""
    pos, n = 8, len(buf)
    while pos < n:
        ln, = struct.unpack(">I", bytes(buf[pos:pos + 4]))
        ty = bytes(buf[pos + 4:pos + 8])
        crc, = struct.unpack(">I", bytes(buf[pos + 8 + ln:pos + 12 + ln]))
        yield ty, pos + 8, ln, crc
        pos += 12 + ln


def _host_archive(ctx, pna, algo, names, views):
    """pna_gpu_create_solid_archive_host over numpy views (pageable memory): the archive as one numpy array"""
    import numpy as np
    parts = []

    def _sink(_u, buf, k):
        parts.append(np.ctypeslib.as_array(ctypes.cast(buf, ctypes.POINTER(ctypes.c_ubyte)), shape=(k,)).copy())
        return 0
    scb = pna.SINK_FN(_sink)
    n = len(names)
    a_names = (ctypes.c_char_p * n)(*[s.encode() for s in names])
    a_src = (ctypes.c_void_p * n)(*[v.ctypes.data if len(v) else 0 for v in views])
    a_len = (ctypes.c_size_t * n)(*[len(v) for v in views])
    ctx._check(ctx._L.pna_gpu_create_solid_archive_host(ctx._h, algo, pna.LEVEL_DEFAULT, n, a_names, a_src, a_len, scb, None))
    return np.concatenate(parts)


def _pinned(ctx):
    ctx._L.pna_gpu_debug_pinned_bytes.restype = ctypes.c_uint64
    ctx._L.pna_gpu_debug_pinned_bytes.argtypes = [ctypes.c_void_p]
    return ctx._L.pna_gpu_debug_pinned_bytes(ctx._h)


def test_deflate_solid_8gib_streams_from_host_memory(big_ctx, pna, pf, codec):
    gpu_ctx = big_ctx
    import numpy as np
    import torch
    n1, L = 8192, 1 << 20
    _need_hbm(torch, 120)
    src = torch.empty(n1 * L + 8192, dtype=torch.uint8, device="cuda")
    gpu_ctx.corpus_fill_device(0, 0, n1, L, L, src.data_ptr())
    host = src[:n1 * L].cpu().numpy()

    # ---- input 1: one inner entry of 4.6 GiB between smaller ones, ~8 GiB in all
    big = 4710 * L + 12345
    assert big > CH + (1 << 29)
    cuts = [0, 3000, 3000 + big, 3000 + big + 777, 3000 + big + 777 + 5 * L]
    views = [host[a:b] for a, b in zip(cuts, cuts[1:])]
    pos = cuts[-1]
    while pos + L + 4321 <= n1 * L:
        views.append(host[pos:pos + L + 4321]); pos += L + 4321
    views.insert(2, host[:0])                                                   # an empty inner entry
    names = [f"big/{i:05d}.bin" for i in range(len(views))]
    assert sum(len(v) for v in views) > (8 << 30) - (2 << 20)
    arc = _host_archive(gpu_ctx, pna, pna.ALGO_DEFLATE, names, views)
    assert _pinned(gpu_ctx) <= (3 << 29), _pinned(gpu_ctx)

    # ---- structure: AHED, SHED, SDAT*, SEND, AEND; every chunk CRC (crc32(type || data))
    assert bytes(arc[:8]) == bytes.fromhex("89504e410d0a1a0a")
    kinds, sdat = [], []
    for ty, off, ln, crc in _chunks(arc):
        assert zlib.crc32(arc[off:off + ln], zlib.crc32(ty)) == crc, (ty, off)
        if ty == b"SDAT":
            sdat.append((off, ln))
        else:
            kinds.append(ty)
    assert kinds == [b"AHED", b"SHED", b"SEND", b"AEND"]

    # ---- the serialised inner stream, piece by piece from the oracle's writer: FHED, fSIZ, FDAT (cut at 2^32 - 5), FEND per entry
    def expected_pieces():
        for nm, v in zip(names, views):
            hdr = pf.write_chunk(b"FHED", pf.file_entry_header(0, pf.sanitize_name(nm))) + pf.write_chunk(b"fSIZ", pf.fsiz_bytes(len(v)))
            yield np.frombuffer(hdr, dtype=np.uint8)
            for o in range(0, len(v), CH):
                piece = v[o:o + CH]
                yield np.frombuffer(struct.pack(">I", len(piece)) + b"FDAT", dtype=np.uint8)
                for a in range(0, len(piece), 256 << 20):
                    yield piece[a:a + (256 << 20)]
                yield np.frombuffer(struct.pack(">I", pf.chunk_crc(b"FDAT", piece)), dtype=np.uint8)
            yield np.frombuffer(pf.write_chunk(b"FEND"), dtype=np.uint8)
    want = expected_pieces()
    cur = [np.zeros(0, dtype=np.uint8)]
    seen = [0]

    def check(out):
        o = np.frombuffer(out, dtype=np.uint8)
        while len(o):
            while not len(cur[0]):
                cur[0] = next(want)
            k = min(len(o), len(cur[0]))
            assert np.array_equal(o[:k], cur[0][:k]), seen[0]
            o, cur[0], seen[0] = o[k:], cur[0][k:], seen[0] + k
    d = zlib.decompressobj()
    for off, ln in sdat:
        check(d.decompress(arc[off:off + ln]))
    check(d.flush())
    assert d.eof and d.unused_data == b"" and not len(cur[0]) and next(want, None) is None    # zlib has checked the Adler-32 trailer
    ratio = sum(len(v) for v in views) / sum(ln for _, ln in sdat)
    assert 2.2 < ratio < 3.2, ratio

    # (the extract driver is not asked here: it decodes a zlib solid stream of unknown size into at most 1 GiB -- pna_extract.cpp -- and this one is 8 GiB;
    # tests/test_gpu_solid_deflate.py reads windowed deflate archives back through it)
    del arc

    # ---- input 2: 8 192 x 1 MiB, the host archive == the one-shot device archive
    names2 = [f"solid/f{i:05d}.txt" for i in range(n1)]
    so, sl = [i * L for i in range(n1)], [L] * n1
    cap = pna.solid_archive_bound(pna.ALGO_DEFLATE, names2, sl)
    dst = torch.empty(cap, dtype=torch.uint8, device="cuda")
    total = gpu_ctx.create_solid_archive_device(names2, src.data_ptr(), so, sl, dst.data_ptr(), cap, algo=pna.ALGO_DEFLATE)
    dev_arc = dst[:total].cpu().numpy()
    del dst, src
    torch.cuda.empty_cache()
    arc2 = _host_archive(gpu_ctx, pna, pna.ALGO_DEFLATE, names2, [host[i * L:(i + 1) * L] for i in range(n1)])
    assert len(arc2) == len(dev_arc) and np.array_equal(arc2, dev_arc)
    assert _pinned(gpu_ctx) <= (3 << 29), _pinned(gpu_ctx)
