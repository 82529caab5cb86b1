"""Streams whose decoded size is recorded nowhere -- a solid entry's SDAT stream, an entry without fSIZ -- are measured on the device first
(pna_gpu_open_size_device: the exact size, or a proven bound) and decoded into a buffer of that size by the extract driver: streams that compress
better than 64 : 1, and streams of more than 1 GiB, of this library's writers and of the reference's shapes."""
import ctypes
import hashlib
import os
import zlib

import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ZSTD_MAGIC = bytes.fromhex("28b52ffd")
PNA_E_INVAL = -2                                                        # include/pna_gpu.h


def _plain(pf, names, ents):
    """the serialised inner stream of a solid entry (STORE records, fSIZ included)"""
    return b"".join(pf.write_normal_entry(pf.file_entry_header(0, pf.sanitize_name(nm)), [e] if e else [], len(e)) for nm, e in zip(names, ents))


def _solid_archive(pf, compression, body, piece=1 << 20):
    return pf.write_archive_header() + pf.write_solid_entry(compression, [body[i:i + piece] for i in range(0, len(body), piece)]) + pf.finalize_archive()


def _zstd_raw_rle(data):
    """one zstd frame WITHOUT Frame_Content_Size (window 128 KiB): an RLE block for every 128 KiB of one byte value, a raw block otherwise"""
    out = bytearray(ZSTD_MAGIC + bytes([0x00, 7 << 3]))
    B = 128 << 10
    for i in range(0, len(data), B):
        blk = data[i:i + B]
        last = 1 if i + B >= len(data) else 0
        if blk.count(blk[:1]) == len(blk):
            out += ((len(blk) << 3) | (1 << 1) | last).to_bytes(3, "little") + blk[:1]
        else:
            out += ((len(blk) << 3) | last).to_bytes(3, "little") + blk
    return bytes(out)


def _mixed(codec):
    names = ["logs/a.txt", "zeros.img", "logs/b.txt", "empty", "tail.txt"]
    ents = [codec.corpus_file(0, 11, 70000), bytes(200 << 20), codec.corpus_file(1, 12, 5000), b"", b"x" * 1000]
    return names, ents


def _check_extract(pna, ctx, arc, names, ents, pf):
    got = pna.extract_archive(ctx, arc)
    assert [g[0] for g in got] == [pf.sanitize_name(n) for n in names]
    for (nm, _, data), e in zip(got, ents):
        assert len(data) == len(e) and data == e, nm


def _measure(ctx, pna, algo, body):
    import torch
    d = torch.zeros(len(body) + 64, dtype=torch.uint8, device="cuda")
    if body:
        d[:len(body)] = torch.frombuffer(bytearray(body), dtype=torch.uint8).cuda()
    return ctx.open_size_device(d.data_ptr(), 0, len(body), algo=algo)


# ---- 1. compressed better than 64 : 1, more than 64 MiB decoded
def test_deflate_solid_of_zeros_extracts(gpu_ctx, pna, pf, codec):
    names, ents = _mixed(codec)
    body = zlib.compress(_plain(pf, names, ents), 6)
    assert len(_plain(pf, names, ents)) > 64 * len(body)
    _check_extract(pna, gpu_ctx, _solid_archive(pf, pna.ALGO_DEFLATE, body), names, ents, pf)


def test_zstd_solid_frame_without_content_size_extracts(gpu_ctx, pna, pf, codec):
    names, ents = _mixed(codec)
    plain = _plain(pf, names, ents)
    body = _zstd_raw_rle(plain)
    assert body[4] == 0 and len(plain) > 64 * len(body)
    assert _measure(gpu_ctx, pna, pna.ALGO_ZSTD, body) == (len(plain), True)      # raw and RLE blocks only: exact
    _check_extract(pna, gpu_ctx, _solid_archive(pf, pna.ALGO_ZSTD, body), names, ents, pf)


# ---- 2. more than 1 GiB decoded
def _corpus_entries(ctx, n, L):
    import torch
    src = torch.empty(n * L + 8192, dtype=torch.uint8, device="cuda")
    ctx.corpus_fill_device(0, 0, n, L, L, src.data_ptr())
    host = src[:n * L].cpu().numpy()
    del src
    return host


def _extract_hashed(pna, ctx, arc, want):
    """pna_gpu_extract_archive_host with the entries compared by hash inside the callback (want: [(name, sha256)])"""
    seen = []

    def _cb(_u, idx, name, kind, data, n):
        h = hashlib.sha256(ctypes.string_at(data, n) if n else b"").digest()
        seen.append((name.decode(), h))
        return 0
    cb = pna.ENTRY_FN(_cb)
    ctx._check(ctx._L.pna_gpu_extract_archive_host(ctx._h, bytes(arc), len(arc), None, 0, cb, None))
    assert len(seen) == len(want)
    for (n1, h1), (n2, h2) in zip(seen, want):
        assert n1 == n2 and h1 == h2, n1


def _host_solid(ctx, pna, algo, names, views):
    """pna_gpu_create_solid_archive_host over numpy arrays: the archive's bytes"""
    import numpy as np
    n = len(names)
    parts = []

    def _sink(_u, buf, k):
        parts.append(np.ctypeslib.as_array(ctypes.cast(buf, ctypes.POINTER(ctypes.c_ubyte)), shape=(k,)).copy())
        return 0
    scb = pna.SINK_FN(_sink)
    a_names = (ctypes.c_char_p * n)(*[s.encode() for s in names])
    a_src = (ctypes.c_void_p * n)(*[v.ctypes.data if len(v) else 0 for v in views])
    a_len = (ctypes.c_size_t * n)(*[len(v) for v in views])
    ctx._check(ctx._L.pna_gpu_create_solid_archive_host(ctx._h, algo, pna.LEVEL_DEFAULT, n, a_names, a_src, a_len, scb, None))
    return np.concatenate(parts).tobytes()


def test_deflate_solid_above_1gib_from_this_library_extracts(big_ctx, pna, pf):
    n, L = 1536, 1 << 20
    host = _corpus_entries(big_ctx, n, L)
    names = [f"c/{i:05d}.txt" for i in range(n)]
    views = [host[i * L:(i + 1) * L] for i in range(n)]
    arc = _host_solid(big_ctx, pna, pna.ALGO_DEFLATE, names, views)
    _extract_hashed(pna, big_ctx, arc, [(nm, hashlib.sha256(v.tobytes()).digest()) for nm, v in zip(names, views)])


def test_zstd_solid_above_1gib_reference_shape_extracts(big_ctx, pna, pf, codec):
    if codec.system_libzstd() is None:
        pytest.skip("no system libzstd")
    n, L = 1280, 1 << 20
    host = _corpus_entries(big_ctx, n, L)
    names = [f"r/{i:05d}.txt" for i in range(n)]
    ents = [host[i * L:(i + 1) * L].tobytes() for i in range(n)]
    del host
    body = codec.libzstd_compress_checksum(_plain(pf, names, ents), 3, extra=((200, 0),))   # ZSTD_c_contentSizeFlag = 0: one frame, no content size
    assert body[:4] == ZSTD_MAGIC and body[4] >> 6 == 0 and not body[4] & 0x20
    want = [(pf.sanitize_name(nm), hashlib.sha256(e).digest()) for nm, e in zip(names, ents)]
    del ents
    _extract_hashed(pna, big_ctx, _solid_archive(pf, pna.ALGO_ZSTD, body), want)


# ---- 3. an entry without fSIZ at 100 : 1 and more
def test_deflate_entry_without_fsiz_extracts(gpu_ctx, pna, pf, codec):
    data = codec.corpus_file(0, 21, 30000) + bytes(100 << 20) + b"end"
    payload = zlib.compress(data, 9)
    assert len(data) > 100 * len(payload)
    small = codec.corpus_file(1, 22, 4000)
    arc = (pf.write_archive_header()
           + pf.write_normal_entry(pf.file_entry_header(pna.ALGO_DEFLATE, "big.img"), [payload], None)
           + pf.write_normal_entry(pf.file_entry_header(pna.ALGO_DEFLATE, "small.txt"), [zlib.compress(small)], None)
           + pf.finalize_archive())
    _check_extract(pna, gpu_ctx, arc, ["big.img", "small.txt"], [data, small], pf)


# ---- 4. the measurement itself
def test_measure_this_library_streams(gpu_ctx, pna, codec):
    data = codec.corpus_file(0, 31, 5 << 20) + bytes(3 << 20) + codec.corpus_file(1, 32, 777777)
    z = gpu_ctx.compress_batch([data])[0]
    size, exact = _measure(gpu_ctx, pna, pna.ALGO_ZSTD, z)
    # this library's frames carry no Frame_Content_Size: a bound of 128 KiB per compressed block, never below the size
    assert len(data) <= size <= len(data) + (len(z) // 3) * (128 << 10)
    assert exact == (size == len(data)) or not exact
    d = gpu_ctx.compress_batch([data], algo=pna.ALGO_DEFLATE)[0]
    assert _measure(gpu_ctx, pna, pna.ALGO_DEFLATE, d) == (len(data), True)       # sync-flush pieces: counted exactly
    assert _measure(gpu_ctx, pna, pna.ALGO_DEFLATE, zlib.compress(data, 6)) == (len(data), True)   # a foreign zlib stream
    assert _measure(gpu_ctx, pna, pna.ALGO_STORE, data[:1000]) == (1000, True)


def test_measure_reference_fixtures(gpu_ctx, pna, pf, codec):
    for name, algo in (("solid_zstd.pna", pna.ALGO_ZSTD), ("solid_deflate.pna", pna.ALGO_DEFLATE)):
        with open(os.path.join(GOLDEN, name), "rb") as f:
            arc = f.read()
        body = pf.read_archive(arc)[1][0].data
        true = len(zlib.decompress(body)) if algo == pna.ALGO_DEFLATE else len(codec.zstd_decompress(body, 64 << 20))
        size, exact = _measure(gpu_ctx, pna, algo, body)
        assert size >= true and size <= true + (128 << 10), (name, size, true)
        assert exact == (size == true) or not exact
        if algo == pna.ALGO_DEFLATE:
            assert exact and size == true
        assert len(pna.extract_archive(gpu_ctx, arc)) >= 1


def test_measure_rejects_damage(gpu_ctx, pna, codec):
    data = codec.corpus_file(0, 41, 400000)
    z = gpu_ctx.compress_batch([data])[0]
    d = zlib.compress(data, 6)
    cases = [(pna.ALGO_ZSTD, z[:len(z) // 2]),                                 # truncated inside a block
             (pna.ALGO_ZSTD, z[:5]),                                           # truncated header
             (pna.ALGO_ZSTD, b"\x00" + z[1:]),                                 # bad magic
             (pna.ALGO_DEFLATE, d[:len(d) // 2]),                              # truncated zlib stream
             (pna.ALGO_DEFLATE, b"\x78\x9c\xff" + d[3:]),                      # reserved block type at the first block
             (pna.ALGO_DEFLATE, b"")]
    zb = bytearray(z)
    zb[z.index(ZSTD_MAGIC) + 6] |= 0x06                                        # first block header: reserved block type 3
    cases.append((pna.ALGO_ZSTD, bytes(zb)))
    for algo, body in cases:
        with pytest.raises(pna.PnaGpuError) as ei:
            _measure(gpu_ctx, pna, algo, body)
        assert ei.value.code == PNA_E_INVAL, (algo, len(body), str(ei.value))


# ---- 5. every existing solid shape still extracts
def test_existing_solid_shapes_still_extract(gpu_ctx, pna, pf, codec):
    names = [f"s/{i}.txt" for i in range(6)]
    ents = [codec.corpus_file(0, 51, 2600000), b"", codec.corpus_file(1, 52, 70000), codec.corpus_file(2, 53, 300000), bytes(5000), b"tail"]
    for algo in (pna.ALGO_ZSTD, pna.ALGO_DEFLATE):
        import numpy as np
        arc = _host_solid(gpu_ctx, pna, algo, names, [np.frombuffer(e, dtype=np.uint8) for e in ents])
        _check_extract(pna, gpu_ctx, arc, names, ents, pf)
    plain = _plain(pf, names, ents)
    for body, algo in ((zlib.compress(plain, 9), pna.ALGO_DEFLATE), (codec.libzstd_compress(plain, 3) if codec.system_libzstd() else _zstd_raw_rle(plain), pna.ALGO_ZSTD),
                       (plain, pna.ALGO_STORE)):
        _check_extract(pna, gpu_ctx, _solid_archive(pf, algo, body), names, ents, pf)
    for name in ("solid_zstd.pna", "solid_deflate.pna"):
        with open(os.path.join(GOLDEN, name), "rb") as f:
            arc = f.read()
        items = pf.read_archive(arc)[1]
        body = items[0].data
        plain = zlib.decompress(body) if items[0].compression == pna.ALGO_DEFLATE else codec.zstd_decompress(body, 64 << 20)
        got = pna.extract_archive(gpu_ctx, arc)
        inner = pf.read_solid_inner(plain)
        assert [g[2] for g in got] == [it.data for it in inner]
