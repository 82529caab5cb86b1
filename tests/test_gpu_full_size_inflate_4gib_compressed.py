"""zlib streams of more than 4 GiB of COMPRESSED bytes (the reference writes one ZlibEncoder stream per deflate entry and per solid archive,
lib/src/compress.rs:32-41): the chunk decoder splits them at dynamic and stored block starts and reads them with 64-bit stream positions.
  (a) a foreign stored-only stream (incompressible data: zlib at level 0),
  (b) a foreign stream of dynamic blocks (a 7-bit alphabet under Z_HUFFMAN_ONLY),
  (c) a deflate `--solid` archive from pna_gpu_create_solid_archive_host whose SDAT stream is more than 4 GiB, read back by pna_gpu_extract_archive_host,
  (d) the reference's shape: one deflate entry of such a stream in FDAT chunks of 2^32 - 5 bytes (FlattenWriter, lib/src/util/io.rs:60-77), with and
      without fSIZ.
Until these streams could be split they were PNA_E_UNSUPPORTED, and the extracts were refused by the measurement step."""
import ctypes
import hashlib
import struct
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MIB, GIB = 1 << 20, 1 << 30
CHUNK = (1 << 32) - 5                                               # FlattenWriter's cut


def _need_hbm(torch, gib):
    free, _ = torch.cuda.mem_get_info()
    assert free >= gib * GIB, f"the full-size case needs {gib} GiB of free HBM, found {free / GIB:.0f} GiB: an MI355X has 288 GB"


def _need_ram(gib):
    with open("/proc/meminfo") as f:
        avail = {k: int(v.split()[0]) for k, v in (ln.split(":", 1) for ln in f)}["MemAvailable"] << 10
    assert avail >= gib * GIB, f"the full-size case needs {gib} GiB of free host memory, found {avail / GIB:.0f} GiB"


def _random_host(n, seed):
    import torch
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    d = torch.randint(0, 256, (n,), dtype=torch.uint8, device="cuda", generator=g)
    h = d.cpu().numpy()
    del d
    torch.cuda.empty_cache()
    return h


def _zlib(host, level, strategy=zlib.Z_DEFAULT_STRATEGY, piece=256 * MIB):
    co = zlib.compressobj(level, zlib.DEFLATED, 15, 8, strategy)
    parts = [np.frombuffer(co.compress(host[a:a + piece]), dtype=np.uint8) for a in range(0, host.size, piece)]
    parts.append(np.frombuffer(co.flush(), dtype=np.uint8))
    return np.concatenate(parts)


@pytest.fixture(scope="module")
def stored_stream():
    """(a): 4 GiB + 20 MiB of random bytes at level 0 -- stored blocks of up to 65 535 bytes, more than 4 GiB compressed."""
    _need_ram(40)
    raw = _random_host(4 * GIB + 20 * MIB + 777, 11)
    comp = _zlib(raw, 0)
    assert comp.size > 1 << 32
    return raw, comp


def _decode_known(ctx, pna, torch, raw, comp):
    d_src = torch.from_numpy(comp).cuda()
    out = torch.zeros(raw.size + 64, dtype=torch.uint8, device="cuda")
    ctx.decompress_batch_device(d_src.data_ptr(), [0], [comp.size], out.data_ptr(), [0], [raw.size], algo=pna.ALGO_DEFLATE)
    assert ctx.timing().lz_match_launches == 1                     # (the streams that went through the chunk decoder)
    want = torch.from_numpy(raw).cuda()
    assert torch.equal(out[:raw.size], want)
    return d_src, out, want


def _damage_past_4gib(ctx, pna, torch, raw, d_src, out, want, at):
    """One byte past the 4 GiB mark damaged: refused, or decoded differently (the Adler-32 trailer is checked on the device)."""
    assert at > 1 << 32
    d_src[at] ^= 0x10
    out.zero_()
    try:
        ctx.decompress_batch_device(d_src.data_ptr(), [0], [d_src.numel()], out.data_ptr(), [0], [raw.size], algo=pna.ALGO_DEFLATE)
        same = torch.equal(out[:raw.size], want)
    except pna.PnaGpuError:
        same = False
    d_src[at] ^= 0x10
    assert not same


def test_a_stored_stream_beyond_4gib_compressed(big_ctx, pna, stored_stream):
    import torch
    raw, comp = stored_stream
    _need_hbm(torch, 60)
    assert zlib.adler32(raw) == int.from_bytes(comp[-4:].tobytes(), "big")
    d_src, out, want = _decode_known(big_ctx, pna, torch, raw, comp)
    assert big_ctx.open_size_device(d_src.data_ptr(), 0, comp.size, algo=pna.ALGO_DEFLATE) == (raw.size, True)
    out.zero_()
    assert big_ctx.inflate_open_device(d_src.data_ptr(), 0, comp.size, out.data_ptr(), 0, raw.size + 64) == raw.size
    assert big_ctx.timing().lz_match_launches == 1
    assert torch.equal(out[:raw.size], want)
    _damage_past_4gib(big_ctx, pna, torch, raw, d_src, out, want, comp.size - 5 * MIB)


def test_b_dynamic_stream_beyond_4gib_compressed(big_ctx, pna):
    """(b): 7-bit symbols under Z_HUFFMAN_ONLY: dynamic blocks of literals only, 7/8 of the content's size."""
    import torch
    _need_hbm(torch, 60)
    _need_ram(40)
    raw = _random_host(4 * GIB + 700 * MIB + 333, 12)
    raw &= 0x7F
    comp = _zlib(raw, 6, zlib.Z_HUFFMAN_ONLY)
    assert comp.size > 1 << 32
    assert zlib.adler32(raw) == int.from_bytes(comp[-4:].tobytes(), "big")
    d_src, out, want = _decode_known(big_ctx, pna, torch, raw, comp)
    assert big_ctx.open_size_device(d_src.data_ptr(), 0, comp.size, algo=pna.ALGO_DEFLATE) == (raw.size, True)
    _damage_past_4gib(big_ctx, pna, torch, raw, d_src, out, want, (1 << 32) + 12345)


def _extract(ctx, pna, arc):
    seen = []

    def _cb(_u, idx, name, kind, data, k):
        h = hashlib.sha256(np.ctypeslib.as_array(ctypes.cast(data, ctypes.POINTER(ctypes.c_ubyte)), shape=(k,)) if k else b"").digest()
        seen.append((name.decode(), k, h))
        return 0
    cb = pna.ENTRY_FN(_cb)
    ctx._check(ctx._L.pna_gpu_extract_archive_host(ctx._h, arc.ctypes.data_as(ctypes.c_char_p), arc.size, None, 0, cb, None))
    return seen


def test_c_deflate_solid_archive_beyond_4gib_compressed(big_ctx, pna):
    import torch
    _need_hbm(torch, 80)
    _need_ram(48)
    n = 4 * GIB + 64 * MIB
    host = _random_host(n, 13)
    text = np.frombuffer(b"the quick brown fox jumps over the lazy dog; " * 40000, dtype=np.uint8)
    cuts = [0, 5000, 5000 + 3 * GIB, 5000 + 3 * GIB + 99, n - 3 * MIB, n]
    views = [host[a:b] for a, b in zip(cuts, cuts[1:])] + [text, host[:0]]
    names = [f"big/{i:03d}.bin" for i in range(len(views))]
    parts = []

    def _sink(_u, buf, k):
        parts.append(np.ctypeslib.as_array(ctypes.cast(buf, ctypes.POINTER(ctypes.c_ubyte)), shape=(k,)).copy())
        return 0
    scb = pna.SINK_FN(_sink)
    k = len(views)
    a_names = (ctypes.c_char_p * k)(*[s.encode() for s in names])
    a_src = (ctypes.c_void_p * k)(*[v.ctypes.data if len(v) else 0 for v in views])
    a_len = (ctypes.c_size_t * k)(*[len(v) for v in views])
    big_ctx._check(big_ctx._L.pna_gpu_create_solid_archive_host(big_ctx._h, pna.ALGO_DEFLATE, pna.LEVEL_DEFAULT, k, a_names, a_src, a_len, scb, None))
    arc = np.concatenate(parts)
    del parts
    assert arc.size > (1 << 32) + (64 << 20)                         # (the SDAT stream: all of the archive but a few hundred bytes)
    want = [(nm, len(v), hashlib.sha256(v).digest()) for nm, v in zip(names, views)]
    del views, host
    assert _extract(big_ctx, pna, arc) == want


def _reference_entry_archive(pf, pna, name, comp, raw_size):
    """AHED, FHED (deflate), fSIZ (when raw_size is not None), FDAT chunks of 2^32 - 5 bytes, FEND, AEND -- the bytes the reference writes for one entry."""
    parts = [np.frombuffer(pf.write_archive_header(), dtype=np.uint8),
             np.frombuffer(pf.write_chunk(b"FHED", pf.entry_header_bytes(0, pna.ALGO_DEFLATE, 0, 0, name)), dtype=np.uint8)]
    if raw_size is not None:
        parts.append(np.frombuffer(pf.write_chunk(b"fSIZ", struct.pack(">Q", raw_size)), dtype=np.uint8))
    for a in range(0, comp.size, CHUNK):
        body = comp[a:a + CHUNK]
        parts.append(np.frombuffer(struct.pack(">I", body.size) + b"FDAT", dtype=np.uint8))
        parts.append(body)
        parts.append(np.frombuffer(struct.pack(">I", zlib.crc32(body, zlib.crc32(b"FDAT")) & 0xFFFFFFFF), dtype=np.uint8))
    parts += [np.frombuffer(pf.write_chunk(b"FEND"), dtype=np.uint8), np.frombuffer(pf.finalize_archive(), dtype=np.uint8)]
    return np.concatenate(parts)


@pytest.mark.parametrize("fsiz", [True, False])
def test_d_reference_entry_beyond_4gib_compressed(big_ctx, pna, pf, stored_stream, fsiz):
    import torch
    raw, comp = stored_stream
    _need_hbm(torch, 80)
    arc = _reference_entry_archive(pf, pna, "big.bin", comp, raw.size if fsiz else None)
    assert arc.size > comp.size > CHUNK
    assert _extract(big_ctx, pna, arc) == [("big.bin", raw.size, hashlib.sha256(raw).digest())]
