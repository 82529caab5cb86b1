"""Single zstd frames of more than 4 GiB of COMPRESSED bytes, and with more than 4 GiB of Huffman-coded literals (the reference writes one frame per entry
and one per `--solid` archive, whatever the size: lib/src/compress/zstandard.rs, lib/src/archive/write.rs:443-470): the header walk (k_zscan, k_zparse_a) and
the literal scratch count in 64 bits, so such a frame is parsed a wave per block and executed by pointer jumping like any other large frame.
  (1) this library's frame (option single_frame) of 6 GiB of barely compressible data: known size, open size, damage behind compressed offset 2^32,
  (2) libzstd's frames of the same data: 4.5 GiB (below 4 GiB compressed, above 4 GiB of literals), 5 GiB and 6 GiB (above both),
  (3) the drivers on an archive whose entry is frame (1) -- its payload spans two FDAT chunks --: verify, extract-select to device memory, diff; and a
      solid archive of the same bytes, whose SDAT stream is one such frame without a content size, through extract.
Every context refuses the one-workgroup kernel (zdec_fallback_max_mib = 1): until the counters were widened these frames went there (~11 MiB/s: nine minutes
for 6 GiB) and every case here failed at once with PNA_E_UNSUPPORTED.

The data: every 1 MiB segment is 832 KiB of random 7-bit bytes followed by the segment's first 192 KiB again -- 7 bits per literal, and one long match per
segment for an encoder that looks 832 KiB back (0.71 of the input would remain).  Neither this library's level 1 nor libzstd's does: 0.875 of the input
remains (6 GiB -> 5 638 477 861 bytes here), all of it literals -- more than the cases need."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KIB, MIB, GIB = 1 << 10, 1 << 20, 1 << 30
LIT_KIB, REP_KIB = 832, 192


def _need_hbm(torch, gib):
    free, _ = torch.cuda.mem_get_info()
    assert free >= gib * GIB, f"the full-size case needs {gib} GiB of free HBM, found {free / GIB:.0f} GiB: an MI355X has 288 GB"


def _need_ram(gib):
    with open("/proc/meminfo") as f:
        avail = {k: int(v.split()[0]) for k, v in (ln.split(":", 1) for ln in f)}["MemAvailable"] << 10
    assert avail >= gib * GIB, f"the full-size case needs {gib} GiB of free host memory, found {avail / GIB:.0f} GiB"


def _recipe(torch, mib, seed, hi=128):
    """mib segments of 1 MiB on the device (a flat uint8 tensor)"""
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    d = torch.randint(0, hi, (mib, MIB), dtype=torch.uint8, device="cuda", generator=g)
    d[:, LIT_KIB * KIB:] = d[:, :REP_KIB * KIB]
    return d.view(-1)


def _own_frame(ctx, pna, torch, src):
    """src as ONE frame of this library at level 1 (device to device): the compressed bytes"""
    n = src.numel()
    cap = pna.bound(pna.ALGO_ZSTD, n) + 64
    comp = torch.empty(cap, dtype=torch.uint8, device="cuda")
    ctx.set_option("single_frame", 1)
    offs = ctx.compress_batch_device(src.data_ptr(), [0, n], [n], comp.data_ptr(), cap, level=1)
    ctx.set_option("single_frame", 0)
    assert offs[0] == 0
    out = comp[:offs[1]].clone()
    del comp
    torch.cuda.empty_cache()
    return out


def _zstd_open(ctx, d_src, src_len, d_dst, dst_cap):
    f = ctx._L.pna_gpu_zstd_decompress_open_device
    f.restype = ctypes.c_int
    f.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64,
                  ctypes.POINTER(ctypes.c_uint64), ctypes.c_void_p]
    raw = ctypes.c_uint64()
    ctx._check(f(ctx._h, ctypes.c_void_p(d_src), 0, src_len, ctypes.c_void_p(d_dst), 0, dst_cap, ctypes.byref(raw), None))
    return raw.value


def test_1_own_frame_beyond_4gib_compressed(big_ctx, pna):
    import torch
    ctx = big_ctx
    _need_hbm(torch, 100)
    mib = 6 * 1024
    src = _recipe(torch, mib, 21)
    n = src.numel()
    comp = _own_frame(ctx, pna, torch, src)
    comp_len = comp.numel()
    print(f"6 GiB -> {comp_len} compressed bytes ({comp_len / n:.4f}), at least {mib * LIT_KIB * KIB} literal bytes")
    assert comp_len > 2 ** 32                                          # conditions of the test: both old counters overflow
    assert mib * LIT_KIB * KIB > 2 ** 32                               # (the random part of every segment can only be literals)
    assert comp[:4].cpu().numpy().tobytes() == bytes.fromhex("28b52ffd")
    ctx.set_option("zdec_fallback_max_mib", 1)
    out = torch.zeros(n + 64, dtype=torch.uint8, device="cuda")
    ctx.decompress_batch_device(comp.data_ptr(), [0], [comp_len], out.data_ptr(), [0], [n])
    assert torch.equal(out[:n], src)
    # the open forms: the size from the frame's block headers (no content size in this library's frames: a bound), then the decode into that room
    size, exact = ctx.open_size_device(comp.data_ptr(), 0, comp_len)
    assert n <= size <= 2 * n and not exact
    out = None
    out = torch.zeros(size + 64, dtype=torch.uint8, device="cuda")
    assert _zstd_open(ctx, comp.data_ptr(), comp_len, out.data_ptr(), size) == n
    assert torch.equal(out[:n], src)
    # one byte behind compressed offset 2^32 flipped: refused, or other bytes -- never a fault
    at = 2 ** 32 + 300 * MIB + 12345
    assert 2 ** 32 < at < comp_len - 8
    comp[at] ^= 0x10
    out.zero_()
    try:
        ctx.decompress_batch_device(comp.data_ptr(), [0], [comp_len], out.data_ptr(), [0], [n])
        same = torch.equal(out[:n], src)
    except pna.PnaGpuError as e:
        assert e.code == pna.E_INVAL, e
        same = False
    assert not same


@pytest.mark.parametrize("mib", [4608, 5120, 6144])
def test_2_foreign_frame(big_ctx, pna, codec, mib):
    """libzstd at level 1 (its own tables per block, repeat codes), one ZSTD_compress call.  Its window for inputs of this size is 512 KiB (asserted from the
    frame header), so the segment's repeat, 832 KiB back, is out of its reach and every byte is a literal: the frames are 0.875 of their content, not the 0.71
    the recipe was made for -- measured on an MI355X box: 5 GiB -> 4 698 398 799 bytes.  So 5 GiB and 6 GiB both exceed BOTH old limits (4 GiB of compressed
    bytes, 4 GiB of literals); the frame below the compressed limit and above the literal limit is the one of 4.5 GiB (about 3.94 GiB compressed)."""
    import torch
    Z = codec.system_libzstd()
    if Z is None:
        pytest.skip("system libzstd (the writer of the test frame) is absent")
    ctx = big_ctx
    _need_hbm(torch, 100)
    _need_ram(24)
    src = _recipe(torch, mib, 30 + mib // 1024)
    n = src.numel()
    host = src.cpu().numpy()
    cap = Z.ZSTD_compressBound(n)
    buf = np.empty(cap, dtype=np.uint8)
    k = Z.ZSTD_compress(buf.ctypes.data, cap, ctypes.c_char_p(host.ctypes.data), n, 1)
    assert not Z.ZSTD_isError(k)
    del host
    fhd = int(buf[4])
    assert (fhd >> 6) == 3 and not (fhd >> 5) & 1                       # one frame with an 8-byte Frame_Content_Size behind a window descriptor
    wd = int(buf[5])
    window = (1 << (10 + (wd >> 3))) + ((1 << (10 + (wd >> 3))) >> 3) * (wd & 7)
    print(f"{mib} MiB -> {k} compressed bytes ({k / n:.4f}), window {window >> 10} KiB")
    # conditions of the test: no match reaches the segment's repeat, so the content (more than 4 GiB) is literals; the compressed size is on its side of 2^32
    assert window <= LIT_KIB * KIB and n > 2 ** 32
    assert (k > 2 ** 32) == (mib > 4608)
    comp = torch.from_numpy(buf[:k]).cuda()
    del buf
    ctx.set_option("zdec_fallback_max_mib", 1)
    out = torch.zeros(n + 64, dtype=torch.uint8, device="cuda")
    ctx.decompress_batch_device(comp.data_ptr(), [0], [k], out.data_ptr(), [0], [n])
    assert torch.equal(out[:n], src)


def _host_call(fn, ctx, pna, algo, level, names, views):
    parts = []

    def _sink(_u, buf, k):
        parts.append(np.ctypeslib.as_array(ctypes.cast(buf, ctypes.POINTER(ctypes.c_ubyte)), shape=(k,)).copy())
        return 0
    scb = pna.SINK_FN(_sink)
    k = len(views)
    a_names = (ctypes.c_char_p * k)(*[s.encode() for s in names])
    a_src = (ctypes.c_void_p * k)(*[v.ctypes.data for v in views])
    a_len = (ctypes.c_size_t * k)(*[len(v) for v in views])
    ctx._check(fn(ctx._h, algo, level, k, a_names, a_src, a_len, scb, None))
    return np.concatenate(parts)


def _chunk_kinds(arc):
    """(type, length) of every chunk of an archive image"""
    pos, out = 8, []
    while pos < arc.size:
        ln = int.from_bytes(arc[pos:pos + 4].tobytes(), "big")
        out.append((arc[pos + 4:pos + 8].tobytes(), ln))
        pos += 12 + ln
    return out


def test_3_drivers(big_ctx, pna):
    import torch
    ctx = big_ctx
    _need_hbm(torch, 120)
    _need_ram(48)
    mib = 6 * 1024
    src = _recipe(torch, mib, 21)
    n = src.numel()
    host = src.cpu().numpy()
    ctx.set_option("zdec_fallback_max_mib", 1)
    # ---- one entry, one frame, through the host pipeline: the payload is cut into two FDAT chunks
    ctx.set_option("single_frame", 1)
    arc = _host_call(ctx._L.pna_gpu_create_archive_host, ctx, pna, pna.ALGO_ZSTD, 1, ["big/one.bin"], [host])
    kinds = _chunk_kinds(arc)
    fdat = [ln for ty, ln in kinds if ty == b"FDAT"]
    assert len(fdat) == 2 and sum(fdat) > 2 ** 32, kinds
    image = arc.tobytes()
    del arc
    recs, s = pna.verify_archive(ctx, image)
    assert s["rc"] == 0 and [(r[0], r[2], r[4]) for r in recs] == [("big/one.bin", pna.VERIFY_OK, n)], recs
    dst = torch.zeros(n, dtype=torch.uint8, device="cuda")
    recs, s = pna.extract_select(ctx, image, lambda i, name, kind, stored: dst)
    assert [(r[1], r[3], r[5]) for r in recs] == [("big/one.bin", pna.EXTRACT_OK, n)], recs
    assert torch.equal(dst, src)
    del dst
    recs, s = pna.diff_archive(ctx, image, lambda i, p, k, st: (pna.DIFF_FS_FILE, (host.ctypes.data, n)))
    assert [(r.name, r.status, r.first_diff, r.size) for r in recs] == [("big/one.bin", pna.DIFF_SAME, None, n)], recs
    del image
    # ---- the same bytes as a solid archive of twelve inner entries: the SDAT stream is ONE frame without a content size
    step = 512 * MIB
    views = [host[a:a + step] for a in range(0, n, step)]
    names = [f"solid/{i:02d}.bin" for i in range(len(views))]
    arc = _host_call(ctx._L.pna_gpu_create_solid_archive_host, ctx, pna, pna.ALGO_ZSTD, 1, names, views)
    ctx.set_option("single_frame", 0)
    assert sum(ln for ty, ln in _chunk_kinds(arc) if ty == b"SDAT") > 2 ** 32
    seen = []

    def _cb(_u, idx, name, kind, data, k):
        got = np.ctypeslib.as_array(ctypes.cast(data, ctypes.POINTER(ctypes.c_ubyte)), shape=(k,)) if k else host[:0]
        seen.append((name.decode(), k, k == len(views[idx]) and bool(np.array_equal(got, views[idx]))))
        return 0
    cb = pna.ENTRY_FN(_cb)
    ctx._check(ctx._L.pna_gpu_extract_archive_host(ctx._h, arc.ctypes.data_as(ctypes.c_char_p), arc.size, None, 0, cb, None))
    assert seen == [(nm, len(v), True) for nm, v in zip(names, views)]
