"""Compression::XZ on the write side (option xz_encode): .xz streams written on the device -- one block per 1 MiB segment, one LZMA2 chunk per LZ block.
The references: liblzma (the stdlib's lzma module) decodes every stream; the library's own device decoder does; and the bytes equal those of the encoder
core on the CPU (csrc/xz_enc_core.h, tests/xz_enc_cases.py) over the sequences of the oracle's LZ model for the same level and block size -- the device's
LZ stage is bit-exact with that model, so any difference is the new kernels'.  Every test that sets the option fails without the encoder: the option's
name is PNA_E_INVAL there."""
import hashlib
import io
import lzma

import pytest

import xz_enc_cases as E
from xz_enc_cases import _check_archive, _entries

pytestmark = pytest.mark.gpu

NAMES = [n for n, _ in E.inputs()]
PHSF = "$pbkdf2-sha256$i=1000,l=32$c2FsdHNhbHRzYWx0"


@pytest.fixture(scope="module")
def ctx(pna):
    """64 KiB and 8 KiB blocks whatever the batch: the latency mode off, the block size set per test"""
    import torch  # noqa: F401  (shares its HIP runtime with the extension)
    c = pna.Context(0)
    c.set_option("latency_max_mib", 0)
    c.set_option("xz_encode", 1)
    yield c
    c.close()


@pytest.fixture(scope="module")
def plain_ctx(pna):
    """the library's defaults (latency mode included) with the option"""
    import torch  # noqa: F401
    c = pna.Context(0)
    c.set_option("xz_encode", 1)
    yield c
    c.close()


@pytest.mark.parametrize("blk_log", [16, 13])
def test_batch_decodes_and_equals_the_cpu_core(pna, ctx, blk_log):
    datas = [d for _, d in E.inputs()]
    ctx.set_option("blk_log", blk_log)
    try:
        outs = ctx.compress_batch(datas, algo=pna.ALGO_XZ)
        assert ctx.timing().blk_log == blk_log
        back = ctx.decompress_batch(outs, [len(d) for d in datas], algo=pna.ALGO_XZ)
    finally:
        ctx.set_option("blk_log", 0)
    for (name, d), o, b in zip(E.inputs(), outs, back):
        assert lzma.decompress(o, format=lzma.FORMAT_XZ) == d, name
        assert b == d, name
        assert len(o) <= pna.bound(pna.ALGO_XZ, len(d)), name
        recs, check = E.index_records(o)
        assert len(recs) == (len(d) + E.SEG - 1) // E.SEG and check == lzma.CHECK_CRC64, name
        assert o == E.cpu_stream(name, 6, blk_log), name
        for control, usize, cost in E.chunks(o):                        # (what the bound counts: no chunk takes more than its stored form)
            assert cost <= 3 + usize and (control >= 0x80) == (cost < 3 + usize), (name, hex(control), usize, cost)
    if blk_log == 13:                                                   # "near_stored" is at the edge between the two kinds of chunk, on both sides of it
        cs = E.chunks(outs[NAMES.index("near_stored")])
        assert any(c < 0x80 for c, _, _ in cs) and any(c >= 0x80 and cost >= u for c, u, cost in cs)


def test_plain_context_latency_mode(pna, plain_ctx):
    """a small batch on a context with the library's defaults: latency mode's blocks of 16 KiB (zstd's choice below 32 MiB of input), and the bytes are the
    CPU core's at that block size"""
    names = ["empty", "forty", "text5k", "text65537", "random_then_text", "near_stored"]
    datas = [dict(E.inputs())[n] for n in names]
    outs = plain_ctx.compress_batch(datas, algo=pna.ALGO_XZ)
    blk_log = plain_ctx.timing().blk_log
    assert blk_log == 14
    for name, d, o in zip(names, datas, outs):
        assert lzma.decompress(o, format=lzma.FORMAT_XZ) == d, name
        assert o == E.cpu_stream(name, 6, blk_log), name
    assert plain_ctx.decompress_batch(outs, [len(d) for d in datas], algo=pna.ALGO_XZ) == datas


@pytest.mark.parametrize("level", [0, 3, 6, 9])
def test_levels(pna, ctx, level):
    d = dict(E.inputs())["text1m12345"][:300000]
    (o,) = ctx.compress_batch([d], algo=pna.ALGO_XZ, level=level)
    assert lzma.decompress(o, format=lzma.FORMAT_XZ) == d
    assert ctx.decompress_batch([o], [len(d)], algo=pna.ALGO_XZ) == [d]


def test_level_scale(pna):
    """lib/src/compress/xz.rs:36-46: default 6, 0 .. 9"""
    assert [pna.clamp_level(pna.ALGO_XZ, lv) for lv in (pna.LEVEL_DEFAULT, -5, 0, 4, 9, 10, 100)] == [6, 0, 0, 4, 9, 9, 9]
    assert 32 <= pna.bound(pna.ALGO_XZ, 0) <= 64                                         # (an empty entry's stream is 32 bytes)
    n = (3 << 20) + 5
    assert pna.bound(pna.ALGO_XZ, n) >= n + 3 * ((n + 8191) // 8192) + 3 * 24 + 3 * 8 + 32 + 1


def test_device_batch_guard_bands(pna, ctx):
    """compress_batch_device, entries at offsets 0 and 16: nothing outside [0, total) of d_dst is written; entry i's stream is [off[i], off[i + 1])"""
    import torch
    a, b = dict(E.inputs())["three"] + b"0123456789abc", dict(E.inputs())["text65537"]
    assert len(a) == 16
    src = torch.frombuffer(bytearray(a + b + bytes(64)), dtype=torch.uint8).cuda()
    cap = pna.bound(pna.ALGO_XZ, len(a)) + pna.bound(pna.ALGO_XZ, len(b)) + 16
    G = 4096
    dst = torch.full((G + cap + G,), 0xA5, dtype=torch.uint8, device="cuda")
    offs = ctx.compress_batch_device(src.data_ptr(), [0, 16], [len(a), len(b)], dst.data_ptr() + G, cap, algo=pna.ALGO_XZ)
    host = dst.cpu().numpy().tobytes()
    assert host[:G] == b"\xA5" * G and host[G + offs[2]:] == b"\xA5" * (len(host) - G - offs[2])
    assert lzma.decompress(host[G + offs[0]:G + offs[1]]) == a
    assert lzma.decompress(host[G + offs[1]:G + offs[2]]) == b


def test_archive_plain_host_and_device(pna, pf, codec, ctx):
    import torch
    names, ents = _entries()
    arc = pna.create_archive(ctx, names, ents, algo=pna.ALGO_XZ)
    _check_archive(pna, pf, codec, ctx, arc, names, ents)
    offs, pos = [], 0
    for e in ents:
        offs.append(pos)
        pos = (pos + len(e) + 15) & ~15
    src = torch.frombuffer(bytearray(b"".join(e + bytes(-len(e) % 16) for e in ents) + bytes(64)), dtype=torch.uint8).cuda()
    cap = pna.archive_bound(pna.ALGO_XZ, names, [len(e) for e in ents])
    dst = torch.full((cap + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    total, _ = ctx.create_archive_device(names, src.data_ptr(), offs, [len(e) for e in ents], dst.data_ptr(), cap, algo=pna.ALGO_XZ)
    dev = dst[:total].cpu().numpy().tobytes()
    assert dev == arc                                                                   # (both forms write the same archive)
    assert dst[cap:].cpu().numpy().tobytes() == b"\xA5" * 64


def test_archive_aes_ctr(pna, pf, codec, ctx):
    names, ents = _entries()
    key = hashlib.pbkdf2_hmac("sha256", b"password", b"saltsaltsalt", 1000, 32)
    arc = pna.create_archive_encrypted(ctx, names, ents, b"password", algo=pna.ALGO_XZ, cipher=pna.Cipher(key, PHSF, pna.MODE_CTR))
    items = _check_archive(pna, pf, codec, ctx, arc, names, ents, b"password")
    assert all(it.encryption == pna.ENC_AES and it.cipher_mode == pna.MODE_CTR for it in items)


def test_archive_chunked(pna, pf, codec, ctx):
    """max_chunk_size below a payload: the stream is cut into FDAT chunks anywhere, xz knows nothing of it"""
    names, ents = _entries()
    arc = pna.create_archive_chunked(ctx, names, ents, 3000, algo=pna.ALGO_XZ)
    items = _check_archive(pna, pf, codec, ctx, arc, names, ents)
    assert max(len(d) for it in items for ty, d in it.chunks if ty == b"FDAT") == 3000
    assert sum(1 for ty, _ in items[2].chunks if ty == b"FDAT") > 10


def test_refusals(pna, ctx):
    d = dict(E.inputs())["text5k"]
    plain = pna.Context(0)
    try:
        for call in (lambda c: c.compress_batch([d], algo=pna.ALGO_XZ), lambda c: pna.create_archive(c, ["a"], [d], algo=pna.ALGO_XZ)):
            with pytest.raises(pna.PnaGpuError) as ei:                                   # without the option: as before
                call(plain)
            assert ei.value.code == pna.E_UNSUPPORTED
    finally:
        plain.close()
    solid = [lambda: pna.create_archive(ctx, ["a"], [d], algo=pna.ALGO_XZ, solid=True),
             lambda: ctx.create_solid_archive_enc_host(["a"], [d], algo=pna.ALGO_XZ),
             lambda: ctx.compress_solid(d, algo=pna.ALGO_XZ),
             lambda: ctx.writer(io.BytesIO(), algo=pna.ALGO_XZ)]
    for call in solid:                                                                   # with it: the solid entry points and the facade still refuse
        with pytest.raises(pna.PnaGpuError) as ei:
            call()
        assert ei.value.code == pna.E_UNSUPPORTED
    with pytest.raises(pna.PnaGpuError) as ei:
        ctx.set_option("xz_encode", 2)
    assert ei.value.code == pna.E_INVAL
