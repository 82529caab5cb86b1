"""Compression::XZ on the write side (option xz_encode), in every form of the call that tests/test_gpu_xz_encode.py does not run: many small entries (the
write kernel's wave-per-block form, the short segments' geometries of the LZ stage, block sizes chosen from the longest entry), a call cut into several
sub-batches, the forms of the LZ stage behind the coder, forced and latency-mode block sizes, every level set byte for byte, the CRC kernel's piece counts,
CBC and GCM around the payloads, and a zstd / deflate call on a context that has just written xz.  The references are those of test_gpu_xz_encode.py:
liblzma (which verifies the CRC64 as well), the library's own decoder, and the encoder core on the CPU over the oracle's LZ model (xz_enc_cases.cpu_stream_of)
-- every comparison byte for byte."""
import hashlib
import lzma
import random

import pytest

import xz_enc_cases as E
from conftest import headline_context
from xz_enc_cases import _check_archive, _entries

pytestmark = pytest.mark.gpu

PHSF = "$pbkdf2-sha256$i=1000,l=32$c2FsdHNhbHRzYWx0"
NAMED_SIZES = [0, 1, 2, 3, 5, 63, 64, 255, 256, 257, 4095, 4096, 4097, 8191, 8192, 8193, 16383, 16384, 16385, 32767, 32768]


@pytest.fixture(scope="module")
def ctx(pna):
    """the headline form (latency mode off) with the option: 64 KiB blocks unless the entries are short or the test says otherwise"""
    import torch  # noqa: F401  (shares its HIP runtime with the extension)
    c = headline_context(pna)
    c.set_option("xz_encode", 1)
    yield c
    c.close()


def _checked(pna, ctx, datas, outs, level=6, blk_log=None, equal=(), decode=None, **model):
    """liblzma decodes every stream to its entry and every stream fits its bound; the device decodes entries `decode` (all by default); entries `equal` are
    the CPU core's bytes at `blk_log`"""
    assert len(outs) == len(datas)
    for i, (d, o) in enumerate(zip(datas, outs)):
        assert lzma.decompress(o, format=lzma.FORMAT_XZ) == d, i
        assert len(o) <= pna.bound(pna.ALGO_XZ, len(d)), i
    idx = list(range(len(datas))) if decode is None else list(decode)
    assert ctx.decompress_batch([outs[i] for i in idx], [len(datas[i]) for i in idx], algo=pna.ALGO_XZ) == [datas[i] for i in idx]
    bad = [i for i in equal if outs[i] != E.cpu_stream_of(datas[i], level, blk_log, **model)]
    assert not bad, (bad[:8], [len(datas[i]) for i in bad[:8]], blk_log, model)


@pytest.fixture(scope="module")
def small_entries(codec):
    """text, one repeated byte, noise, empty: the named sizes -- around every power of two up to 32 KiB --, then 4 200 random sizes below 9 000, a few of 12 000"""
    rnd = random.Random(11)
    sizes = NAMED_SIZES + [12000 if rnd.random() < 0.01 else rnd.choice((rnd.randrange(1, 700), rnd.randrange(700, 9000), 4096)) for _ in range(4200)]
    ents = []
    for i, n in enumerate(sizes):
        k = i % 5
        if k == 3:
            ents.append(bytes([97 + i % 5]) * n)
        elif k == 4:
            ents.append(rnd.randbytes(n))
        else:
            ents.append(codec.corpus_file(k & 1, 900 + i, n) if n else b"")
    return ents


def _sample(n):
    return sorted(set(range(len(NAMED_SIZES))) | set(range(0, n, 7)))


@pytest.fixture(scope="module")
def small_streams(pna, ctx, small_entries):
    """the batch of many small entries, compressed once: (streams, the block size the call reported)"""
    outs = ctx.compress_batch(small_entries, algo=pna.ALGO_XZ)
    return outs, ctx.timing().blk_log


def test_many_small_entries(pna, ctx, small_entries, small_streams):
    """At least 4 096 segments, none above 32 KiB: the write kernel runs a wave per block (its three small jobs on thread 0), the segments of at most 4 KiB
    and 16 KiB run the short geometries of the match finder, and the block size is the power of two that holds the longest entry: 32 KiB."""
    outs, blk_log = small_streams
    assert blk_log == 15
    _checked(pna, ctx, small_entries, outs, blk_log=15, equal=_sample(len(outs)), decode=range(600))


def test_many_small_entries_of_at_most_4k(pna, ctx, small_entries):
    """the same entries cut at 4 096 bytes: 8 KiB blocks, and every segment is of the shortest geometry -- no launch of the large one"""
    ents = [e[:4096] for e in small_entries]
    outs = ctx.compress_batch(ents, algo=pna.ALGO_XZ)
    assert ctx.timing().blk_log == 13
    _checked(pna, ctx, ents, outs, blk_log=13, equal=_sample(len(outs)), decode=range(600))


def test_many_small_entries_device_batch_guard_bands(pna, ctx, small_entries, small_streams):
    """compress_batch_device over the same entries at 16-byte strides: nothing outside [0, total) of the destination is written, the offsets rise, and
    [offs[i], offs[i + 1]) is entry i's stream -- the one the host form returned"""
    import torch
    ents, (outs, _) = small_entries, small_streams
    offs, pos = [], 0
    for e in ents:
        offs.append(pos)
        pos = (pos + len(e) + 15) & ~15
    src = torch.frombuffer(bytearray(b"".join(e + bytes(-len(e) % 16) for e in ents) + bytes(64)), dtype=torch.uint8).cuda()
    cap = sum(pna.bound(pna.ALGO_XZ, len(e)) for e in ents) + 16
    G = 4096
    dst = torch.full((G + cap + G,), 0xA5, dtype=torch.uint8, device="cuda")
    o = ctx.compress_batch_device(src.data_ptr(), offs, [len(e) for e in ents], dst.data_ptr() + G, cap, algo=pna.ALGO_XZ)
    assert ctx.timing().blk_log == 15
    host = dst.cpu().numpy().tobytes()
    assert len(o) == len(ents) + 1 and o[0] == 0 and all(a < b for a, b in zip(o, o[1:])) and o[-1] <= cap
    assert host[:G] == b"\xA5" * G and host[G + o[-1]:] == b"\xA5" * (len(host) - G - o[-1])
    got = [host[G + a:G + b] for a, b in zip(o, o[1:])]
    sample = _sample(len(ents))
    _checked(pna, ctx, [ents[i] for i in sample], [got[i] for i in sample], blk_log=15, decode=range(0, len(sample), 5))
    assert got == outs


def test_many_small_entries_archive(pna, pf, ctx, small_entries):
    """create_archive over the entries of at most 4 KiB: the framing kernel's wave-per-entry form over xz payloads"""
    ents = [e[:4096] for e in small_entries]
    names = ["s/%05d" % i for i in range(len(ents))]
    arc = pna.create_archive(ctx, names, ents, algo=pna.ALGO_XZ)
    got = pna.extract_archive(ctx, arc)
    assert [n for n, _, _ in got] == names and [d for _, _, d in got] == ents
    _, items = pf.read_archive(arc)
    assert [(it.name, it.compression, it.raw_file_size) for it in items] == [(n, pna.ALGO_XZ, len(e)) for n, e in zip(names, ents)]
    for i in _sample(len(ents)):
        assert lzma.decompress(items[i].data, format=lzma.FORMAT_XZ) == ents[i], i


def _corpus_entries(ctx, first_file, n):
    """n entries of 1 MiB of the device's corpus, on the host"""
    import torch
    L = 1 << 20
    src = torch.empty(n * L + 8192, dtype=torch.uint8, device="cuda")
    ctx.corpus_fill_device(0, first_file, n, L, L, src.data_ptr())
    host = src[:n * L].cpu().numpy()
    return [host[i * L:(i + 1) * L].tobytes() for i in range(n)]


def test_several_sub_batches(pna, ctx):
    """A call cut into pieces of at most 16 MiB -- the host batch by batch_piece_mib, the archive pipeline by sub_mib: three at least -- writes what the call in
    one piece writes.  Among the 1 MiB entries an empty one, a short one and one of two segments (its Index is sized by a walk back to the entry's first
    segment, which is not the sub-batch's first)."""
    ents = _corpus_entries(ctx, 2300, 40)
    ents[5], ents[6], ents[20] = b"", ents[6][:12345], ents[20] + ents[21][:100]
    names = ["p/%04d" % i for i in range(len(ents))]
    with ctx.options(sub_mib=(16, 256), batch_piece_mib=(16, 256)):
        cut = ctx.compress_batch(ents, algo=pna.ALGO_XZ)
        arc_cut = pna.create_archive(ctx, names, ents, algo=pna.ALGO_XZ)
    whole = ctx.compress_batch(ents, algo=pna.ALGO_XZ)
    assert ctx.timing().blk_log == 16
    assert cut == whole
    cuts, acc = [], 0                                                   # the first entries of the pieces: a piece takes entries while they fit 16 MiB
    for i, e in enumerate(ents):
        if acc and acc + len(e) > (16 << 20):
            cuts.append(i)
            acc = 0
        acc += len(e)
    assert len(cuts) >= 2
    _checked(pna, ctx, ents, cut, blk_log=16, equal=sorted({5, 6, 20} | {i - 1 for i in cuts} | set(cuts)))
    assert arc_cut == pna.create_archive(ctx, names, ents, algo=pna.ALGO_XZ)
    recs, summ = pna.verify_archive(ctx, arc_cut)
    assert summ["rc"] == 0 and len(recs) == len(names) and all(r[2] == pna.VERIFY_OK for r in recs)


FORM_NAMES = ["text1m12345", "rep_cycle", "random_then_text", "text65537"]


@pytest.mark.parametrize("form", ["lz_split=0", "lz_split=2", "unit_log=14", "mtile=512", "fused"])
def test_lz_stage_forms(pna, ctx, form):
    """The forms of the LZ stage are bit-exact with the model, so behind each of them the coder writes the CPU core's bytes (mtile: the model's with the same
    mtile).  A form that let a match above 273 bytes through would still decode -- the coder cuts it -- and differ here."""
    datas = [dict(E.inputs())[n] for n in FORM_NAMES]
    every = range(len(datas))
    if form == "fused":
        c = headline_context(pna, flags=pna.F_STD | pna.F_LZ_FUSED)
        try:
            c.set_option("xz_encode", 1)
            outs = c.compress_batch(datas, algo=pna.ALGO_XZ)
            assert c.timing().blk_log == 16
            _checked(pna, c, datas, outs, blk_log=16, equal=every)
        finally:
            c.close()
        return
    name, value = form.split("=")
    restore = {"lz_split": 1, "unit_log": 0, "mtile": 0}[name]
    with ctx.options(**{name: (int(value), restore)}):
        outs = ctx.compress_batch(datas, algo=pna.ALGO_XZ)
        t = ctx.timing()
        assert t.blk_log == 16
        # (the form ran: the one-kernel LZ stage launches no match kernel, the split forms do; the option's units are reported)
        assert (t.lz_match_launches == 0) == (form in ("lz_split=0", "unit_log=14")) and (t.lz_units > 0) == (form == "unit_log=14"), (t.lz_match_launches, t.lz_units)
    _checked(pna, ctx, datas, outs, blk_log=16, equal=every, **({"mtile": 512} if name == "mtile" else {}))


@pytest.mark.parametrize("forced,reported", [(14, 14), (15, 15), (17, 16)])
def test_forced_block_sizes(pna, ctx, forced, reported):
    """option blk_log: 16 and 32 KiB chunks; 128 KiB is no LZMA2 chunk, the call runs 64 KiB and says so"""
    datas = [dict(E.inputs())[n] for n in ("text65537", "rep_cycle", "random_then_text", "near_stored", "forty", "empty")]
    with ctx.options(blk_log=(forced, 0)):
        outs = ctx.compress_batch(datas, algo=pna.ALGO_XZ)
        assert ctx.timing().blk_log == reported
    _checked(pna, ctx, datas, outs, blk_log=reported, equal=range(len(datas)))


def test_latency_mode_32k_blocks(pna, ctx):
    """A context with the library's defaults: above 32 MiB of input the latency mode cuts 32 KiB blocks (16 KiB below, tests/test_gpu_xz_encode.py).  The
    streams are those of a forced block size with the latency mode off, and the CPU core's."""
    ents = _corpus_entries(ctx, 4100, 33)
    c = pna.Context(0)
    try:
        c.set_option("xz_encode", 1)
        with c.options(latency_max_mib=(64, 128)):
            outs = c.compress_batch(ents, algo=pna.ALGO_XZ)
            assert c.timing().blk_log == 15
    finally:
        c.close()
    with ctx.options(blk_log=(15, 0)):
        forced = ctx.compress_batch(ents, algo=pna.ALGO_XZ)
        assert ctx.timing().blk_log == 15
    assert outs == forced
    _checked(pna, ctx, ents, outs, blk_log=15, equal=(0, 32), decode=(0, 16, 32))


@pytest.mark.parametrize("level", [0, 3, 9])
def test_levels_byte_exact(pna, ctx, level):
    datas = [dict(E.inputs())["rep_cycle"], dict(E.inputs())["text1m12345"][:300000]]
    outs = ctx.compress_batch(datas, algo=pna.ALGO_XZ, level=level)
    _checked(pna, ctx, datas, outs, level=level, blk_log=16, equal=(0, 1))


def test_far_distances_at_level_9(pna, ctx):
    """level 9, the LZ set whose offsets span the segment: distances beyond 2^19 -- slots 38 and 39, 19 direct bits -- through the device's coder"""
    d = E.far()
    (o,) = ctx.compress_batch([d], algo=pna.ALGO_XZ, level=9)
    _checked(pna, ctx, [d], [o], level=9, blk_log=16, equal=(0,))
    ev = E.events(o)
    assert ev.data == d and ev["slot38"] + ev["slot39"] >= 1 and ev["len273"] >= 1


@pytest.mark.parametrize("pieces,lengths", [(1, (1023, 1024, 1025, 262143, 262144)),
                                            (2, (1023, 1024, 1025, 262143, 262144, 262145, 524288)),
                                            (4, (1023, 1024, 1025, 262143, 262144, 262145, 524289, (1 << 20) - 1, 1 << 20, (1 << 20) + 1))])
def test_crc64_piece_edges(pna, ctx, pieces, lengths):
    """The CRC kernel takes a segment in pieces of 256 KiB, a thread per KiB, as many pieces per segment as the batch's longest segment has: lengths on both
    sides of a thread's KiB and of a piece, in batches of one, two and four pieces per segment.  liblzma verifies every block's CRC64."""
    assert (min(max(lengths), 1 << 20) + (256 << 10) - 1) // (256 << 10) == pieces
    text = dict(E.inputs())["text1m12345"]
    datas = [text[7 * i:7 * i + n] for i, n in enumerate(lengths)]
    outs = ctx.compress_batch(datas, algo=pna.ALGO_XZ)
    _checked(pna, ctx, datas, outs, blk_log=16, equal=range(len(datas)))
    for d, o in zip(datas, outs):
        recs, check = E.index_records(o)
        assert check == lzma.CHECK_CRC64 and [u for _, u in recs] == [min(E.SEG, len(d) - s) for s in range(0, len(d), E.SEG)]


@pytest.mark.parametrize("mode_name", ["cbc", "gcm"])
def test_archive_aes_cbc_and_gcm(pna, pf, codec, ctx, mode_name):
    mode = pna.MODE_CBC if mode_name == "cbc" else pna.MODE_GCM
    names, ents = _entries()
    key = hashlib.pbkdf2_hmac("sha256", b"password", b"saltsaltsalt", 1000, 32)
    arc = pna.create_archive_encrypted(ctx, names, ents, b"password", algo=pna.ALGO_XZ, cipher=pna.Cipher(key, PHSF, mode))
    items = _check_archive(pna, pf, codec, ctx, arc, names, ents, b"password")
    assert all(it.encryption == pna.ENC_AES and it.cipher_mode == mode for it in items)


def test_archive_aes_ctr_device_equals_host(pna, pf, codec, ctx):
    """the device-resident encrypted entry point with the caller's IVs: the host form's archive"""
    import torch
    names, ents = _entries()
    key = hashlib.pbkdf2_hmac("sha256", b"password", b"saltsaltsalt", 1000, 32)
    ci = pna.Cipher(key, PHSF, pna.MODE_CTR, ivs=bytes(range(16 * len(ents))))
    arc = pna.create_archive_encrypted(ctx, names, ents, b"password", algo=pna.ALGO_XZ, cipher=ci)
    _check_archive(pna, pf, codec, ctx, arc, names, ents, b"password")
    offs, pos = [], 0
    for e in ents:
        offs.append(pos)
        pos = (pos + len(e) + 15) & ~15
    src = torch.frombuffer(bytearray(b"".join(e + bytes(-len(e) % 16) for e in ents) + bytes(64)), dtype=torch.uint8).cuda()
    cap = pna.archive_enc_bound(pna.ALGO_XZ, names, [len(e) for e in ents], ci)
    dst = torch.full((cap + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    total, _ = ctx.create_archive_device(names, src.data_ptr(), offs, [len(e) for e in ents], dst.data_ptr(), cap, algo=pna.ALGO_XZ, cipher=ci)
    assert dst[:total].cpu().numpy().tobytes() == arc
    assert dst[cap:].cpu().numpy().tobytes() == b"\xA5" * 64


def test_zstd_and_deflate_after_xz(pna, codec, ctx):
    """xz caps a call's LZ blocks at 64 KiB and its matches at 273 bytes; neither outlives the call: the next zstd and deflate calls on the context write the
    model's default bytes, on 128 KiB blocks"""
    import zlib
    datas = [dict(E.inputs())[n] for n in ("text1m12345", "zeros2m1", "abab", "text5k", "empty")]
    outs = ctx.compress_batch(datas, algo=pna.ALGO_XZ)
    assert ctx.timing().blk_log == 16
    _checked(pna, ctx, datas, outs, blk_log=16, equal=range(len(datas)))
    z = ctx.compress_batch(datas)
    assert ctx.timing().blk_log == 17
    p = codec.params_for_level(3)
    for d, o in zip(datas, z):
        assert o == codec.model_compress(d, p) and codec.zstd_decompress(o, len(d)) == d
    f = ctx.compress_batch(datas, algo=pna.ALGO_DEFLATE)
    for d, o in zip(datas, f):
        assert o == codec.deflate_model_compress(d) and zlib.decompress(o) == d
