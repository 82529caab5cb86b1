"""Compression::XZ on the read side: .xz streams (LZMA2) decoded on the device -- the batch decoder, the open decoder, the size measurement, and
the extract / verify / diff / select drivers over archives with xz entries.  The reference is liblzma (the stdlib's lzma module), the decoder the
reference itself links.

Fixtures: tests/golden/xz.pna and solid_xz.pna are byte copies of the reference's resources/test archives (CRC64, LZMA2, 8 MiB dictionary, no fSIZ).
tests/golden/xz/mb4.xz and mb4_t2.xz are multi-block streams, which the stdlib module cannot write: made with the xz 5.2.5 tool from
codec.corpus_file(0, 7, 120000) by `xz -6 --block-size=32768` (4 blocks, no sizes in the block headers) and `xz -1 -T2 --block-size=32768` (block
headers that carry both sizes); their expected bytes come from codec.corpus_file, not from a file.  Everything else is made here with lzma."""
import lzma
import zlib

import pytest

import xz_cases as X
from conftest import golden

pytestmark = pytest.mark.gpu

PW = b"password"


@pytest.fixture(scope="module")
def ctx(pna):
    import torch  # noqa: F401  (shares its HIP runtime with the extension)
    c = pna.Context(0)
    yield c
    c.close()


def to_device(blobs):
    """the blobs behind each other at 16-byte strides in one device tensor: (tensor, offsets)"""
    import torch
    offs, at = [], 0
    for b in blobs:
        offs.append(at)
        at += (len(b) + 15) & ~15
    host = bytearray(max(at, 16))
    for o, b in zip(offs, blobs):
        host[o:o + len(b)] = b
    return torch.frombuffer(host, dtype=torch.uint8).cuda(), offs


def test_streams_in_one_batch(pna, ctx):
    """every stream of the list through ONE decompress_batch call: each equals its input"""
    cases = X.streams()
    outs = ctx.decompress_batch([s for _, s, _ in cases], [len(d) for _, _, d in cases], algo=pna.ALGO_XZ)
    for (name, _, d), o in zip(cases, outs):
        assert o == d, name


def _controls(stream):
    """the LZMA2 control bytes of a single-block stream"""
    hs = (stream[12] + 1) * 4
    pos, out = 12 + hs, []
    while True:
        c = stream[pos]
        out.append(c)
        if c == 0:
            return out
        if c < 0x80:
            pos += 3 + ((stream[pos + 1] << 8) | stream[pos + 2]) + 1
        else:
            pos += (6 if c >= 0xC0 else 5) + ((stream[pos + 3] << 8) | stream[pos + 4]) + 1


def test_chunk_kinds_of_the_list():
    """what the list is there for: liblzma wrote LZMA chunks with and without resets and uncompressed chunks of both kinds"""
    by = {n: s for n, s, _ in X.streams()}
    mixed = _controls(by["mixed"])
    assert mixed[0] == 0xE1 and 0x02 in mixed and 0xA1 in mixed
    assert _controls(by["random65537"])[:2] == [0x01, 0x02]
    assert any(0x80 <= c < 0xA0 for c in _controls(by["text300k"]))       # (a chunk behind another: no reset, the model carries on)


def test_streams_one_by_one_and_their_sizes(pna, ctx):
    """each stream through xz_open_device with its exact size as the room; open_size_device gives that size with exact == 1"""
    import torch
    cases = X.streams()
    src, offs = to_device([s for _, s, _ in cases])
    for (name, s, d), off in zip(cases, offs):
        size, exact = ctx.open_size_device(src.data_ptr(), off, len(s), algo=pna.ALGO_XZ)
        assert (size, exact) == (len(d), True), name
        dst = torch.zeros(len(d) + 64, dtype=torch.uint8, device="cuda")
        got = ctx.xz_open_device(src.data_ptr(), off, len(s), dst.data_ptr(), 32, len(d))
        assert got == len(d), name
        back = dst.cpu().numpy().tobytes()
        assert back[32:32 + len(d)] == d, name
        assert back[:32] == bytes(32) and back[32 + len(d):] == bytes(32), name      # nothing written outside the room
    with pytest.raises(pna.PnaGpuError) as ei:                                   # room one byte short
        _, s, d = cases[6]
        dst = torch.zeros(len(d), dtype=torch.uint8, device="cuda")
        ctx.xz_open_device(src.data_ptr(), offs[6], len(s), dst.data_ptr(), 0, len(d) - 1)
    assert ei.value.code == pna.E_INVAL


def test_refusals(pna, ctx):
    text = X.streams()[6]
    for name, s in X.unsupported():
        with pytest.raises(pna.PnaGpuError) as ei:
            ctx.decompress_batch([s], [5000], algo=pna.ALGO_XZ)
        assert ei.value.code == pna.E_UNSUPPORTED, name
        if name == "sha256":
            assert "SHA-256" in str(ei.value)
    for wrong in (len(text[2]) - 1, len(text[2]) + 1):
        with pytest.raises(pna.PnaGpuError) as ei:
            ctx.decompress_batch([text[1]], [wrong], algo=pna.ALGO_XZ)
        assert ei.value.code == pna.E_INVAL
    with pytest.raises(pna.PnaGpuError) as ei:                                   # bytes behind the footer: a documented departure from the reference
        ctx.decompress_batch([text[1] + bytes(4)], [len(text[2])], algo=pna.ALGO_XZ)
    assert ei.value.code == pna.E_INVAL
    for algo in (3, pna.ALGO_XZ):                                                # no encoder
        with pytest.raises(pna.PnaGpuError) as ei:
            ctx.compress_batch([b"abc"], algo=algo)
        assert ei.value.code == pna.E_UNSUPPORTED
    assert ctx.decompress_batch([text[1]], [len(text[2])], algo=pna.ALGO_XZ) == [text[2]]


@pytest.mark.parametrize("name", ["xz.pna", "solid_xz.pna"])
def test_golden_archives(pna, ctx, name):
    """the reference's own xz archives: the same nine entries as zstd.pna (names, kinds, bytes; the solid archive holds them in another order), and every
    verify record OK with the entry's size"""
    want = pna.extract_archive(ctx, golden("zstd.pna"))
    assert [len(d) for _, _, d in want] == [0, 51475, 1984, 4194442, 3, 40, 57032, 0, 10]
    got = pna.extract_archive(ctx, golden(name))
    assert got == want if name == "xz.pna" else (len(got) == 9 and sorted(got) == sorted(want))
    recs, s = pna.verify_archive(ctx, golden(name))
    assert s["rc"] == 0
    assert [(r[0], r[1], r[2], r[4]) for r in recs] == [(n, k, pna.VERIFY_OK, len(d)) for n, k, d in got]


@pytest.fixture(scope="module")
def drivers_archive(pna, pf, codec):
    """xz entries with and without fSIZ beside a zstd and a deflate entry, an AES-CTR entry with an xz payload, a solid xz block"""
    files = {"x/sized": codec.corpus_file(0, 1, 5000), "x/open": codec.corpus_file(0, 9, 70001), "z/zstd": codec.corpus_file(1, 2, 30000),
             "d/deflate": codec.corpus_file(2, 3, 20000), "x/enc": codec.corpus_file(0, 5, 40000), "s/one": codec.corpus_file(0, 6, 9000),
             "s/two": bytes(3000), "x/empty": b""}
    key, phsf = pna.kdf_pbkdf2_sha256(PW, bytes(range(16)), 1000)
    iv = bytes(range(100, 116))
    body = pf.write_normal_entry(pf.file_entry_header(pna.ALGO_XZ, "x/sized"), [X.xz(files["x/sized"])], 5000)
    body += pf.write_normal_entry(pf.file_entry_header(pna.ALGO_XZ, "x/open"), [X.xz(files["x/open"])], None)
    body += pf.write_normal_entry(pf.file_entry_header(pna.ALGO_ZSTD, "z/zstd"), [codec.model_compress(files["z/zstd"])], 30000)
    body += pf.write_normal_entry(pf.file_entry_header(pna.ALGO_DEFLATE, "d/deflate"), [zlib.compress(files["d/deflate"])], 20000)
    body += pf.write_encrypted_file_entry(pna.ALGO_XZ, pna.ENC_AES, pna.MODE_CTR, "x/enc", phsf, iv, codec.aes_ctr(key, iv, X.xz(files["x/enc"])), 40000)
    solid = X.xz(pna.inner_entry_bytes("s/one", files["s/one"]) + pna.inner_entry_bytes("s/two", files["s/two"]))
    body += pf.write_solid_entry(pna.ALGO_XZ, [solid[i:i + 1000] for i in range(0, len(solid), 1000)])
    body += pf.write_normal_entry(pf.file_entry_header(pna.ALGO_XZ, "x/empty"), [X.xz(b"")], 0)
    return pf.write_archive_header() + body + pf.finalize_archive(), files


def test_drivers(pna, ctx, drivers_archive):
    arc, files = drivers_archive
    got = pna.extract_archive(ctx, arc, PW)
    assert {n: d for n, _, d in got} == files and len(got) == len(files)
    recs, s = pna.verify_archive(ctx, arc, PW)
    assert s["rc"] == 0 and all(r[2] == pna.VERIFY_OK for r in recs) and {r[0]: r[4] for r in recs} == {n: len(d) for n, d in files.items()}
    recs, s = pna.diff_archive(ctx, arc, files, PW)
    assert s["rc"] == 0 and [(r.status, r.first_diff) for r in recs] == [(pna.DIFF_SAME, None)] * len(files)
    for name, off in (("x/open", 66000), ("s/one", 8999), ("x/enc", 0)):
        other = dict(files)
        b = bytearray(files[name])
        b[off] ^= 1
        other[name] = bytes(b)
        recs, s = pna.diff_archive(ctx, arc, other, PW)
        assert [(r.name, r.status, r.first_diff) for r in recs if r.status != pna.DIFF_SAME] == [(name, pna.DIFF_CONTENTS_DIFFER, off)]
    dev = pna.extract_to_device(ctx, arc, ["x/sized", "x/open"], PW)
    assert {n: t.cpu().numpy().tobytes() for n, t in dev.items()} == {n: files[n] for n in ("x/sized", "x/open")}
    assert all(t.is_cuda for t in dev.values())


@pytest.fixture(scope="module")
def damage_archive(pf, pna, codec):
    """three entries, the `mixed` stream in the middle one; make(stream): the archive with that stream in its place (chunk CRCs recomputed)"""
    a, c = codec.corpus_file(0, 1, 5000), codec.corpus_file(1, 2, 3000)
    mixed = [s for n, s, _ in X.streams() if n == "mixed"][0]

    def make(stream, sized):
        return (pf.write_archive_header() + pf.write_normal_entry(pf.file_entry_header(pna.ALGO_XZ, "a"), [X.xz(a)], len(a))
                + pf.write_normal_entry(pf.file_entry_header(pna.ALGO_XZ, "m/mixed"), [stream], len(X.mixed_plain()) if sized else None)
                + pf.write_normal_entry(pf.file_entry_header(pna.ALGO_XZ, "c"), [X.xz(c)], None) + pf.finalize_archive())
    return make, mixed, [("a", a), ("m/mixed", X.mixed_plain()), ("c", c)]


@pytest.mark.parametrize("case", range(14))
@pytest.mark.parametrize("sized", [True, False])
def test_damage(pna, ctx, damage_archive, case, sized):
    """one damaged stream between two good ones (with fSIZ: the batch decoder; without: the measurement and the open decoder): liblzma refuses it, so verify
    says BAD_STREAM for that entry alone, extract fails with E_INVAL naming it, and the context goes on working"""
    make, mixed, plain = damage_archive
    name, stream = X.damage_cases(mixed)[case]
    assert len(X.damage_cases(mixed)) == 14
    assert X.liblzma_refuses(stream), name + ": liblzma accepts this stream -- the case is a test bug"
    arc = make(stream, sized)
    recs, s = pna.verify_archive(ctx, arc)
    assert [r[0] for r in recs] == ["a", "m/mixed", "c"], name
    assert recs[0][2] == pna.VERIFY_OK and recs[2][2] == pna.VERIFY_OK, (name, recs)
    assert recs[1][2] in (pna.VERIFY_BAD_STREAM, pna.VERIFY_BAD_STRUCTURE), (name, recs[1])
    with pytest.raises(pna.PnaGpuError) as ei:
        pna.extract_archive(ctx, arc)
    assert ei.value.code == pna.E_INVAL and "m/mixed" in str(ei.value), (name, str(ei.value))
    assert [(n, d) for n, _, d in pna.extract_archive(ctx, make(mixed, sized))] == plain, name
