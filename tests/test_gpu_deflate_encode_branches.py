"""The crafted deflate-encoder inputs (deflate_enc_cases.py; what each reaches is proved on the CPU by test_deflate_enc_cases.py) through every device form
of the entropy stage: k_dstats<256> / k_adler<256> (a workgroup per segment / block), k_dstats<64> / k_adler<64> and the 64-thread k_dwrite (a wave per
entry: batches of >= 4 096 entries of at most 32 KiB), k_dblock behind each form of the LZ stage (its chunk table is written by different kernels),
k_dplan / k_dwrite / k_dfinal on the device-resident route, k_dfold on the streams compressed in runs.  Expected bytes are always the model's
(codec.deflate_model_compress) -- no tolerance anywhere -- and every output also inflates with zlib."""
import functools
import zlib

import pytest

import deflate_enc_cases as dc
from conftest import headline_context

pytestmark = pytest.mark.gpu

CASES = dc.cases()
PLAIN = {n: p for n, p, _ in CASES}
PAIRS = [(n, lv) for n, _, levels in CASES for lv in levels]


@functools.lru_cache(maxsize=None)
def _want(name, level):
    return dc.model_stream(PLAIN[name], level)


def _family(*letters):
    return [(n, lv) for n, lv in PAIRS if n[0] in letters]


def _check(outs, pairs, what):
    bad = [(n, lv) for (n, lv), o in zip(pairs, outs) if o != _want(n, lv)]
    assert not bad, (what, bad[:6])
    for (n, lv), o in zip(pairs, outs):
        assert zlib.decompress(o) == PLAIN[n], (what, n, lv)


def _by_level(pairs):
    return {lv: [(n, l2) for n, l2 in pairs if l2 == lv] for lv in sorted({lv for _, lv in pairs})}


def test_workgroup_form_every_case(gpu_ctx, pna):
    """all cases of a level in one batch: a workgroup per segment builds the codes (k_dstats<256>), a workgroup per block the Adler-32 halves"""
    for level, pairs in _by_level(PAIRS).items():
        outs = gpu_ctx.compress_batch([PLAIN[n] for n, _ in pairs], algo=pna.ALGO_DEFLATE, level=level)
        _check(outs, pairs, "level %d" % level)
        for (n, _), o in zip(pairs, outs):
            assert len(o) <= pna.bound(pna.ALGO_DEFLATE, len(PLAIN[n])), n


def test_wave_per_entry_form(gpu_ctx, pna, codec):
    """the small cases at the front, in the middle and at the end of a batch of more than 4 200 entries of at most 32 KiB: one wave per entry builds the codes
    (k_dstats<64>: five rounds of 64 over the code lengths instead of two of 256), sums the Adler-32 halves and writes the stream.  Every entry, fillers
    included, must be the model's."""
    small = [(n, lv) for n, lv in PAIRS if lv == 6 and n[0] in "BCDEGH" and len(PLAIN[n]) <= 32768]
    assert {n[0] for n, _ in small} >= set("BCDE") and len(small) >= 50
    fillers = [codec.corpus_file(i & 1, 7000 + i, 64 + (i * 37) % 537) for i in range(240)]
    fill_want = [codec.deflate_model_compress(f) for f in fillers]
    third = len(small) // 3
    ents, want = [], []

    def put_cases(part):
        for n, lv in part:
            ents.append(PLAIN[n]); want.append(_want(n, lv))

    def put_fillers(k):
        for i in range(k):
            ents.append(fillers[i % len(fillers)]); want.append(fill_want[i % len(fillers)])
    put_cases(small[:third]); put_fillers(2100); put_cases(small[third:2 * third]); put_fillers(2100); put_cases(small[2 * third:])
    assert len(ents) >= 4200 and max(map(len, ents)) <= 32768
    outs = gpu_ctx.compress_batch(ents, algo=pna.ALGO_DEFLATE, level=6)
    bad = [i for i, (o, w) in enumerate(zip(outs, want)) if o != w]
    assert not bad, (bad[:8], [len(ents[i]) for i in bad[:8]])
    where = list(range(third)) + list(range(third + 2100, 2 * third + 2100)) + list(range(2 * third + 4200, len(ents)))
    assert all(zlib.decompress(outs[i]) == ents[i] for i in where + list(range(third, third + 2100, 97)))


@pytest.mark.parametrize("form", ["one_kernel", "wave_parse", "no_workspace"])
def test_lz_forms_feed_the_block_coder(pna, form):
    """families A, F and G behind the one-kernel LZ stage, the wave-per-region parse and the fall-back without a words workspace: k_dblock reads the chunk
    table each of them writes"""
    import torch  # noqa: F401  (shares its HIP runtime with the extension)
    pairs = _family("A", "F", "G")
    with (headline_context(pna, flags=pna.F_STD | pna.F_LZ_WAVEPARSE) if form == "wave_parse" else headline_context(pna)) as ctx:
        if form == "one_kernel":
            ctx.set_option("lz_split", 0)
        if form == "no_workspace":
            ctx.set_option("lz_pbuf_fail", 1)
        for level, part in _by_level(pairs).items():
            outs = ctx.compress_batch([PLAIN[n] for n, _ in part], algo=pna.ALGO_DEFLATE, level=level)
            _check(outs, part, (form, level))


def test_device_resident_route_with_guard_bands(gpu_ctx, pna):
    """compress_batch_device: sources at odd multiples of 16 bytes with a guard pattern between them, the destination inside guard bands of 0xA5.  The offsets
    are exact, nothing outside [0, total) of the destination is written, the sources are untouched, and a second call gives the same bytes."""
    import torch
    pairs = [(n, lv) for n, lv in PAIRS if lv == 6]
    ents = [PLAIN[n] for n, _ in pairs]
    offs, pos = [], 16
    for e in ents:
        offs.append(pos)
        pos = (pos + len(e) + 15) & ~15
        pos += 16 if (pos >> 4) & 1 == 0 else 32              # an odd multiple of 16, at least 16 guard bytes in between
    image = bytearray(b"\x5a" * (pos + 4096))
    for o, e in zip(offs, ents):
        image[o:o + len(e)] = e
    assert all(o % 32 == 16 for o in offs)
    src = torch.frombuffer(bytearray(image), dtype=torch.uint8).cuda()
    cap = sum(pna.bound(pna.ALGO_DEFLATE, len(e)) for e in ents) + 16
    G = 4096
    first = None
    for _ in range(2):
        dst = torch.full((G + cap + G,), 0xA5, dtype=torch.uint8, device="cuda")
        o = gpu_ctx.compress_batch_device(src.data_ptr(), offs, [len(e) for e in ents], dst.data_ptr() + G, cap, algo=pna.ALGO_DEFLATE, level=6)
        host = dst.cpu().numpy().tobytes()
        assert len(o) == len(ents) + 1 and o[0] == 0 and all(a < b for a, b in zip(o, o[1:])) and o[-1] <= cap
        assert host[:G] == b"\xA5" * G and host[G + o[-1]:] == b"\xA5" * (len(host) - G - o[-1])
        got = [host[G + a:G + b] for a, b in zip(o, o[1:])]
        assert [b - a for a, b in zip(o, o[1:])] == [len(_want(n, lv)) for n, lv in pairs]
        _check(got, pairs, "device route")
        assert src.cpu().numpy().tobytes() == bytes(image)
        assert first is None or host == first
        first = host


class _Sink:
    def __init__(self):
        self.parts = []

    def write(self, b):
        self.parts.append(bytes(b))


def test_stream_facade_and_solid_payload(gpu_ctx, pna):
    """the CompressionWriter facade (write in odd pieces, finish) and pna_gpu_compress_solid on families A, G and H"""
    for n, lv in _family("A", "G", "H"):
        d = PLAIN[n]
        w = gpu_ctx.writer(_Sink(), algo=pna.ALGO_DEFLATE, level=lv)
        for i in range(0, len(d), 333331):
            w.write(d[i:i + 333331])
        got = b"".join(w.try_into_inner().parts)
        assert got == _want(n, lv), ("writer", n, lv)
        assert zlib.decompress(got) == d
    for n, lv in _family("A", "G", "H"):
        got = b"".join(gpu_ctx.compress_solid(PLAIN[n], algo=pna.ALGO_DEFLATE, level=lv))
        assert got == _want(n, lv), ("solid payload", n, lv)


def test_solid_archive_in_windows_carries_the_adler_sum(gpu_ctx, pna, pf, codec):
    """a solid deflate archive streamed through windows of 1 MiB: families A and H span several runs, so k_dfold carries the Adler-32 over a cut between two
    entries (the first record ends exactly on the window's edge) and over cuts in the middle of an entry of 0xFF bytes -- the largest sums there are.  The SDAT
    body is the model's stream of the serialised inner entries, for 1 and for 2 MiB windows."""
    record = lambda nm, e: pf.write_normal_entry(pf.file_entry_header(0, pf.sanitize_name(nm)), [e] if e else [], len(e))
    names = ["s/%d" % i for i in range(7)]
    ln = (1 << 20) - 100
    for _ in range(8):                                         # the first entry's length that ends its record exactly on the first window's edge
        ln += (1 << 20) - len(record(names[0], PLAIN["A.geo_2.0_x28"][:ln]))
    ents = [PLAIN["A.geo_2.0_x28"][:ln], PLAIN["H.ff_3145745"], PLAIN["A.geo_1.1_x256"], b"", PLAIN["H.ff_00_blocks_2mib"][:(1 << 20) + (1 << 17) + 5],
            PLAIN["A.geo_1.7_x40"], PLAIN["H.f1_65521"]]
    plain = b"".join(record(nm, e) for nm, e in zip(names, ents))
    assert len(record(names[0], ents[0])) == 1 << 20 and plain[(1 << 21) - 8:(1 << 21) + 8] == b"\xff" * 16          # a cut between entries; a cut inside the 0xFF entry
    try:
        for win, level in ((1, 6), (1, 1), (2, 6), (1, 0)):
            gpu_ctx.set_option("solid_win_mib", win)
            arc = pna.create_archive(gpu_ctx, names, ents, algo=pna.ALGO_DEFLATE, level=level, solid=True)
            _, items = pf.read_archive(arc)
            assert len(items) == 1
            body = items[0].data
            assert zlib.decompress(body) == plain, (win, level)
            assert body == codec.deflate_model_compress(plain, codec.params_for_level(level, deflate=True)), (win, level)
    finally:
        gpu_ctx.set_option("solid_win_mib", 256)


def test_streams_decode_on_the_device(gpu_ctx, pna):
    """every case stream through the project's own inflate: deep codes, one-code and no-code distance tables, stored pieces, headers of every size"""
    pairs = PAIRS
    back = gpu_ctx.decompress_batch([_want(n, lv) for n, lv in pairs], [len(PLAIN[n]) for n, _ in pairs], algo=pna.ALGO_DEFLATE)
    bad = [(n, lv) for (n, lv), b in zip(pairs, back) if b != PLAIN[n]]
    assert not bad, bad[:6]
