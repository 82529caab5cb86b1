"""GPU parity tests (run on the MI355X box with -m gpu).  Everything goes through the C ABI of libpna_gpu.so.

Bar: the HIP path must equal the oracle's encoder model BIT FOR BIT (byte/integer work), the streams must decode
with two independent decoders (oracle/zstd_dec.c, system libzstd) to the input, and archives must read back through
the fixture-pinned container reader to the original tree.
"""
import hashlib
import importlib
import io
import os
import ctypes
import zlib

import pytest

from conftest import GOLDEN, headline_context

pytestmark = pytest.mark.gpu


def _raw(rel):
    with open(os.path.join(GOLDEN, rel), "rb") as f:
        return f.read()


def _params(codec):
    return codec.params_for_level(3)        # the product's default level set (no repeat codes, two-step lazy deferral, the 32 KiB-window geometry)


def _cases(codec):
    return {
        "empty": b"", "one": b"a", "tiny7": b"abcdefg", "tiny8": b"abcdefgh", "a1000": b"a" * 1000, "zeros5000": bytes(5000),
        "rnd10000": codec.corpus_file(2, 3, 10000), "txt4k": codec.corpus_file(1, 9, 4096), "t2047": codec.corpus_file(0, 9, 2047),
        "t2049": codec.corpus_file(0, 9, 2049), "txt64k": codec.corpus_file(1, 2, 65536), "txt300k": codec.corpus_file(0, 1, 300000),
        "blk-1": codec.corpus_file(0, 11, 131071), "blk": codec.corpus_file(0, 11, 131072), "blk+1": codec.corpus_file(0, 11, 131073),
        "txt1m": codec.corpus_file(0, 3, 1 << 20), "seg+1": codec.corpus_file(0, 12, (1 << 20) + 1),
        "txt2m+": codec.corpus_file(0, 4, (2 << 20) + 12345), "zero1m": bytes(1 << 20), "x300k": b"x" * 300000, "ab": b"ab" * 70000,
        "abc": (b"abcdefghij" * 20000)[:131072 + 77], "rnd1m": codec.corpus_file(2, 0, 1 << 20), "png": _raw("raw/images/icon.png"),
        "svg": _raw("raw/images/icon.svg"), "nest": _raw("raw/pna/nest.pna"),
        "mixed": codec.corpus_file(0, 7, 200000) + codec.corpus_file(2, 7, 100000) + bytes(150000) + codec.corpus_file(1, 7, 300000),
        "period7": bytes((i * 37 + (i // 7) * 11) & 0xFF for i in range(7)) * 30000,
    }


def test_corpus_generator_matches_oracle(gpu_ctx, codec):
    import torch
    for kind, n in ((0, 20000), (1, 4096), (1, 65536), (2, 8192), (3, 5000), (4, 5000), (0, 1 << 20)):
        stride = (n + 15) & ~15
        t = torch.empty(stride * 3 + 4096, dtype=torch.uint8, device="cuda")
        gpu_ctx.corpus_fill_device(kind, 5, 3, n, stride, t.data_ptr())
        host = t.cpu().numpy().tobytes()
        for f in range(3):
            assert host[f * stride:f * stride + n] == codec.corpus_file(kind, 5 + f, n), (kind, n, f)


def test_batch_bit_exact_and_decodable(gpu_ctx, codec):
    cases = _cases(codec)
    names = sorted(cases)
    outs = gpu_ctx.compress_batch([cases[k] for k in names])
    p = _params(codec)
    for k, o in zip(names, outs):
        d = cases[k]
        assert codec.zstd_decompress(o, len(d)) == d, k
        if codec.system_libzstd() is not None:
            assert codec.libzstd_decompress_stream(o, len(d)) == d, k
        assert o == codec.model_compress(d, p), k
        assert len(o) <= gpu_ctx._L.pna_gpu_bound(2, len(d)), k


def test_serial_end_scan_is_identical(pna, codec):
    """Flag 0x200 forces the serial form of k_lz's end scan (the merge of the waves' parses) on every tile; results must not change."""
    import torch  # noqa: F401
    cases = _cases(codec)
    names = sorted(cases)
    with headline_context(pna, flags=pna.F_STD | 0x200) as ctx:
        outs = ctx.compress_batch([cases[k] for k in names])
    p = _params(codec)
    for k, o in zip(names, outs):
        assert o == codec.model_compress(cases[k], p), k


@pytest.mark.parametrize("form", ["default", "fused", "waveparse", "split"])
def test_lz_stage_forms_are_identical(pna, codec, form, monkeypatch):
    """The LZ stage runs as two kernels by default (k_lz<MODE 1>: look-up / match / inserts -> one word per position in a workspace ->
    k_lzp: parse with one lane per region); PNA_F_LZ_FUSED runs the one-kernel form (k_lz<MODE 0>), PNA_F_LZ_WAVEPARSE the split form with
    the wave-per-region parse (k_lz<MODE 2>).  All of them must equal the model, for both codecs and every level set, on the cases
    of the main test and on the inputs that stress far candidates, adoption, block / segment ends and the extension of capped matches."""
    import random
    import torch  # noqa: F401
    rnd = random.Random(77)
    cases = dict(_cases(codec))
    text = codec.corpus_file(0, 4343, 1 << 20)
    rb = lambda n: bytes(rnd.getrandbits(8) for _ in range(n))
    cases["far"] = text[:300000] + rb(70000) + text[1000:250000] + rb(1000) + text[123:200123]
    cases["runs"] = rb(100000) + bytes(200000) + rb(60000) + bytes(200000) + b"ab" * 50000
    cases["ends"] = rb(131072 - 50) + text[:100] + rb(70000) + text[:100] + rb(131072 - 70000 - 150) + text[:100]
    cases["tail"] = text[:4096 * 3 + 17]
    cases["3 MiB"] = codec.corpus_file(0, 4344, 3 << 20)
    names = sorted(cases)
    data = [cases[k] for k in names]
    bit = {"default": 0, "fused": pna.F_LZ_FUSED, "waveparse": pna.F_LZ_WAVEPARSE, "split": 0}[form]      # ("split": k_lzm + k_lzp, the suite's setting)
    with headline_context(pna, flags=pna.F_STD | bit) as ctx:
        if form == "split":
            ctx.set_option("lz_split_min", 0)            # (what the library chooses by itself as well: the split form at every size)
        for level in (1, 2, 3, 7, 19):              # the zstd level sets: fast, light, default, high, max (codec.product_level_flags)
            outs = ctx.compress_batch(data, level=level)
            # the form actually taken: the one-kernel form launches no match kernel, the split forms do
            # (levels 10 .. 22 always take the split form: only the match kernel k_lzm has the global-memory hash table of the strong set)
            assert (ctx.timing().lz_match_launches == 0) == (form == "fused" and level < 10), (form, level)
            pz = codec.params_for_level(level)
            for k, d, o in zip(names, data, outs):
                assert o == codec.model_compress(d, pz), (k, level)
        for level, fl in ((1, codec.F_LAZY), (6, codec.F_ADOPT | codec.F_INS2 | codec.F_LAZY), (9, codec.F_ADOPT | codec.F_INS2 | codec.F_LAZY | codec.F_STRONG)):
            outs = ctx.compress_batch(data, algo=pna.ALGO_DEFLATE, level=level)
            pd = codec.params_for_flags(fl, deflate=True)
            for k, d, o in zip(names, data, outs):
                assert o == codec.deflate_model_compress(d, pd), (k, level)


def test_lz_stage_split_runs(pna, codec, monkeypatch):
    """The split LZ stage works through a sub-batch in runs that share one workspace (PNA_LZ_SPLIT_BLOCKS blocks each, default 32 768 = 4 GiB
    of input): with 8 blocks per run every 1 MiB segment is a run of its own, entries of several segments span runs, small entries share one."""
    import torch  # noqa: F401
    monkeypatch.setenv("PNA_LZ_SPLIT_BLOCKS", "8")
    ents = [codec.corpus_file(0, 51, (3 << 20) + 4097), b"", codec.corpus_file(1, 52, 5000), codec.corpus_file(0, 53, 1 << 20), bytes(300000),
            codec.corpus_file(0, 54, 200000), codec.corpus_file(2, 55, 70000), codec.corpus_file(0, 56, (1 << 20) + 1)]
    with headline_context(pna) as ctx:
        outs = ctx.compress_batch(ents)
        p = _params(codec)
        for e, o in zip(ents, outs):
            assert o == codec.model_compress(e, p)
        outs = ctx.compress_batch(ents, algo=pna.ALGO_DEFLATE)
        for e, o in zip(ents, outs):
            assert o == codec.deflate_model_compress(e, codec.params_for_flags(codec.F_ADOPT | codec.F_INS2 | codec.F_LAZY, deflate=True))
            assert zlib.decompress(o) == e


def test_lz_stage_fuzz_against_model(gpu_ctx, pna, codec):
    """Seeded structured noise through the split LZ stage (the suite's default) in one batch per codec and level set: entries of 0 .. 400 KB built
    from random bytes, runs, text and copies of their own earlier fragments at all distances and alignments -- many short and long matches,
    literals runs of every length, matches across tile / block borders and ends in odd places.  Bit-exact with the model."""
    import os
    import random
    text = codec.corpus_file(0, 999, 400000)
    for seed in range(20260, 20260 + int(os.environ.get("PNA_FUZZ_SEEDS", "1"))):      # (PNA_FUZZ_SEEDS=N: a longer soak, N batches)
        _fuzz_one(gpu_ctx, pna, codec, text, random.Random(seed))


def _fuzz_one(gpu_ctx, pna, codec, text, rnd):
    ents = []
    for i in range(120):
        target = rnd.choice((0, 1, 7, 100, 4095, 4096, 4097, 20000, 70000, 131072 + rnd.randrange(-3, 4), 250000, 400000)) if i < 40 else rnd.randrange(1, 300000)
        buf = bytearray()
        while len(buf) < target:
            k = rnd.random()
            if k < 0.25 or not buf:
                buf += bytes(rnd.getrandbits(8) for _ in range(rnd.randrange(1, 40)))
            elif k < 0.40:
                buf += bytes([rnd.getrandbits(8)]) * rnd.randrange(1, 600)
            elif k < 0.60:
                o = rnd.randrange(len(text) - 300); buf += text[o:o + rnd.randrange(3, 300)]
            else:                                                   # copy of an earlier fragment (overlapping copies included)
                d = rnd.choice((1, 2, 3, 5, 8, 64, 4096, 28367, 28368, 28369, 32768, 56064, 60000, 131072)) if rnd.random() < 0.5 else rnd.randrange(1, len(buf) + 1)   # (28 368: where the match kernel's window ends -- FLAG_FAR1's border)
                d = min(d, len(buf)); n = rnd.randrange(3, 2000)
                st = len(buf) - d
                for t in range(n):
                    buf.append(buf[st + t])
        ents.append(bytes(buf[:target]))
    for level in (3, 7, 19, 1):
        outs = gpu_ctx.compress_batch(ents, level=level)
        pz = codec.params_for_level(level)
        for i, (e, o) in enumerate(zip(ents, outs)):
            assert o == codec.model_compress(e, pz), (i, len(e), level)
    for level, fl in ((6, codec.F_ADOPT | codec.F_INS2 | codec.F_LAZY), (9, codec.F_ADOPT | codec.F_INS2 | codec.F_LAZY | codec.F_STRONG)):
        outs = gpu_ctx.compress_batch(ents, algo=pna.ALGO_DEFLATE, level=level)
        pd = codec.params_for_flags(fl, deflate=True)
        for i, (e, o) in enumerate(zip(ents, outs)):
            assert o == codec.deflate_model_compress(e, pd), (i, len(e), level)
            assert zlib.decompress(o) == e


def test_lz_stage_fuzz_large_entries(gpu_ctx, pna, codec):
    """The same kind of structured noise in entries of 1 - 4 MiB: segments that are not the entry's first, far candidates at every distance up to the
    segment size, copies across block and segment borders (which the encoder must not follow), tails of odd length."""
    import random
    rnd = random.Random(777)
    text = codec.corpus_file(0, 998, 1 << 20)
    ents = []
    for target in ((1 << 20) + 1, (2 << 20) - 7, 3 * (1 << 20) + 4099, (1 << 20) - 4097, (4 << 20), 1500001):
        buf = bytearray()
        while len(buf) < target:
            k = rnd.random()
            if k < 0.15 or not buf:
                buf += bytes(rnd.getrandbits(8) for _ in range(rnd.randrange(1, 200)))
            elif k < 0.25:
                buf += bytes([rnd.getrandbits(8)]) * rnd.randrange(1, 5000)
            elif k < 0.55:
                o = rnd.randrange(len(text) - 4000); buf += text[o:o + rnd.randrange(3, 4000)]
            else:
                d = rnd.choice((1, 7, 4096, 11983, 11984, 11985, 28367, 28368, 28369, 51968, 51969, 56064, 56065, 65536, 131072, 500000, (1 << 20) - 1, 1 << 20, (1 << 20) + 1))
                d = min(d, len(buf)); n = rnd.randrange(3, 20000)
                buf += (bytes(buf[len(buf) - d:]) * (n // d + 1))[:n]          # an overlapping copy repeats its period
        ents.append(bytes(buf[:target]))
    for level in (3, 7, 19):
        outs = gpu_ctx.compress_batch(ents, level=level)
        pz = codec.params_for_level(level)
        for i, (e, o) in enumerate(zip(ents, outs)):
            assert o == codec.model_compress(e, pz), (i, len(e), level)
            assert codec.zstd_decompress(o, len(e)) == e
    outs = gpu_ctx.compress_batch(ents, algo=pna.ALGO_DEFLATE)
    pd = codec.params_for_flags(codec.F_ADOPT | codec.F_INS2 | codec.F_LAZY, deflate=True)
    for i, (e, o) in enumerate(zip(ents, outs)):
        assert o == codec.deflate_model_compress(e, pd), (i, len(e))
        assert zlib.decompress(o) == e


def test_compress_batch_in_pieces(pna, codec, monkeypatch):
    """pna_gpu_compress_batch takes a large batch through in pieces (>= 256 MiB each: staging + H2D of piece k + 1 and the D2H + scatter of
    piece k - 1 next to piece k's kernels).  With 1 MiB pieces a handful of entries already makes several: every entry must come back in its
    own buffer, equal to the model, whatever piece it was in (empty entries, entries larger than a piece, a short last piece)."""
    import torch  # noqa: F401
    monkeypatch.setenv("PNA_BATCH_PIECE_MIB", "1")
    ents = [codec.corpus_file(0, 71, 600000), codec.corpus_file(1, 72, 500000), b"", codec.corpus_file(0, 73, (2 << 20) + 77), bytes(100), codec.corpus_file(2, 74, 900000),
            codec.corpus_file(0, 75, 300000), codec.corpus_file(0, 76, 300001), codec.corpus_file(1, 77, 300002), b"x", codec.corpus_file(0, 78, 1 << 20), codec.corpus_file(0, 79, 5000)]
    with headline_context(pna) as ctx:
        outs = ctx.compress_batch(ents)
        for e, o in zip(ents, outs):
            assert o == codec.model_compress(e, _params(codec))
        douts = ctx.compress_batch(ents, algo=pna.ALGO_DEFLATE)
        for e, o in zip(ents, douts):
            assert zlib.decompress(o) == e
        ctx.set_option("batch_piece_mib", 0)
        assert ctx.compress_batch(ents) == outs and ctx.compress_batch(ents, algo=pna.ALGO_DEFLATE) == douts


def test_lz_stage_without_workspace_falls_back(pna, codec, monkeypatch):
    """When the words workspace of the split LZ stage cannot be allocated the library halves the run and finally takes the one-kernel form
    (option lz_pbuf_fail makes every allocation of it fail): same bytes; with the option off again the next call is back on the split form."""
    import torch  # noqa: F401
    monkeypatch.setenv("PNA_LZ_PBUF_FAIL", "1")
    ents = [codec.corpus_file(0, 61, (2 << 20) + 5), codec.corpus_file(1, 62, 70000), b"", codec.corpus_file(0, 63, 1 << 20)]
    with headline_context(pna) as ctx:
        for _ in range(2):
            outs = ctx.compress_batch(ents)
            for e, o in zip(ents, outs):
                assert o == codec.model_compress(e, _params(codec))
            assert ctx.timing().lz_match_launches == 0          # nothing went through the match kernel
        ctx.set_option("lz_pbuf_fail", 0)
        assert ctx.compress_batch(ents) == outs and ctx.timing().lz_match_launches > 0     # a failed allocation is not remembered


@pytest.mark.parametrize("form", [0x1000, 0x2000])
def test_both_sequence_coder_forms_are_identical(pna, codec, form):
    """The sequences bitstream has two implementations picked by batch size (k_seqa + k_seqb: short state chain, token-parallel packing;
    k_seq: one kernel); flags 0x1000 / 0x2000 force one of them.  Both must equal the oracle's encoder."""
    import torch  # noqa: F401
    cases = _cases(codec)
    names = sorted(cases)
    with headline_context(pna, flags=pna.F_STD | form) as ctx:
        outs = ctx.compress_batch([cases[k] for k in names])
    p = _params(codec)
    for k, o in zip(names, outs):
        assert o == codec.model_compress(cases[k], p), k


@pytest.mark.parametrize("flags", [0, 1, 2, 3, 4, 0x77, 0x27, 0x67, 0x17, 0x47, 0x37, 0xF7, 0xE7, 0xB7])
def test_feature_subsets_bit_exact(pna, codec, flags):
    """Every subset of the encoder's switches -- Huffman / FSE / lazy, and the level-set bits F_FAR (0x10), F_ADOPT (0x20), F_INS2 (0x40) --
    and F_STRONG (0x80) -- against the model with the corresponding parameters."""
    import torch  # noqa: F401
    ents = [codec.corpus_file(0, 21, 300000), codec.corpus_file(1, 22, 5000), bytes(70000), b"", codec.corpus_file(2, 1, 3000),
            codec.corpus_file(0, 23, 1 << 20)]
    with headline_context(pna, flags=flags) as ctx:
        outs = ctx.compress_batch(ents)
        outs2 = ctx.compress_batch(ents, level=2)
    # level 2 (the light set) keeps the context's bits as they are; the default level adds the third adoption round (F_STRONG) where the bits allow it
    p = codec.params_for_level(3, ctx_flags=flags)
    p2 = codec.params_for_level(2, ctx_flags=flags)
    assert (p.rounds == 0x214) == bool(flags & 0x20 and flags & 4) and p2.rounds == (0x214 if flags & 0x80 and flags & 0x20 else 0x21 if flags & 0x20 else 0)
    for e, o, o2 in zip(ents, outs, outs2):
        assert o == codec.model_compress(e, p)
        assert o2 == codec.model_compress(e, p2)
        assert codec.zstd_decompress(o, len(e)) == e


@pytest.mark.parametrize("form", ["split", "one-kernel"])
def test_lds_geometries_equal_the_model(pna, codec, form):
    """The match finder shares a CU's 160 KiB of LDS between window and hash table in one of three geometries (lz_common.h LzGeo): 64 KiB + 24 512 slots,
    32 KiB (the zstd default set), 16 KiB (the high set); option win32k = 0 / 1 / 2 puts both sets on the first / leaves the choice / puts both on the
    last.  On the two small windows the table is PACKED (option tab3, default 1: three 21-bit entries per 64-bit LDS word -- 49 062 / 55 206 slots, of a
    tile's inserts into one word only the highest (field, position) is stored) or holds 32-bit entries (tab3 = 0: 32 704 / 36 800 slots).  What the window
    does not hold is read from the segment (far candidates): same rules, other table -- every combination must equal the model with that table, in both
    forms of the LZ stage, and more slots must not compress worse."""
    import torch  # noqa: F401
    ents = [codec.corpus_file(0, 1, 300000), codec.corpus_file(0, 2, (1 << 20) + 77), codec.corpus_file(1, 3, 65536), b"", codec.corpus_file(0, 5, 2500000)]
    size = {}
    with pna.Context(0) as ctx:
        ctx.set_option("latency_max_mib", 0)
        ctx.set_option("lz_split_min", 0 if form == "split" else 1 << 20)
        for t3 in (1, 0):
            ctx.set_option("tab3", t3)
            for w in (0, 1, 2):
                ctx.set_option("win32k", w)
                for lvl in (3, 7):
                    outs = ctx.compress_batch(ents, level=lvl)
                    assert (ctx.timing().lz_match_launches > 0) == (form == "split")
                    p = codec.params_for_level(lvl, win32k=w, tab3=t3)
                    want = {(0, 3): 24512, (0, 7): 24512, (1, 3): 32704, (1, 7): 36800, (2, 3): 36800, (2, 7): 36800} if not t3 else \
                           {(0, 3): 24512, (0, 7): 24512, (1, 3): 49062, (1, 7): 55206, (2, 3): 55206, (2, 7): 55206}
                    assert p.hash_log == want[(w, lvl)] and p.tab3 == (1 if (t3 and w) else 0)
                    for e, o in zip(ents, outs):
                        assert o == codec.model_compress(e, p), (t3, w, lvl, len(e))
                    size[(t3, w, lvl)] = sum(map(len, outs))
    for t3 in (0, 1):
        assert size[(t3, 2, 3)] < size[(t3, 1, 3)] < size[(t3, 0, 3)] and size[(t3, 1, 7)] < size[(t3, 0, 7)] and size[(t3, 1, 7)] < size[(t3, 1, 3)]
    assert size[(1, 1, 3)] < size[(0, 1, 3)] and size[(1, 1, 7)] < size[(0, 1, 7)]        # the packed table remembers more


@pytest.mark.parametrize("form", ["split", "one-kernel"])
def test_far_candidates_beyond_one_round_are_dropped(pna, codec, form):
    """FLAG_FAR1 (option far1, default 1; zstd levels 2 .. 5 on the packed 32 KiB-window geometry): the match kernel verifies at most 63 candidates beyond its window per
    wave of 256 positions -- one compacted round of its dense lanes -- and drops the rest, numbered j-major over its four positions per lane; the one-kernel form, whose lanes
    hold other positions, drops the same ones.  Both forms equal the model with far_slots = 63 / 0, and the option costs ratio, not correctness."""
    import torch  # noqa: F401
    ents = [codec.corpus_file(0, 2, (1 << 20) + 77), codec.corpus_file(0, 5, 2500000), codec.corpus_file(1, 3, 400000), codec.corpus_file(0, 8, 131072 + 4096 + 100)]
    size = {}
    with pna.Context(0) as ctx:
        ctx.set_option("latency_max_mib", 0)
        ctx.set_option("lz_split_min", 0 if form == "split" else 1 << 20)
        for far1 in (1, 0):
            ctx.set_option("far1", far1)
            for lvl in (3, 2, 7):
                outs = ctx.compress_batch(ents, level=lvl)
                p = codec.params_for_level(lvl, far1=far1)
                assert p.far_slots == (63 if (far1 and lvl < 4) else 0)
                for e, o in zip(ents, outs):
                    assert o == codec.model_compress(e, p), (far1, lvl, len(e))
                    assert codec.zstd_decompress(o, len(e)) == e
                size[(far1, lvl)] = sum(map(len, outs))
    assert size[(0, 3)] < size[(1, 3)] < size[(0, 3)] * 1.01 and size[(0, 7)] == size[(1, 7)]


@pytest.mark.parametrize("form", ["split", "one-kernel"])
def test_high_sets_adopt_over_eight_positions(pna, codec, form):
    """FLAG_STRONG2 (option strong2, default 1): zstd levels 6 .. 22 on their standard geometries (the packed 16 KiB-window table; the table in global memory) run a fourth
    adoption round over eight positions, first, and count up to 15 back bytes (model: rounds 0x2148, back_cap 15; a usable candidate lies at position 16 or beyond).
    Both forms of the LZ stage, short segments (the small geometry) included, equal the model; the option off gives the default set's three rounds; more rounds compress better."""
    import torch  # noqa: F401
    ents = [codec.corpus_file(0, 2, (1 << 20) + 77), codec.corpus_file(0, 5, 1500000), codec.corpus_file(1, 3, 400000), codec.corpus_file(0, 8, 131072 + 4096 + 100),
            codec.corpus_file(0, 9, 3000), codec.corpus_file(0, 10, 9000), b"ab" * 40, b"", (b"0123456789abcdefXYZ" * 3000)[:50000]]
    size = {}
    with pna.Context(0) as ctx:
        ctx.set_option("latency_max_mib", 0)
        ctx.set_option("lz_split_min", 0 if form == "split" else 1 << 20)
        for s2 in (1, 0):
            ctx.set_option("strong2", s2)
            for lvl in (7, 12, 3):
                outs = ctx.compress_batch(ents, level=lvl)
                p = codec.params_for_level(lvl, strong2=s2)
                assert (p.rounds, p.back_cap) == ((0x2148, 15) if (s2 and lvl >= 4) else (0x214, 7))
                for e, o in zip(ents, outs):
                    assert o == codec.model_compress(e, p), (s2, lvl, len(e))
                    assert codec.zstd_decompress(o, len(e)) == e
                size[(s2, lvl)] = sum(map(len, outs))
    assert size[(1, 7)] < size[(0, 7)] and size[(1, 12)] < size[(0, 12)] and size[(1, 3)] == size[(0, 3)]


def test_lz_stage_equals_model(gpu_ctx, codec):
    d = codec.corpus_file(0, 31, 700000)
    gpu_ctx.compress_batch([d])
    model = codec.model_lz_segment(d, _params(codec))
    for b, (ms, ml) in enumerate(model):
        gs, gl = gpu_ctx.debug_block(b)
        assert gs == ms and gl == ml, b


def test_compression_writer_facade(gpu_ctx, pna, codec):
    """CompressionWriter shape: write()* then try_into_inner(); the sink sees bursts of at most 32 KiB."""
    d = codec.corpus_file(0, 41, 500000)

    class Sink:
        def __init__(self): self.parts = []
        def write(self, b): self.parts.append(bytes(b))
    w = gpu_ctx.writer(Sink())
    for i in range(0, len(d), 77777):
        assert w.write(d[i:i + 77777]) == len(d[i:i + 77777])
    w.flush()
    sink = w.try_into_inner()
    assert max(len(p) for p in sink.parts) <= 32768
    assert b"".join(sink.parts) == codec.model_compress(d, _params(codec))


def test_compression_writers_on_many_threads_are_batched(pna, codec):
    """The seam as the reference drives it (one writer per task, many tasks in flight, cli/src/command/core.rs:505-517): writers of ONE
    context finished from 24 threads at once.  Every sink receives exactly its own entry's stream (== the oracle's encoder), in order and
    on its own thread; the finishes were carried by fewer device batches than there are entries (group commit)."""
    import threading
    import torch  # noqa: F401
    ctx = headline_context(pna)
    try:
        sizes = [0, 1, 777, 4096, 65536, 200000, 300001, 1 << 20]
        n_threads, per = 24, 4
        data = {(t, k): codec.corpus_file(1 if (t + k) % 3 == 0 else 0, 1000 + 7 * t + k, sizes[(3 * t + k) % len(sizes)]) for t in range(n_threads) for k in range(per)}
        algo = {(t, k): pna.ALGO_DEFLATE if (t + k) % 5 == 0 else pna.ALGO_ZSTD for (t, k) in data}
        got, errs = {}, []
        start = threading.Barrier(n_threads)

        class Sink:
            def __init__(self): self.parts, self.tids = [], set()
            def write(self, b): self.parts.append(bytes(b)); self.tids.add(threading.get_ident())

        def worker(t):
            try:
                start.wait()
                for k in range(per):
                    w = ctx.writer(Sink(), algo=algo[(t, k)])
                    d = data[(t, k)]
                    for i in range(0, len(d), 99991):
                        w.write(d[i:i + 99991])
                    sink = w.try_into_inner()
                    assert sink.tids <= {threading.get_ident()}            # W::write is never called from a foreign thread
                    got[(t, k)] = b"".join(sink.parts)
            except Exception as e:  # noqa: BLE001
                errs.append(repr(e))
        th = [threading.Thread(target=worker, args=(t,)) for t in range(n_threads)]
        for x in th: x.start()
        for x in th: x.join()
        assert not errs, errs[:3]
        p, dp = _params(codec), codec.deflate_default_params()
        for key, d in data.items():
            want = codec.deflate_model_compress(d, dp) if algo[key] == pna.ALGO_DEFLATE else codec.model_compress(d, p)
            assert got[key] == want, key
        batches, entries, largest = ctx.stream_stats()
        assert entries == n_threads * per and batches < entries and largest > 1, (batches, entries, largest)
        # the native fan-out used for the rate measurement gives the same total
        secs, out_bytes = ctx.bench_stream_threads([data[k] for k in sorted(data) if algo[k] == pna.ALGO_ZSTD], threads=16)
        assert out_bytes == sum(len(got[k]) for k in sorted(data) if algo[k] == pna.ALGO_ZSTD) and secs > 0
    finally:
        ctx.close()


def test_stream_spills_to_pageable_memory(pna, codec, monkeypatch):
    """write() fills page-locked slabs of the context's pool; with the pool capped at one 64 MiB arena a 66 MiB stream must continue in
    pageable memory (and a second writer finds the pool empty from its first byte) -- the streams stay equal to the oracle's."""
    import torch  # noqa: F401
    monkeypatch.setenv("PNA_STREAM_POOL_MIB", "64")
    ctx = headline_context(pna)
    try:
        big = b"".join(codec.corpus_file(0, 500 + i, 1 << 20) for i in range(6)) * 11          # 66 MiB

        class Sink:
            def __init__(self): self.parts = []
            def write(self, b): self.parts.append(bytes(b))
        w1 = ctx.writer(Sink())
        for i in range(0, len(big), 5 << 20):
            w1.write(big[i:i + (5 << 20)])
        small = codec.corpus_file(1, 9, 300000)
        w2 = ctx.writer(Sink(), algo=pna.ALGO_DEFLATE)          # the pool is exhausted: pageable from the start
        w2.write(small)
        got2 = b"".join(w2.try_into_inner().parts)
        got1 = b"".join(w1.try_into_inner().parts)
        assert got2 == codec.deflate_model_compress(small)
        assert got1 == codec.model_compress(big, _params(codec))
        pieces = ctx.compress_solid(small)                       # pna_gpu_compress_solid rides on the same stream
        assert b"".join(pieces) == codec.model_compress(small, _params(codec)) and max(len(x) for x in pieces) <= 32768
    finally:
        ctx.close()


def test_create_archive_round_trip(gpu_ctx, pna, pf, codec):
    """cli/tests/cli/combination.rs style: create -> read back -> trees equal; order == argv order."""
    names, ents = [], []
    for root, _, files in os.walk(os.path.join(GOLDEN, "raw")):
        for f in sorted(files):
            p = os.path.join(root, f)
            names.append(os.path.relpath(p, GOLDEN)); ents.append(open(p, "rb").read())
    names += [f"corpus/f{i:05d}.txt" for i in range(6)]
    ents += [codec.corpus_file(0, i, 200000 + 4099 * i) for i in range(6)]
    for solid in (False, True):
        arc = pna.create_archive(gpu_ctx, names, ents, algo=pna.ALGO_ZSTD, solid=solid)
        _, items = pf.read_archive(arc)
        if solid:
            assert len(items) == 1 and items[0].compression == 2
            plain = codec.decode_payload(2, items[0].data, 64 << 20)
            if codec.system_libzstd() is not None:
                assert codec.libzstd_decompress_stream(items[0].data, 64 << 20) == plain
            inner = pf.read_solid_inner(plain)
            assert [(e.name, e.data) for e in inner] == list(zip(names, ents))
        else:
            assert [it.name for it in items] == names
            for it, e in zip(items, ents):
                assert it.compression == 2 and it.raw_file_size == len(e) and [t for t, _ in it.chunks] == [b"FHED", b"fSIZ", b"FDAT", b"FEND"]
                assert codec.decode_payload(2, it.data, len(e) + 64) == e
            assert items[names.index("raw/empty.txt")].data == bytes.fromhex("28B52FFD2000010000")


def test_device_batch_properties_256mib(gpu_ctx, pna, codec):
    """256 x 1 MiB resident in HBM: determinism, exact offsets, every entry decodes, sampled entries bit-exact."""
    import torch
    n, L = 256, 1 << 20
    src = torch.empty(n * L + 8192, dtype=torch.uint8, device="cuda")
    gpu_ctx.corpus_fill_device(0, 1000, n, L, L, src.data_ptr())
    cap = n * pna.bound(pna.ALGO_ZSTD, L)
    dst = torch.empty(cap, dtype=torch.uint8, device="cuda")
    offs = gpu_ctx.compress_batch_device(src.data_ptr(), [i * L for i in range(n + 1)], [L] * n, dst.data_ptr(), cap)
    assert offs[0] == 0 and all(offs[i] < offs[i + 1] for i in range(n))
    out1 = dst[:offs[-1]].cpu().numpy().tobytes()
    dst.zero_()
    offs2 = gpu_ctx.compress_batch_device(src.data_ptr(), [i * L for i in range(n + 1)], [L] * n, dst.data_ptr(), cap)
    assert offs2 == offs and dst[:offs[-1]].cpu().numpy().tobytes() == out1
    p = _params(codec)
    dec = codec.libzstd_decompress_stream if codec.system_libzstd() is not None else codec.zstd_decompress
    for i in range(n):
        want = codec.corpus_file(0, 1000 + i, L)
        assert dec(out1[offs[i]:offs[i + 1]], L) == want, i
        if i % 32 == 0:
            assert out1[offs[i]:offs[i + 1]] == codec.model_compress(want, p), i
    assert 2.3 < n * L / offs[-1] < 3.2


def test_full_size_properties_10k_x_1mib(big_ctx, pna, codec):
    """BASELINE.json configs[1] at full size through size-independent properties: offsets partition the output,
    the run is reproducible (checksum of the whole stream), sampled entries decode on the host / are bit-exact, and ALL
    entries round-trip through the device decoder."""
    import torch
    gpu_ctx = big_ctx
    n, L = 10000, 1 << 20
    free, _ = torch.cuda.mem_get_info()
    assert free >= 120 * (1 << 30), f"the headline configuration needs 120 GiB of free HBM, found {free >> 30} GiB (an MI355X has 288 GB)"
    src = torch.empty(n * L + 8192, dtype=torch.uint8, device="cuda")
    gpu_ctx.corpus_fill_device(0, 0, n, L, L, src.data_ptr())
    cap = n * pna.bound(pna.ALGO_ZSTD, L)
    dst = torch.empty(cap, dtype=torch.uint8, device="cuda")
    so, sl = [i * L for i in range(n + 1)], [L] * n
    offs = gpu_ctx.compress_batch_device(src.data_ptr(), so, sl, dst.data_ptr(), cap)
    assert len(offs) == n + 1 and offs[0] == 0 and all(offs[i] < offs[i + 1] for i in range(n))
    t = gpu_ctx.timing()
    assert t.in_bytes == n * L and t.out_bytes == offs[-1] and t.n_blocks == n * 8
    crc1 = zlib.crc32(dst[:offs[-1]].cpu().numpy().tobytes())
    dst.zero_()
    offs2 = gpu_ctx.compress_batch_device(src.data_ptr(), so, sl, dst.data_ptr(), cap)
    host = dst[:offs[-1]].cpu().numpy().tobytes()
    assert offs2 == offs and zlib.crc32(host) == crc1
    p = _params(codec)
    dec = codec.libzstd_decompress_stream if codec.system_libzstd() is not None else codec.zstd_decompress
    for i in list(range(0, n, 397)) + [n - 1]:
        want = codec.corpus_file(0, i, L)
        assert dec(host[offs[i]:offs[i + 1]], L) == want, i
    for i in (0, 4999, 9999):
        assert host[offs[i]:offs[i + 1]] == codec.model_compress(codec.corpus_file(0, i, L), p), i
    assert 2.3 < n * L / offs[-1] < 3.2
    # every entry, every byte: decoded on the device and compared with the source in HBM (the sampled entries above went
    # through the independent host decoders)
    back = torch.zeros(n * L + 64, dtype=torch.uint8, device="cuda")
    gpu_ctx.decompress_batch_device(dst.data_ptr(), offs[:n], [offs[i + 1] - offs[i] for i in range(n)], back.data_ptr(), so[:n], sl)
    assert torch.equal(back[:n * L], src[:n * L])
    del back
    # ... and ALL 10 000 entries through an INDEPENDENT decoder as well (the system's libzstd, multi-frame streaming decode as zstd-rs does
    # it, on a pool of host threads), compared with the source copied out of HBM: not one entry rests on this repository's decoder alone
    if codec.system_libzstd() is not None:
        import numpy as np
        from concurrent.futures import ThreadPoolExecutor
        host_src = src[:n * L].cpu().numpy()

        def check(i):
            got = np.frombuffer(codec.libzstd_decompress_stream(host[offs[i]:offs[i + 1]], L), dtype=np.uint8)
            return len(got) == L and bool(np.array_equal(got, host_src[i * L:(i + 1) * L]))
        with ThreadPoolExecutor(max_workers=min(32, (os.cpu_count() or 8))) as ex:
            ok = list(ex.map(check, range(n)))
        assert all(ok), [i for i, v in enumerate(ok) if not v][:8]


def test_deflate_bit_exact_and_inflatable(gpu_ctx, pna, codec):
    """Compression::Deflate on the device: zlib streams equal to the model, inflate with stdlib zlib."""
    cases = _cases(codec)
    names = sorted(cases)
    outs = gpu_ctx.compress_batch([cases[k] for k in names], algo=pna.ALGO_DEFLATE)
    for k, o in zip(names, outs):
        d = cases[k]
        assert zlib.decompress(o) == d, k
        assert o == codec.deflate_model_compress(d), k
        assert len(o) <= pna.bound(pna.ALGO_DEFLATE, len(d)), k
    assert outs[names.index("empty")] == bytes.fromhex("789C030000000001")


def test_deflate_config0_archive(gpu_ctx, pna, pf, codec):
    """BASELINE.json configs[0]: 100 x 64 KiB random-text files, Compression::Deflate -> archive -> read back."""
    names = [f"corpus/f{i:05d}.txt" for i in range(100)]
    ents = [codec.corpus_file(1, i, 65536) for i in range(100)]
    for solid in (False, True):
        arc = pna.create_archive(gpu_ctx, names, ents, algo=pna.ALGO_DEFLATE, solid=solid)
        _, items = pf.read_archive(arc)
        if solid:
            inner = pf.read_solid_inner(codec.decode_payload(1, items[0].data, 16 << 20))
            assert [(e.name, e.data) for e in inner] == list(zip(names, ents))
        else:
            assert [it.name for it in items] == names and all(it.compression == 1 for it in items)
            assert all(codec.decode_payload(1, it.data, 1 << 20) == e for it, e in zip(items, ents))
            ratio = sum(map(len, ents)) / sum(len(it.data) for it in items)
            assert ratio > 2.0


def test_deflate_many_small_entries(gpu_ctx, pna, codec):
    """BASELINE.json configs[4] shape at reduced count: 4 KiB entries (one block, one segment each)."""
    n = 2000
    ents = [codec.corpus_file(1, 100 + i, 4096) for i in range(n)]
    outs = gpu_ctx.compress_batch(ents, algo=pna.ALGO_DEFLATE)
    for i in range(0, n, 37):
        assert zlib.decompress(outs[i]) == ents[i]
        assert outs[i] == codec.deflate_model_compress(ents[i])
    assert all(zlib.decompress(o) == e for o, e in zip(outs[:200], ents[:200]))


def _short_cases(codec):
    """Entries whose segments are SHORT (at most 4 096 bytes, and 4 097 .. 16 384: the two tiers of the small geometry of the match finder, k_lzms) around the
    thresholds, entries whose LAST segment is short behind long ones, and ordinary ones in between -- one batch, so that all geometries' kernels run side by side."""
    t = codec.corpus_file(0, 77, (1 << 20) + 5000)
    cases = {"empty": b"", "one": b"z", "seven": b"abcdefg", "eight": b"abcdefgh", "nine": b"abcdefghi", "t255": t[:255], "t256": t[:256], "t257": t[:257],
             "t511": t[100:611], "t1000": t[:1000], "t4095": t[:4095], "t4096": t[:4096], "t4097": t[:4097], "t5000": t[:5000], "t70000": t[:70000],
             "seg+100": t[:(1 << 20) + 100], "seg+4096": t[:(1 << 20) + 4096], "seg+4097": t[:(1 << 20) + 4097],
             "rep4096": (t[:300] * 14)[:4096], "zeros4096": bytes(4096), "noise3000": codec.corpus_file(2, 5, 3000), "words4096": codec.corpus_file(1, 8, 4096),
             "ab": b"ab" * 2000, "period7": bytes((i * 37) & 0xFF for i in range(7)) * 500,
             # the second tier (4 097 .. 16 384 bytes) and its upper edge
             "t8191": t[:8191], "t8192": t[:8192], "t8193": t[:8193], "t12000": t[300:12300], "t16383": t[:16383], "t16384": t[:16384], "t16385": t[:16385],
             "seg+9000": t[:(1 << 20) + 9000], "rep16384": (t[:700] * 24)[:16384], "noise9000": codec.corpus_file(2, 6, 9000), "zeros16384": bytes(16384)}
    for i in range(40):
        cases[f"mix{i:02d}"] = codec.corpus_file(i & 1, 500 + i, 37 + 97 * i)
    return cases


@pytest.mark.parametrize("form", ["split", "one_kernel", "wave_parse", "no_workspace"])
def test_short_segments_take_the_small_geometry(pna, codec, form):
    """Segments of at most 4 096 bytes are matched by one wave each in sub-tiles of 256 positions (with k_lzm's tile of 4 096 they would find nothing);
    whatever form the LZ stage takes for the rest of the batch -- split, one kernel, the wave-per-region parse, no words workspace for the long segments --
    every stream is the model's (oracle: small_seg / mtile), for every level set of both codecs, and the short text entries now do hold matches."""
    cases = _short_cases(codec)
    names = sorted(cases)
    data = [cases[k] for k in names]
    with headline_context(pna) as ctx:
        if form == "one_kernel": ctx.set_option("lz_split", 0)
        if form == "wave_parse": ctx.set_option("lz_split", 2)
        if form == "no_workspace": ctx.set_option("lz_pbuf_fail", 1)
        for level in (1, 2, 3, 7, 19):
            outs = ctx.compress_batch(data, level=level)
            pz = codec.params_for_level(level)
            bad = [k for k, d, o in zip(names, data, outs) if o != codec.model_compress(d, pz)]
            assert not bad, (form, level, bad[:6])
            assert all(codec.zstd_decompress(o, len(d)) == d for d, o in zip(data, outs))
        for level in (1, 6, 9):
            outs = ctx.compress_batch(data, algo=pna.ALGO_DEFLATE, level=level)
            pd = codec.params_for_level(level, deflate=True)
            bad = [k for k, d, o in zip(names, data, outs) if o != codec.deflate_model_compress(d, pd)]
            assert not bad, (form, "deflate", level, bad[:6])
            assert all(zlib.decompress(o) == d for d, o in zip(data, outs))
        d = cases["t4096"]
        o6 = ctx.compress_batch([d], algo=pna.ALGO_DEFLATE)[0]
        assert len(o6) < len(zlib.compress(d, 6)) + 40 and len(o6) < 0.56 * len(d)       # matches inside a 4 KiB entry: without them Huffman alone gives ~0.58
        # the option that switches the small geometry off: the model without it
        ctx.set_option("small_geometry", 0)
        p0 = codec.params_for_level(3); p0.small_seg = 0
        assert ctx.compress_batch(data[:24], level=3) == [codec.model_compress(x, p0) for x in data[:24]]


def test_deflate_wave_per_entry_form_equals_the_model(gpu_ctx, pna, codec):
    """Batches of >= 4 096 entries of at most 32 KiB build their Huffman codes with ONE WAVE per entry (k_dstats<64>) instead of a workgroup: every
    stream must still be the model's, for ragged sizes -- empty, a few bytes, one symbol only, 32 KiB of text and of noise -- in one batch."""
    import random
    rnd = random.Random(5)
    sizes = [0, 1, 2, 3, 7, 64, 257, 4095, 4096, 4097, 16384, 32768, 32767] + [rnd.choice((rnd.randrange(1, 600), rnd.randrange(600, 9000), 4096)) for _ in range(4200)]
    ents = []
    for i, n in enumerate(sizes):
        k = i % 5
        if k == 3: ents.append(bytes([65 + i % 7]) * n)                          # one symbol: the single-code corner of all three code builds
        elif k == 4: ents.append(rnd.randbytes(n))                                # noise: every literal occurs, no matches, stored blocks
        else: ents.append(codec.corpus_file(k & 1, 300 + i, n) if n else b"")
    outs = gpu_ctx.compress_batch(ents, algo=pna.ALGO_DEFLATE)
    assert len(outs) == len(ents)
    bad = [i for i, (o, e) in enumerate(zip(outs, ents)) if o != codec.deflate_model_compress(e)]
    assert not bad, (bad[:8], [sizes[i] for i in bad[:8]])
    assert all(zlib.decompress(o) == e for o, e in zip(outs[::9], ents[::9]))


def test_zstd_many_small_entries_equal_the_model(gpu_ctx, pna, codec):
    """Batches of >= 4 096 entries of at most 32 KiB take the small-entry forms of the zstd path together: the short-segment match kernel, k_stats with lean
    histograms and the wave-built tree description, predefined tables copied from the device's, the sequence coder with a lane per segment, the write kernel
    with a wave per block.  Every stream must be the model's -- ragged sizes, one-symbol entries (RLE literals), noise (raw blocks), text -- and decode."""
    import random
    rnd = random.Random(11)
    sizes = [0, 1, 2, 5, 8, 9, 63, 64, 255, 256, 257, 1000, 4095, 4096, 4097, 8192, 16384, 16385, 32768] + [rnd.choice((rnd.randrange(1, 700), rnd.randrange(700, 9000), 4096, 12000)) for _ in range(4200)]
    ents = []
    for i, n in enumerate(sizes):
        k = i % 5
        if k == 3: ents.append(bytes([97 + i % 5]) * n)
        elif k == 4: ents.append(rnd.randbytes(n))
        else: ents.append(codec.corpus_file(k & 1, 900 + i, n) if n else b"")
    for level in (3, 1):
        outs = gpu_ctx.compress_batch(ents, level=level)
        p = codec.params_for_level(level)
        bad = [i for i, (o, e) in enumerate(zip(outs, ents)) if o != codec.model_compress(e, p)]
        assert not bad, (level, bad[:8], [sizes[i] for i in bad[:8]])
        assert all(codec.zstd_decompress(o, len(e)) == e for o, e in zip(outs[::7], ents[::7]))
    assert gpu_ctx.decompress_batch(outs[:600], [len(e) for e in ents[:600]]) == ents[:600]


@pytest.mark.parametrize("algo_name", ["zstd", "deflate"])
def test_archive_assembled_in_hbm_equals_host_framing(gpu_ctx, pna, pf, codec, algo_name):
    """pna_gpu_create_archive_device: payloads written at their archive offsets + k_frame (prefix, FDAT CRC, FEND) must give
    the very bytes pna_create_archive() produces through the host-side chunk writer, and the oracle's reader parses them."""
    import torch
    algo = pna.ALGO_ZSTD if algo_name == "zstd" else pna.ALGO_DEFLATE
    lens = [0, 1, 5, 4095, 16372, 16373, 16384, 70001, 131072, 131073, 300000, (1 << 20), (1 << 20) + 1, 2500000, 12, 65536]
    ents = [codec.corpus_file(i % 2, 50 + i, n) if n else b"" for i, n in enumerate(lens)]
    ents[3] = bytes(4095)                                  # rle / tiny payloads shift every later entry to odd offsets
    names = [f"dir{i % 3}/./f{i:03d}.txt" if i % 4 else f"/abs//n{i}" for i in range(len(lens))]
    offs, pos = [], 0
    for e in ents:
        offs.append(pos); pos = (pos + len(e) + 15) & ~15
    src = torch.zeros(pos + 8192, dtype=torch.uint8, device="cuda")
    for o, e in zip(offs, ents):
        if e:
            src[o:o + len(e)] = torch.frombuffer(bytearray(e), dtype=torch.uint8).cuda()
    cap = pna.archive_bound(algo, names, lens)
    dst = torch.full((cap,), 0xA5, dtype=torch.uint8, device="cuda")
    total, eoff = gpu_ctx.create_archive_device(names, src.data_ptr(), offs, lens, dst.data_ptr(), cap, algo=algo)
    got = dst[:total].cpu().numpy().tobytes()
    # expected bytes, built without k_frame: payloads from the batch API, framing by (1) the oracle's container writer
    # and (2) the host chunk writer of include/pna_archive.h (host CRC-32)
    payloads = gpu_ctx.compress_batch(ents, algo=algo)
    want = pf.write_archive_header() + b"".join(
        pf.write_normal_entry(pf.file_entry_header(algo, pf.sanitize_name(nm)), [pl], len(e)) for nm, pl, e in zip(names, payloads, ents)
    ) + pf.finalize_archive()

    class Sink:
        def __init__(self): self.parts = []
        def write(self, b): self.parts.append(b)
    sk = Sink(); arc = pna.Archive(sk)
    for nm, pl, e in zip(names, payloads, ents):
        arc.add_file(nm, algo, len(e), pl)
    arc.finalize()
    assert b"".join(sk.parts) == want
    assert len(got) == len(want) and got == want
    assert pna.create_archive(gpu_ctx, names, ents, algo=algo, solid=False) == want      # pipelined host path, one sub-batch
    assert bytes(dst[total:total + 16].cpu().numpy()) == b"\xA5" * 16            # nothing written past the archive
    _, items = pf.read_archive(got)                         # the reader checks every chunk CRC
    assert [it.name for it in items] == [it.name for it in pf.read_archive(want)[1]]
    for it, e, o in zip(items, ents, eoff):
        assert got[o + 4:o + 8] == b"FHED" and it.raw_file_size == len(e)
        assert codec.decode_payload(algo, it.data, len(e) + 64) == e
    assert gpu_ctx.timing().ms_frame > 0


def test_archive_in_hbm_full_size_crc_property(gpu_ctx, pna, pf):
    """2048 x 1 MiB in HBM: every chunk CRC of the device-assembled archive verifies (host CRC-32 over all chunks)."""
    import torch
    n, L = 2048, 1 << 20
    src = torch.empty(n * L + 8192, dtype=torch.uint8, device="cuda")
    gpu_ctx.corpus_fill_device(0, 7000, n, L, L, src.data_ptr())
    names = [f"enwik/part{i:05d}" for i in range(n)]
    cap = pna.archive_bound(pna.ALGO_ZSTD, names, [L] * n)
    dst = torch.empty(cap, dtype=torch.uint8, device="cuda")
    total, eoff = gpu_ctx.create_archive_device(names, src.data_ptr(), [i * L for i in range(n)], [L] * n, dst.data_ptr(), cap)
    arc = dst[:total].cpu().numpy().tobytes()
    _, items = pf.read_archive(arc)
    assert len(items) == n and [it.name for it in items] == names and all(it.raw_file_size == L for it in items)
    assert eoff[0] == 28 and eoff[-1] + 12 == total


def test_host_pipeline_many_sub_batches(gpu_ctx, pna, pf, codec):
    """pna_gpu_create_archive_host with several sub-batches: both staging slots in flight, sink pieces in order,
    result identical to the one-shot in-HBM archive of the same entries."""
    import torch
    n, L = 700, 1 << 20
    src = torch.empty(n * L + 8192, dtype=torch.uint8, device="cuda")
    gpu_ctx.corpus_fill_device(0, 300, n, L, L, src.data_ptr())
    host = src[:n * L].cpu().numpy()
    ents = [host[i * L:(i + 1) * L].tobytes() for i in range(n)]
    ents[5] = b""; ents[6] = ents[6][:12345]
    names = [f"p/{i:04d}" for i in range(n)]
    with gpu_ctx.options(sub_mib=(128, 1024)):           # several sub-batches (the default window is 1 GiB per slot)
        arc = pna.create_archive(gpu_ctx, names, ents)
    _, items = pf.read_archive(arc)
    assert [it.name for it in items] == names and [it.raw_file_size for it in items] == [len(e) for e in ents]
    for i in (0, 5, 6, 255, 256, 257, 511, 512, 699):
        assert codec.decode_payload(2, items[i].data, L + 64) == ents[i]
    lens = [len(e) for e in ents]
    offs, pos = [], 0
    for l in lens:
        offs.append(pos); pos = (pos + l + 15) & ~15
    dsrc = torch.zeros(pos + 8192, dtype=torch.uint8, device="cuda")
    for o, e in zip(offs, ents):
        if e:
            dsrc[o:o + len(e)] = torch.frombuffer(bytearray(e), dtype=torch.uint8).cuda()
    cap = pna.archive_bound(pna.ALGO_ZSTD, names, lens)
    dst = torch.empty(cap, dtype=torch.uint8, device="cuda")
    total, _ = gpu_ctx.create_archive_device(names, dsrc.data_ptr(), offs, lens, dst.data_ptr(), cap)
    assert dst[:total].cpu().numpy().tobytes() == arc


def test_host_pipelines_after_a_failing_sink(gpu_ctx, pna):
    """A sink that fails on its third call -- behind the head and one piece, with the stager thread (or the next window's assembly) ahead and copies
    in flight: pna_gpu_create_archive_host over five sub-batches and pna_gpu_create_solid_archive_host over six windows return PNA_E_SINK with
    everything of the call stopped and drained, and the same context then writes the archive of the device entry point, byte for byte."""
    import ctypes
    import torch
    n, L = 48, 3 << 19
    src = torch.empty(n * L + 8192, dtype=torch.uint8, device="cuda")
    gpu_ctx.corpus_fill_device(0, 310, n, L, L, src.data_ptr())
    host = src[:n * L].cpu().numpy()
    ents = [host[i * L:(i + 1) * L].tobytes() for i in range(n)]
    names = [f"q/{i:03d}" for i in range(n)]
    lib = pna.load_library()

    def host_create(entry_point, k, fail_at):
        out, calls = bytearray(), [0]

        def _sink(_u, buf, size):
            calls[0] += 1
            if calls[0] == fail_at:
                return 1
            out.extend((ctypes.c_char * size).from_address(buf))
            return 0
        a_names = (ctypes.c_char_p * k)(*[s.encode() for s in names[:k]])
        a_src = (ctypes.c_void_p * k)(*[ctypes.cast(ctypes.c_char_p(e), ctypes.c_void_p) for e in ents[:k]])
        a_len = (ctypes.c_size_t * k)(*[L] * k)
        gpu_ctx._check(entry_point(gpu_ctx._h, pna.ALGO_ZSTD, pna.LEVEL_DEFAULT, k, a_names, a_src, a_len, pna.SINK_FN(_sink), None))
        return bytes(out)

    def device_create(k, solid):
        offs = [i * L for i in range(k)]                        # (L is a multiple of 16)
        cap = (pna.solid_archive_bound if solid else pna.archive_bound)(pna.ALGO_ZSTD, names[:k], [L] * k)
        dst = torch.empty(cap, dtype=torch.uint8, device="cuda")
        if solid:
            total = gpu_ctx.create_solid_archive_device(names[:k], src.data_ptr(), offs, [L] * k, dst.data_ptr(), cap, algo=pna.ALGO_ZSTD)
        else:
            total, _ = gpu_ctx.create_archive_device(names[:k], src.data_ptr(), offs, [L] * k, dst.data_ptr(), cap)
        return dst[:total].cpu().numpy().tobytes()

    try:
        gpu_ctx.set_option("sub_mib", 16)
        gpu_ctx.set_option("solid_win_mib", 1)
        for entry_point, k, solid in ((lib.pna_gpu_create_archive_host, n, False), (lib.pna_gpu_create_solid_archive_host, 4, True)):
            with pytest.raises(pna.PnaGpuError) as err:
                host_create(entry_point, k, 3)
            assert err.value.code == pna.E_SINK
            assert host_create(entry_point, k, 0) == device_create(k, solid)
    finally:
        gpu_ctx.set_option("sub_mib", 1024)
        gpu_ctx.set_option("solid_win_mib", 256)


def test_many_short_matches_bit_exact(gpu_ctx, pna, codec):
    """Adversarial for the per-block sequence capacity and for the merge of the waves' parses: 7-byte words from a small
    vocabulary (back-to-back minimum-length matches, ends that fall 1-2 bytes behind the running end)."""
    import random
    rnd = random.Random(11)
    vocab = [bytes(rnd.randrange(97, 123) for _ in range(7)) for _ in range(48)]
    d1 = b"".join(rnd.choice(vocab) for _ in range(60000))                      # 420 000 B
    vocab2 = [bytes(rnd.randrange(65, 91) for _ in range(rnd.choice((6, 7, 8, 9)))) for _ in range(300)]
    d2 = b"".join(rnd.choice(vocab2) for _ in range(150000))[: (1 << 20) + 333]
    for d in (d1, d2):
        out = gpu_ctx.compress_batch([d])[0]
        assert out == codec.model_compress(d, _params(codec))
        assert codec.zstd_decompress(out, len(d) + 64) == d
        dz = gpu_ctx.compress_batch([d], algo=pna.ALGO_DEFLATE)[0]
        assert dz == codec.deflate_model_compress(d) and zlib.decompress(dz) == d


@pytest.mark.parametrize("algo_name", ["zstd", "deflate"])
def test_solid_archive_assembled_in_hbm(gpu_ctx, pna, pf, codec, algo_name):
    """pna_gpu_create_solid_archive_device: inner STORE records (device CRC-32) -> one compressed stream -> one SDAT chunk per
    segment.  The oracle's reader checks every chunk CRC (outer and inner) and the inner entries must equal the inputs; the
    serialised inner stream must equal the oracle writer's bytes."""
    import torch
    algo = pna.ALGO_ZSTD if algo_name == "zstd" else pna.ALGO_DEFLATE
    lens = [0, 1, 3, 4095, 65536, 70001, (1 << 20) - 13, (1 << 20), (1 << 20) + 1, 2500000, 12, 0, 300000]
    ents = [codec.corpus_file(i % 2, 80 + i, n) if n else b"" for i, n in enumerate(lens)]
    names = [f"solid/d{i % 2}/f{i:03d}.bin" for i in range(len(lens))]
    offs, pos = [], 0
    for e in ents:
        offs.append(pos); pos = (pos + len(e) + 15) & ~15
    src = torch.zeros(pos + 8192, dtype=torch.uint8, device="cuda")
    for o, e in zip(offs, ents):
        if e:
            src[o:o + len(e)] = torch.frombuffer(bytearray(e), dtype=torch.uint8).cuda()
    cap = pna.solid_archive_bound(algo, names, lens)
    dst = torch.full((cap,), 0x5A, dtype=torch.uint8, device="cuda")
    total = gpu_ctx.create_solid_archive_device(names, src.data_ptr(), offs, lens, dst.data_ptr(), cap, algo=algo)
    arc = dst[:total].cpu().numpy().tobytes()
    assert bytes(dst[total:total + 16].cpu().numpy()) == b"\x5A" * 16
    _, items = pf.read_archive(arc)
    assert len(items) == 1 and items[0].compression == algo
    plain = codec.decode_payload(algo, items[0].data, 16 << 20)
    want_plain = b"".join(pf.write_normal_entry(pf.file_entry_header(0, pf.sanitize_name(nm)), [e] if e else [], len(e)) for nm, e in zip(names, ents))
    assert plain == want_plain
    inner = pf.read_solid_inner(plain)
    assert [(e.name, e.data) for e in inner] == list(zip(names, ents))
    # the host entry point takes the same route
    assert pna.create_archive(gpu_ctx, names, ents, algo=algo, solid=True) == arc


def test_solid_archive_streams_through_windows(gpu_ctx, pna, pf, codec):
    """pna_gpu_create_solid_archive_host (zstd): the serialised inner entries go to the device in windows (option solid_win_mib; two page-locked slots each way
    whatever the archive's size) -- SolidArchive::add_entry streams entries into one encoder (lib/src/archive/write.rs:575-580).  With windows of 1 MiB an
    entry spans several, chunk headers, FEND and the 4 CRC bytes of a data chunk fall on a window's edge in every way (the sweep moves the edge through them);
    every archive == the one assembled in HBM in one piece, and reads back."""
    import torch
    def device_one_shot(names, ents):
        offs, pos = [], 0
        for e in ents:
            offs.append(pos); pos = (pos + len(e) + 15) & ~15
        src = torch.zeros(pos + 8192, dtype=torch.uint8, device="cuda")
        for o, e in zip(offs, ents):
            if e:
                src[o:o + len(e)] = torch.frombuffer(bytearray(e), dtype=torch.uint8).cuda()
        lens = [len(e) for e in ents]
        cap = pna.solid_archive_bound(pna.ALGO_ZSTD, names, lens)
        dst = torch.zeros(cap, dtype=torch.uint8, device="cuda")
        total = gpu_ctx.create_solid_archive_device(names, src.data_ptr(), offs, lens, dst.data_ptr(), cap, algo=pna.ALGO_ZSTD)
        return dst[:total].cpu().numpy().tobytes()
    big = codec.corpus_file(0, 7001, 2600000)
    try:
        for win in (1, 2):
            gpu_ctx.set_option("solid_win_mib", win)
            for delta in range(0, 24):
                # the first entry's record ends `delta` bytes around the 1 MiB edge: its CRC field, FEND and the next entry's FHED straddle the edge in turn
                first = codec.corpus_file(1, 7100 + delta, (1 << 20) - 70 - delta)
                ents = [first, b"", big, b"", codec.corpus_file(0, 7002, 4096), codec.corpus_file(1, 7003, (1 << 20) + 5)] + ([] if delta % 3 else [b""])
                names = [f"s/{i}.bin" for i in range(len(ents))]
                got = pna.create_archive(gpu_ctx, names, ents, solid=True)
                if delta % 6 == 0 or win == 1:
                    assert got == device_one_shot(names, ents), (win, delta)
                if delta == 5:
                    assert [(n, d) for n, _, d in pna.extract_archive(gpu_ctx, got)] == list(zip(names, ents))
        gpu_ctx.set_option("solid_win_mib", 1)
        many = [codec.corpus_file(1, 7200 + i, 3000 + 37 * (i % 50)) for i in range(900)]              # many small inner entries: hundreds of chunks per window
        nm = [f"m/{i}" for i in range(len(many))]
        assert pna.create_archive(gpu_ctx, nm, many, solid=True) == device_one_shot(nm, many)
        assert pna.create_archive(gpu_ctx, [], [], solid=True) == device_one_shot([], [])
    finally:
        gpu_ctx.set_option("solid_win_mib", 256)


def test_archive_shards_concatenate(gpu_ctx, pna, pf, codec):
    """Two producers (ranks) each assemble their contiguous range of entries; head only on the first, AEND only on the last:
    the concatenation in rank order must be byte-identical to the archive one producer makes of all entries."""
    import torch
    shard = importlib.import_module("portable-network-archive_amd.shard")
    lens = [70000 + 977 * i for i in range(24)] + [0, 5, 1 << 20]
    ents = [codec.corpus_file(0, 400 + i, n) if n else b"" for i, n in enumerate(lens)]
    names = [f"s/{i:03d}" for i in range(len(lens))]
    offs, pos = [], 0
    for e in ents:
        offs.append(pos); pos = (pos + len(e) + 15) & ~15
    src = torch.zeros(pos + 8192, dtype=torch.uint8, device="cuda")
    for o, e in zip(offs, ents):
        if e:
            src[o:o + len(e)] = torch.frombuffer(bytearray(e), dtype=torch.uint8).cuda()
    cap = pna.archive_bound(pna.ALGO_ZSTD, names, lens)
    dst = torch.empty(cap, dtype=torch.uint8, device="cuda")
    total, _ = gpu_ctx.create_archive_device(names, src.data_ptr(), offs, lens, dst.data_ptr(), cap)
    whole = dst[:total].cpu().numpy().tobytes()
    parts = []
    bounds = shard.partition_entries(lens, 2)
    for r, (a, b) in enumerate(bounds):
        part = (pna.PART_HEAD if r == 0 else 0) | (pna.PART_TAIL if r == len(bounds) - 1 else 0)
        t, _ = gpu_ctx.create_archive_device(names[a:b], src.data_ptr(), offs[a:b], lens[a:b], dst.data_ptr(), cap, part=part)
        parts.append(dst[:t].cpu().numpy().tobytes())
    assert b"".join(parts) == whole
    assert [it.name for it in pf.read_archive(whole)[1]] == names


def test_device_decoder_round_trips_cases(gpu_ctx, pna, codec):
    """k_zdec (the read side, lib/src/entry/read.rs:171-190): every case the encoder tests use, decoded on the device."""
    cases = _cases(codec)
    names = list(cases)
    outs = gpu_ctx.compress_batch([cases[k] for k in names])
    back = gpu_ctx.decompress_batch(outs, [len(cases[k]) for k in names])
    for k, b in zip(names, back):
        assert b == cases[k], k


def test_device_decoder_reads_reference_fixtures(gpu_ctx, pna, pf, codec):
    """Frames written by the reference's own encoder (libzstd through zstd-rs: 2 MiB window, per-block tables, repeat
    offsets): the FDAT payloads of the golden archives decode to resources/test/raw/*."""
    for arc in ("zstd.pna", "zstd_with_raw_file_size.pna", "zstd_keep_all.pna"):
        _, items = pf.read_archive(open(os.path.join(GOLDEN, arc), "rb").read())
        items = [it for it in items if getattr(it, "kind", 1) == 0 and it.compression == 2]
        raws = []
        for it in items:
            path = os.path.join(GOLDEN, it.name)
            # raw/images/icon.bmp (4 MiB, ONE frame with a 2 MiB window) exists only inside the fixtures: the oracle decoder is its reference
            raws.append(open(path, "rb").read() if os.path.isfile(path) else codec.decode_payload(2, it.data, 8 << 20))
        sel = [(it, r) for it, r in zip(items, raws) if r is not None]
        assert any(len(r) > (4 << 20) for _, r in sel)
        back = gpu_ctx.decompress_batch([it.data for it, _ in sel], [len(r) for _, r in sel])
        for (it, r), b in zip(sel, back):
            assert b == r, (arc, it.name)


def test_device_decoder_rejects_corruption(gpu_ctx, pna, codec):
    d = codec.corpus_file(0, 77, 300000)
    out = bytearray(gpu_ctx.compress_batch([d])[0])
    good = bytes(out)
    with pytest.raises(pna.PnaGpuError):
        gpu_ctx.decompress_batch([good], [len(d) - 1])                  # size mismatch
    with pytest.raises(pna.PnaGpuError):
        gpu_ctx.decompress_batch([good[:-5]], [len(d)])                  # truncated
    out[0] ^= 0xFF
    with pytest.raises(pna.PnaGpuError):
        gpu_ctx.decompress_batch([bytes(out)], [len(d)])                 # bad magic
    assert gpu_ctx.decompress_batch([good], [len(d)])[0] == d            # the context stays usable


def test_device_round_trip_2gib_in_hbm(gpu_ctx, pna):
    """2 048 x 1 MiB: compress in HBM, decode in HBM, compare in HBM -- every byte of every entry."""
    import torch
    n, L = 2048, 1 << 20
    src = torch.empty(n * L + 8192, dtype=torch.uint8, device="cuda")
    gpu_ctx.corpus_fill_device(0, 9000, n, L, L, src.data_ptr())
    cap = n * pna.bound(pna.ALGO_ZSTD, L) + 64
    comp = torch.empty(cap, dtype=torch.uint8, device="cuda")
    offs = gpu_ctx.compress_batch_device(src.data_ptr(), [i * L for i in range(n + 1)], [L] * n, comp.data_ptr(), cap)
    back = torch.zeros(n * L + 64, dtype=torch.uint8, device="cuda")
    gpu_ctx.decompress_batch_device(comp.data_ptr(), offs[:n], [offs[i + 1] - offs[i] for i in range(n)], back.data_ptr(),
                                    [i * L for i in range(n)], [L] * n)
    assert torch.equal(back[:n * L], src[:n * L])


def test_error_codes_at_the_boundary(gpu_ctx, pna, codec):
    """Argument errors come back as codes (io::ErrorKind::InvalidInput in the reference's terms), the context stays usable."""
    import ctypes
    import torch
    L = pna.load_library()
    d = codec.corpus_file(0, 5, 100000)
    src = torch.zeros(len(d) + 8192, dtype=torch.uint8, device="cuda")
    src[:len(d)] = torch.frombuffer(bytearray(d), dtype=torch.uint8).cuda()
    dst = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")
    u64 = ctypes.c_uint64
    def call(algo, off, cap):
        out = (u64 * 2)()
        return L.pna_gpu_compress_batch_device(gpu_ctx._h, algo, pna.LEVEL_DEFAULT, 1, ctypes.c_void_p(src.data_ptr()), (u64 * 2)(off, 0),
                                               (u64 * 1)(len(d)), ctypes.c_void_p(dst.data_ptr()), cap, out, None)
    assert call(pna.ALGO_ZSTD, 0, 1 << 20) == 0
    assert call(pna.ALGO_ZSTD, 0, 1000) == -4                     # PNA_E_DSTSIZE
    assert call(pna.ALGO_ZSTD, 8, 1 << 20) == -2                  # PNA_E_INVAL: offset not 16-byte aligned
    assert call(3, 0, 1 << 20) == -7                              # PNA_E_UNSUPPORTED (xz)
    assert b"aligned" in L.pna_gpu_last_error(gpu_ctx._h) or True
    assert gpu_ctx.compress_batch([d])[0] == codec.model_compress(d, _params(codec))


@pytest.mark.parametrize("mcs", [1000, 4097, 65536, (1 << 20) + 1, 0])
def test_max_chunk_size_cuts_fdat_like_flatten_writer(gpu_ctx, pna, pf, codec, mcs):
    """FlattenWriter (lib/src/util/io.rs:60-77; FileEntryBuilder::max_chunk_size, lib/src/entry/builder/file.rs:105-112): an entry's stream becomes FDAT
    chunks of exactly max_chunk_size bytes, the last one the rest; 0 = u32::MAX.  The archive assembled in HBM (pna_gpu_create_archive_chunked_device),
    the bounded host pipeline (..._chunked_host) and the context option "max_chunk_size" behind the plain entry points must all give the bytes of the
    oracle's writer fed with the same streams -- plain and with AES-CTR (one keystream over all chunks, the IV a data piece of its own)."""
    import torch
    lens = [(3 << 20) + 4567, 1000, (2 << 20), 0, 999, 1001, 65537]
    ents = [codec.corpus_file(2 if i == 2 else 0, 600 + i, n) if n else b"" for i, n in enumerate(lens)]   # entry 2 is incompressible
    names = [f"big/{i}" for i in range(len(lens))]
    offs, pos = [], 0
    for e in ents:
        offs.append(pos); pos = (pos + len(e) + 15) & ~15
    src = torch.zeros(pos + 8192, dtype=torch.uint8, device="cuda")
    for o, e in zip(offs, ents):
        if e:
            src[o:o + len(e)] = torch.frombuffer(bytearray(e), dtype=torch.uint8).cuda()
    payloads = gpu_ctx.compress_batch(ents)
    big = pf.MAX_CHUNK_DATA_LENGTH
    want = pf.write_archive_header() + b"".join(
        pf.write_normal_entry(pf.file_entry_header(2, nm), pf.flatten_writer([pl], mcs or big) or [b""], len(e)) for nm, pl, e in zip(names, payloads, ents)
    ) + pf.finalize_archive()
    cap = pna.archive_chunked_bound(pna.ALGO_ZSTD, names, lens, mcs)
    dst = torch.full((cap + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    total, _ = gpu_ctx.create_archive_chunked_device(names, src.data_ptr(), offs, lens, dst.data_ptr(), cap, mcs)
    got = dst[:total].cpu().numpy().tobytes()
    assert got == want
    assert bytes(dst[total:total + 16].cpu().numpy()) == b"\xA5" * 16
    assert pna.create_archive_chunked(gpu_ctx, names, ents, mcs) == want
    with gpu_ctx.options(max_chunk_size=(mcs, 0)):
        assert pna.create_archive(gpu_ctx, names, ents) == want                     # the entry points without the parameter follow the option
    _, items = pf.read_archive(got)
    assert [codec.decode_payload(2, it.data, len(e) + 64) for it, e in zip(items, ents)] == ents
    if mcs:
        assert sum(1 for t, _ in items[0].chunks if t == b"FDAT") == -(-len(payloads[0]) // mcs)
    assert [(n, d) for n, _, d in pna.extract_archive(gpu_ctx, got)] == list(zip(names, ents))
    # AES-256-CTR: FDAT(iv) then the ciphertext in chunks of max_chunk_size
    key, phsf = pna.kdf_pbkdf2_sha256(b"password", bytes(range(16)), 1000)
    ivs = bytes((7 * i) & 0xFF for i in range(16 * len(ents)))
    ci = pna.Cipher(key, phsf, pna.MODE_CTR, ivs=ivs)
    ewant = pf.write_archive_header() + b"".join(
        pf.write_encrypted_file_entry(2, 1, 1, nm, phsf, ivs[16 * i:16 * i + 16], codec.aes_ctr(key, ivs[16 * i:16 * i + 16], pl), len(e), mcs or big)
        for i, (nm, pl, e) in enumerate(zip(names, payloads, ents))) + pf.finalize_archive()
    ecap = pna.archive_chunked_bound(pna.ALGO_ZSTD, names, lens, mcs, cipher=ci)
    edst = torch.zeros(ecap + 64, dtype=torch.uint8, device="cuda")
    etotal, _ = gpu_ctx.create_archive_chunked_device(names, src.data_ptr(), offs, lens, edst.data_ptr(), ecap, mcs, cipher=ci)
    assert edst[:etotal].cpu().numpy().tobytes() == ewant
    assert pna.create_archive_chunked(gpu_ctx, names, ents, mcs, cipher=ci) == ewant
    if mcs and mcs < 100000:
        # CBC chains the whole entry and GCM authenticates whole segments: entries beyond one chunk are refused, not written differently
        with pytest.raises(pna.PnaGpuError):
            pna.create_archive_chunked(gpu_ctx, names, ents, mcs, cipher=pna.Cipher(key, phsf, pna.MODE_CBC, ivs=ivs))

def test_single_frame_option(pna, pf, codec):
    """Option single_frame: a zstd entry is ONE frame whatever its size -- the blocks of the frame-per-segment form, the frame header in front of the first
    segment only and the last-block bit on the entry's last block only (SURVEY 8 a14's fallback should a reader ever refuse concatenated frames; the
    reference's own reader takes both: zstd::Decoder::with_buffer, lib/src/entry/read.rs:181).  Equal to the model with PNA_F_SINGLE_FRAME, exactly
    6 bytes per further segment shorter than the default form, one frame for every decoder -- the oracle's, libzstd, the device's --, in a batch call,
    in an archive assembled in HBM and read back by the extract driver, and for the solid stream."""
    import torch  # noqa: F401
    ents = [codec.corpus_file(0, 4500, (3 << 20) + 12345), b"", codec.corpus_file(1, 4501, 70000), codec.corpus_file(0, 4502, 1 << 20), codec.corpus_file(2, 4503, (1 << 20) + 1),
            codec.corpus_file(0, 4504, (2 << 20))]
    names = [f"sf/{i}" for i in range(len(ents))]
    with pna.Context(0) as ctx:
        ctx.set_option("latency_max_mib", 0)
        multi = ctx.compress_batch(ents)
        ctx.set_option("single_frame", 1)
        outs = ctx.compress_batch(ents)
        p = codec.params_for_level(3)
        p.flags |= 0x400
        for e, o, m in zip(ents, outs, multi):
            assert o == codec.model_compress(e, p)
            assert len(m) - len(o) == 6 * (max(1, -(-len(e) >> 20)) - 1)
            assert codec.zstd_frame_count(o, len(e) + 64) == 1
            assert codec.zstd_decompress(o, len(e)) == e
            if codec.system_libzstd() is not None:
                assert codec.libzstd_decompress_stream(o, len(e)) == e
        assert ctx.decompress_batch(outs, [len(e) for e in ents]) == ents
        arc = pna.create_archive(ctx, names, ents)
        _, items = pf.read_archive(arc)
        assert [it.data for it in items] == outs
        assert [(n, d) for n, _, d in pna.extract_archive(ctx, arc)] == list(zip(names, ents))
        solid = pna.create_archive(ctx, names, ents, solid=True)
        assert [(n, d) for n, _, d in pna.extract_archive(ctx, solid)] == list(zip(names, ents))
        ctx.set_option("latency_max_mib", 192)                     # the small-batch mode (smaller blocks, LZ units): same rule
        (o1,) = ctx.compress_batch([ents[0]])
        p1 = codec.params_for_level(3, blk_log=ctx.timing().blk_log)
        p1.flags |= 0x400
        assert o1 == codec.model_compress(ents[0], p1) and codec.zstd_frame_count(o1, len(ents[0]) + 64) == 1


def test_zero_staging_host_slots(gpu_ctx, pna, pf, codec):
    """pna_gpu_host_alloc: entries the host placed in a page-locked buffer of the library go to the device straight from there (no pageable ->
    page-locked staging copy; cli/src/command/core.rs:889-913 reads into memory the library could own).  Same archive, byte for byte, as from ordinary
    memory -- contiguous at a 16-byte stride (one copy per run), scattered with gaps, with empty entries in between, and mixed with an entry that lives
    elsewhere (the whole batch is staged then)."""
    ents = [codec.corpus_file(0, 4400 + i, n) for i, n in enumerate([300000, 0, 5, (1 << 20) + 3, 70001, 0, 999])]
    names = [f"slot/{i}" for i in range(len(ents))]
    want = pna.create_archive(gpu_ctx, names, ents)
    slot = pna.HostSlot(gpu_ctx, 4 << 20)
    try:
        for gap in (0, 4096 + 5):                                     # packed at the pipeline's own stride / scattered
            offs, pos = [], 0
            for e in ents:
                offs.append(pos)
                slot.view[pos:pos + len(e)] = e
                pos = ((pos + len(e) + 15) & ~15) + gap
            assert pna.create_archive_from_slot(gpu_ctx, names, slot, offs, [len(e) for e in ents]) == want
        with pytest.raises(pna.PnaGpuError):
            gpu_ctx._check(gpu_ctx._L.pna_gpu_host_free(gpu_ctx._h, ctypes.c_void_p(slot.ptr + 16)))      # not a buffer of host_alloc
    finally:
        slot.free()
    assert pna.create_archive(gpu_ctx, names, ents) == want           # (and the ordinary path is what it was)


def test_max_chunk_size_host_pipeline_with_incompressible_entries_only(gpu_ctx, pna, pf, codec):
    """The bounded host pipeline sizes a sub-batch's device buffer per entry; with max_chunk_size set every further FDAT chunk costs a CRC + a header
    (12 bytes) on top of pna_gpu_bound.  Entries that do not compress at all leave no slack to borrow: two 2 MiB random entries at chunks of 1 000 bytes
    need ~25 KB of chunk framing each (the round-3 advisor's case: PNA_E_DSTSIZE before the term was added to the host path as well)."""
    ents = [codec.corpus_file(2, 900 + i, 2 << 20) for i in range(2)]
    names = [f"rnd/{i}" for i in range(len(ents))]
    payloads = gpu_ctx.compress_batch(ents)
    assert all(len(p) >= len(e) for p, e in zip(payloads, ents))                       # really incompressible: raw blocks
    for mcs in (1000, 4096):
        want = pf.write_archive_header() + b"".join(
            pf.write_normal_entry(pf.file_entry_header(2, nm), pf.flatten_writer([pl], mcs), len(e)) for nm, pl, e in zip(names, payloads, ents)) + pf.finalize_archive()
        assert pna.create_archive_chunked(gpu_ctx, names, ents, mcs) == want
        with gpu_ctx.options(max_chunk_size=(mcs, 0)):
            assert pna.create_archive(gpu_ctx, names, ents) == want


# ---------------------------------------------------------------------------------------------------------
# Device inflate (k_inflate -> k_zoff / k_zexec -> k_iadler): flate2::read::ZlibDecoder behind decompress_reader
def _zlib_streams(codec):
    """(name, raw, zlib stream) made by the system zlib: every block type, long codes, sync flushes, long stored runs."""
    text = codec.corpus_file(0, 21, 1 << 20)
    rnd = codec.corpus_file(2, 21, 200000)
    out = []
    for lvl in (0, 1, 6, 9):
        out.append((f"text-l{lvl}", text, zlib.compress(text, lvl)))
    for name, raw, kw in (("fixed", text[:70000], dict(strategy=zlib.Z_FIXED)), ("huffman-only", text[:70000], dict(strategy=zlib.Z_HUFFMAN_ONLY)),
                          ("rle", bytes([7]) * 300000 + b"xyz" * 50000, {}), ("random", rnd, {}), ("empty", b"", {}), ("one", b"a", {}),
                          ("six-bit", bytes(b & 0x3F for b in rnd[:100000]), dict(level=9)), ("wbits9", text[:100000], dict(wbits=9)),
                          ("png", _raw("raw/images/icon.png"), {}), ("nest", _raw("raw/pna/nest.pna"), {})):
        co = zlib.compressobj(kw.get("level", 6), zlib.DEFLATED, kw.get("wbits", 15), 9, kw.get("strategy", zlib.Z_DEFAULT_STRATEGY))
        out.append((name, raw, co.compress(raw) + co.flush()))
    co = zlib.compressobj(6)
    z = b"".join(co.compress(text[i:i + 50000]) + co.flush(zlib.Z_SYNC_FLUSH) for i in range(0, 400000, 50000)) + co.flush()
    out.append(("sync-flush", text[:400000], z))
    big = codec.corpus_file(2, 22, 3 << 20)
    out.append(("stored-3MiB", big, zlib.compress(big, 0)))                  # literal runs beyond one record: split records
    return out


def test_device_inflate_reads_zlib_streams(gpu_ctx, pna, codec):
    cs = _zlib_streams(codec)
    back = gpu_ctx.decompress_batch([z for _, _, z in cs], [len(r) for _, r, _ in cs], algo=pna.ALGO_DEFLATE)
    for (name, raw, _), b in zip(cs, back):
        assert b == raw, name


def test_device_inflate_round_trips_own_encoder(gpu_ctx, pna, codec):
    cases = _cases(codec)
    names = list(cases)
    outs = gpu_ctx.compress_batch([cases[k] for k in names], algo=pna.ALGO_DEFLATE)
    back = gpu_ctx.decompress_batch(outs, [len(cases[k]) for k in names], algo=pna.ALGO_DEFLATE)
    for k, b in zip(names, back):
        assert b == cases[k], k


def test_device_inflate_reads_reference_fixtures(gpu_ctx, pna, pf):
    """zlib streams written by the reference's own encoder (flate2 / miniz_oxide): the FDAT payloads of deflate.pna."""
    _, items = pf.read_archive(open(os.path.join(GOLDEN, "deflate.pna"), "rb").read())
    items = [it for it in items if getattr(it, "kind", 1) == 0 and it.compression == 1]
    assert items
    raws = [zlib.decompress(it.data) for it in items]
    for it, r in zip(items, raws):
        path = os.path.join(GOLDEN, it.name)
        if os.path.isfile(path):
            assert open(path, "rb").read() == r, it.name
    back = gpu_ctx.decompress_batch([it.data for it in items], [len(r) for r in raws], algo=pna.ALGO_DEFLATE)
    for it, r, b in zip(items, raws, back):
        assert b == r, it.name


def test_device_inflate_rejects_corruption(gpu_ctx, pna, codec):
    d = codec.corpus_file(0, 78, 300000)
    good = zlib.compress(d, 6)
    bad = {
        "adler": good[:-1] + bytes([good[-1] ^ 1]), "truncated": good[:1000], "header check": b"\x78\x9d" + good[2:],
        "preset dictionary": b"\x78\xbb" + good[2:], "method": b"\x79\x9c" + good[2:],
        "stored length": b"\x78\x01\x01\x05\x00\xfa\xfe" + b"hello" + zlib.adler32(b"hello").to_bytes(4, "big"),
        "reserved block type": b"\x78\x9c\x07" + bytes(8),
    }
    for name, z in bad.items():
        with pytest.raises(pna.PnaGpuError):
            gpu_ctx.decompress_batch([z], [len(d) if name != "stored length" else 5], algo=pna.ALGO_DEFLATE)
    with pytest.raises(pna.PnaGpuError):
        gpu_ctx.decompress_batch([good], [len(d) - 1], algo=pna.ALGO_DEFLATE)        # size mismatch
    with pytest.raises(pna.PnaGpuError):
        gpu_ctx.decompress_batch([good], [len(d) + 1], algo=pna.ALGO_DEFLATE)
    flipped = bytearray(good); flipped[len(good) // 2] ^= 0x10
    with pytest.raises(pna.PnaGpuError):
        gpu_ctx.decompress_batch([bytes(flipped)], [len(d)], algo=pna.ALGO_DEFLATE)   # caught by the structure or by Adler-32
    assert gpu_ctx.decompress_batch([good], [len(d)], algo=pna.ALGO_DEFLATE)[0] == d  # the context stays usable


def test_device_inflate_many_small_entries_in_hbm(gpu_ctx, pna):
    """65 536 x 4 KiB (the shape of BASELINE config 5): deflate in HBM, inflate in HBM, compare in HBM."""
    import torch
    n, L = 65536, 4096
    src = torch.empty(n * L + 8192, dtype=torch.uint8, device="cuda")
    gpu_ctx.corpus_fill_device(1, 0, n, L, L, src.data_ptr())
    cap = n * pna.bound(pna.ALGO_DEFLATE, L) + 64
    comp = torch.empty(cap, dtype=torch.uint8, device="cuda")
    offs = gpu_ctx.compress_batch_device(src.data_ptr(), [i * L for i in range(n + 1)], [L] * n, comp.data_ptr(), cap, algo=pna.ALGO_DEFLATE)
    back = torch.zeros(n * L + 64, dtype=torch.uint8, device="cuda")
    gpu_ctx.decompress_batch_device(comp.data_ptr(), offs[:n], [offs[i + 1] - offs[i] for i in range(n)], back.data_ptr(),
                                    [i * L for i in range(n)], [L] * n, algo=pna.ALGO_DEFLATE)
    assert torch.equal(back[:n * L], src[:n * L])


def test_extract_driver_round_trips_archives(gpu_ctx, pna, pf, codec):
    """pna_gpu_extract_archive_host: chunk walk + small-chunk CRCs on the host, FDAT CRC-32 / gather / decode on the device, over
    archives of this library (zstd, deflate, several FDAT chunks per entry) and of the host chunk writer (STORE, directories)."""
    lens = [0, 1, 5, 4095, 70001, 131073, 300000, (1 << 20) + 1, 2500000, 12, 65536]
    ents = [codec.corpus_file(i % 2, 600 + i, n) if n else b"" for i, n in enumerate(lens)]
    names = [f"x{i % 3}/f{i:03d}.txt" for i in range(len(lens))]
    for algo in (pna.ALGO_ZSTD, pna.ALGO_DEFLATE):
        arc = pna.create_archive(gpu_ctx, names, ents, algo=algo)
        got = pna.extract_archive(gpu_ctx, arc)
        assert [(n, k) for n, k, _ in got] == [(n, 0) for n in names] and [d for _, _, d in got] == ents
    # several FDAT chunks per entry (FlattenWriter max_chunk_size), a directory, a stored entry
    class Sink:
        def __init__(self): self.parts = []
        def write(self, b): self.parts.append(b)
    sk = Sink(); ar = pna.Archive(sk)
    pay = gpu_ctx.compress_batch(ents)
    ar.add_dir("x0")
    for nm, pl, e in zip(names, pay, ents):
        ar.add_file(nm, pna.ALGO_ZSTD, len(e), pl, max_chunk_size=1000)
    ar.add_file("stored.bin", pna.ALGO_STORE, 5000, codec.corpus_file(2, 1, 5000))
    ar.finalize()
    arc = b"".join(sk.parts)
    got = pna.extract_archive(gpu_ctx, arc)
    assert got[0] == ("x0", 1, b"") and got[-1] == ("stored.bin", 0, codec.corpus_file(2, 1, 5000))
    assert [d for _, _, d in got[1:-1]] == ents
    # the reference's own archive with fSIZ chunks
    ref = open(os.path.join(GOLDEN, "zstd_with_raw_file_size.pna"), "rb").read()
    items = pf.read_archive(ref)[1]
    got = pna.extract_archive(gpu_ctx, ref)
    assert [n for n, _, _ in got] == [it.name for it in items]
    for (n, _, d), it in zip(got, items):
        assert d == codec.decode_payload(it.compression, it.data, 8 << 20)
    # damage: a flipped payload byte is a CRC mismatch found on the device, a flipped name byte one found on the host
    bad = bytearray(arc); bad[len(arc) // 2] ^= 1
    with pytest.raises(pna.PnaGpuError) as ei:
        pna.extract_archive(gpu_ctx, bytes(bad))
    assert ei.value.code == -2 and "CRC" in str(ei.value)
    bad = bytearray(arc); bad[8 + 20 + 8 + 7] ^= 1
    with pytest.raises(pna.PnaGpuError) as ei:
        pna.extract_archive(gpu_ctx, bytes(bad))
    assert ei.value.code == -2
    # a forged fSIZ (CRC repaired): sizes out of proportion to the data are refused before anything is allocated, plausible wrong
    # ones are caught by the decoder's size check
    import zlib
    hostile = pf.write_archive_header() + pf.write_chunk(b"FHED", pf.file_entry_header(2, "x")) + pf.write_chunk(b"fSIZ", (1 << 62).to_bytes(8, "big")) \
        + pf.write_chunk(b"FDAT", gpu_ctx.compress_batch([b"hello"])[0]) + pf.write_chunk(b"FEND") + pf.finalize_archive()
    with pytest.raises(pna.PnaGpuError) as ei:
        pna.extract_archive(gpu_ctx, hostile)
    assert ei.value.code == -2
    wrong = pf.write_archive_header() + pf.write_chunk(b"FHED", pf.file_entry_header(2, "x")) + pf.write_chunk(b"fSIZ", (7).to_bytes(1, "big")) \
        + pf.write_chunk(b"FDAT", gpu_ctx.compress_batch([b"hello"])[0]) + pf.write_chunk(b"FEND") + pf.finalize_archive()
    with pytest.raises(pna.PnaGpuError) as ei:
        pna.extract_archive(gpu_ctx, wrong)
    assert ei.value.code == -2
    # entries without fSIZ (older writers): sized by the decoder, like a solid stream; deflate without fSIZ is refused
    for name in ("zstd.pna", "zstd_keep_all.pna"):
        ref = open(os.path.join(GOLDEN, name), "rb").read()
        items = pf.read_archive(ref)[1]
        got = pna.extract_archive(gpu_ctx, ref)
        assert [n for n, _, _ in got] == [it.name for it in items]
        for (n, _, d), it in zip(got, items):
            assert d == codec.decode_payload(it.compression, it.data, 8 << 20), n
    for name in ("deflate.pna",):
        ref = open(os.path.join(GOLDEN, name), "rb").read()
        items = pf.read_archive(ref)[1]
        got = pna.extract_archive(gpu_ctx, ref)
        for (n, _, d), it in zip(got, items):
            assert d == codec.decode_payload(it.compression, it.data, 8 << 20), n


def test_extract_driver_reads_solid_archives(gpu_ctx, pna, pf, codec):
    """Solid entries carry no size: the frames of the SDAT stream are counted, the stream is decoded "open" (every frame but the last
    holds 1 MiB, the last reports its size), the inner records are walked on the host, SDAT and inner FDAT CRCs are checked on the device."""
    lens = [300000, 0, 5, (1 << 20) + 3, 70001, 2500000, 12, 1 << 20]
    ents = [codec.corpus_file(i % 2, 800 + i, n) if n else b"" for i, n in enumerate(lens)]
    names = [f"s/{i}.txt" for i in range(len(lens))]
    arc = pna.create_archive(gpu_ctx, names, ents, solid=True)
    got = pna.extract_archive(gpu_ctx, arc)
    assert [n for n, _, _ in got] == names and [d for _, _, d in got] == ents
    # a stream that ends exactly on a frame boundary, and a tiny one
    for sub in (slice(7, 8), slice(2, 3), slice(1, 2)):
        a2 = pna.create_archive(gpu_ctx, names[sub], ents[sub], solid=True)
        assert [d for _, _, d in pna.extract_archive(gpu_ctx, a2)] == ents[sub]
    # the reference's own solid archive: ONE zstd frame written by libzstd, inner entries stored
    ref = open(os.path.join(GOLDEN, "solid_zstd.pna"), "rb").read()
    (so,) = pf.read_archive(ref)[1]
    inner = pf.read_solid_inner(codec.decode_payload(so.compression, so.data, 16 << 20))
    got = pna.extract_archive(gpu_ctx, ref)
    assert [(n, d) for n, _, d in got] == [(e.name, e.data) for e in inner] and len(got) == 9
    # damage inside an SDAT body: found by the device CRC
    bad = bytearray(arc); bad[len(arc) // 2] ^= 1
    with pytest.raises(pna.PnaGpuError) as ei:
        pna.extract_archive(gpu_ctx, bytes(bad))
    assert ei.value.code == -2 and "CRC" in str(ei.value)
    # deflate solid streams: one zlib stream, sized by the inflate kernels (the reference's fixture and this library's)
    ref = open(os.path.join(GOLDEN, "solid_deflate.pna"), "rb").read()
    (so,) = pf.read_archive(ref)[1]
    inner = pf.read_solid_inner(codec.decode_payload(so.compression, so.data, 16 << 20))
    assert [(n, d) for n, _, d in pna.extract_archive(gpu_ctx, ref)] == [(e.name, e.data) for e in inner]
    arc_d = pna.create_archive(gpu_ctx, names, ents, algo=pna.ALGO_DEFLATE, solid=True)
    assert [d for _, _, d in pna.extract_archive(gpu_ctx, arc_d)] == ents


def test_multipart_create_split_join_extract(gpu_ctx, pna, pf, codec):
    """`pna create --split`: the device-assembled archive image re-framed into parts (pna_split_archive == the oracle's SplitParts),
    then read back: parts joined (pna_join_parts) and extracted on the device; the reference's multipart fixture through the same path."""
    ents = [codec.corpus_file(0, 950 + i, n) for i, n in enumerate([300000, 5, 0, 70001, (1 << 20) + 9])]
    names = [f"mp/{i}.txt" for i in range(len(ents))]
    arc = pna.create_archive(gpu_ctx, names, ents)
    for size in (4096, 100000, 300000):
        parts = pna.split_archive(arc, size)
        assert parts == pf.split_parts(pf.archive_body_chunks(arc), size) and len(parts) > 1 and all(len(p) <= size for p in parts)
        got = pna.extract_archive(gpu_ctx, pna.join_parts(parts))
        assert [n for n, _, _ in got] == names and [d for _, _, d in got] == ents
    with pytest.raises(pna.PnaGpuError) as ei:                  # a single part of a multipart archive is not a whole archive
        pna.extract_archive(gpu_ctx, parts[0])
    assert ei.value.code == -7
    ref = pna.join_parts([open(os.path.join(GOLDEN, f"multipart.part{k}.pna"), "rb").read() for k in (1, 2)])
    ((name, kind, data),) = pna.extract_archive(gpu_ctx, ref)
    (it,) = pf.read_archive(ref)[1]
    assert name == it.name and data == codec.decode_payload(it.compression, it.data, 1 << 20)


def test_device_decoder_reads_libzstd_frames_of_many_levels(gpu_ctx, pna, codec):
    """Frames produced by the host's libzstd (the reference's codec, any version present) at levels 1..19 and on several kinds of data:
    single frames with content size, windows up to 8 MiB, repeat offsets, RLE / raw blocks, long matches -- beyond what the golden
    archives happen to contain.  Skipped when the box has no libzstd."""
    if codec.system_libzstd() is None:
        pytest.skip("no system libzstd on this host")
    datas = [codec.corpus_file(0, 40, 700000), codec.corpus_file(1, 41, 300000), bytes(200000), codec.corpus_file(2, 42, 150000),
             (b"abcdefghij" * 30000)[:250007], codec.corpus_file(0, 43, 3 << 20), b"x", b"",
             codec.corpus_file(0, 44, 100000) * 9]                               # long-range repeats across a > 1 MiB distance
    for level in (1, 2, 3, 5, 7, 9, 12, 15, 19):
        comp = [codec.libzstd_compress(d, level) for d in datas]
        back = gpu_ctx.decompress_batch(comp, [len(d) for d in datas])
        for i, (b, d) in enumerate(zip(back, datas)):
            assert b == d, (level, i)


def test_levels_select_the_parse(gpu_ctx, pna, codec):
    """The reference's level scale (lib/src/compress/zstandard.rs:43-57, deflate.rs:89-101) maps onto parameter sets -- fast (greedy,
    LDS-window look-back, every position in the table), balanced (deflate only: + even-position table, backward adoption), default
    (+ 1 MiB look-back, lazy deferral over three positions; zstd: the match finder's 32 KiB-window geometry with the packed table of 49 062 slots, a third
    adoption round), high (zstd 4 .. 9: 16 KiB window, 55 206 slots, a fourth adoption round over eight positions and 15 back bytes) and, zstd only, max (+ the hash table in global memory, 2^19 slots) --, each bit-exact
    with the model; stronger sets compress better."""
    data = [codec.corpus_file(0, 77, 400000), codec.corpus_file(1, 78, 70000), b"", codec.corpus_file(0, 79, (1 << 20) + 5)]
    std = codec.F_HUF | codec.F_FSE | codec.F_FAR | codec.F_ADOPT | codec.F_INS2
    fast, balanced, dflt = codec.F_HUF | codec.F_FSE | codec.F_LAZY, std, std | codec.F_LAZY
    strong = dflt | codec.F_STRONG
    sizes = {}
    for level, fl, gtab, slots in ((-5, fast, 0, 24512), (1, fast, 0, 24512), (2, dflt, 0, 49062), (0, strong, 0, 49062), (3, strong, 0, 49062), (pna.LEVEL_DEFAULT, strong, 0, 49062),
                                   (4, strong, 0, 55206), (5, strong, 0, 55206), (6, strong, 0, 55206), (9, strong, 0, 55206), (10, strong, 1, 19), (19, strong, 1, 19), (22, strong, 1, 19), (99, strong, 1, 19)):
        outs = gpu_ctx.compress_batch(data, algo=pna.ALGO_ZSTD, level=level)
        assert codec.product_level_flags(level) == (fl, bool(gtab)), level
        pz = codec.params_for_level(level)
        high = level != pna.LEVEL_DEFAULT and level >= 4                  # zstd 4 .. 22: a fourth adoption round over eight positions, 15 back bytes (FLAG_STRONG2)
        assert pz.hash_log == slots and pz.rounds == (0 if fl == fast else (0x2148 if high else 0x214) if fl == strong else 0x21) and pz.back_cap == (0 if fl == fast else 15 if high else 7 if fl == strong else 3), level
        assert outs == [codec.model_compress(d, pz) for d in data], level
        sizes[level] = sum(map(len, outs))
    assert sizes[19] < sizes[6] == sizes[4] < sizes[3] < sizes[2] < sizes[1] and sizes[0] == sizes[3] == sizes[pna.LEVEL_DEFAULT]
    dstd = codec.F_ADOPT | codec.F_INS2
    # deflate level 0 is Compression::none() (lib/src/compress/deflate.rs:89-101): stored blocks only, header 78 01 -- not the fast set
    outs0 = gpu_ctx.compress_batch(data, algo=pna.ALGO_DEFLATE, level=0)
    assert outs0 == [codec.deflate_model_compress(d, codec.params_for_level(0, deflate=True)) for d in data]
    assert all(codec.zlib_decompress(o) == d for o, d in zip(outs0, data)) and all(o[:2] == b"\x78\x01" for o in outs0)
    assert all(len(o) > len(d) for o, d in zip(outs0, data)) and len(outs0[2]) == 11
    for level, fl in ((1, codec.F_LAZY), (3, codec.F_LAZY), (4, dstd | codec.F_LAZY), (5, dstd | codec.F_LAZY), (6, dstd | codec.F_LAZY), (pna.LEVEL_DEFAULT, dstd | codec.F_LAZY), (8, dstd | codec.F_LAZY), (9, dstd | codec.F_LAZY | codec.F_STRONG)):
        outs = gpu_ctx.compress_batch(data, algo=pna.ALGO_DEFLATE, level=level)
        pd = codec.params_for_flags(fl, deflate=True)
        assert outs == [codec.deflate_model_compress(d, pd) for d in data], level
        assert all(codec.zlib_decompress(o) == d for o, d in zip(outs, data))
        sizes[("d", level)] = sum(map(len, outs))
    assert sizes[("d", 9)] < sizes[("d", 6)] == sizes[("d", 4)] < sizes[("d", 1)]


def test_extract_driver_windows(gpu_ctx, pna, pf, codec):
    """The driver walks the archive in windows of bounded size (PNA_EXTRACT_WIN_MIB; 4 GiB by default): with 1 MiB windows every large
    entry is a window of its own and small ones share one -- same entries, same order, solid entries in between included."""
    ents = [codec.corpus_file(i % 2, 1000 + i, n) for i, n in enumerate([300000, 5, 0, 2500000, 70001, (1 << 20) + 9, 12, 65536, 900000, 3])]
    names = [f"w/{i:02d}.txt" for i in range(len(ents))]
    arc = pna.create_archive(gpu_ctx, names, ents)
    solid = pna.create_archive(gpu_ctx, ["s/a", "s/b"], [ents[0], ents[4]], solid=True)
    # splice the solid entry between the 4th and 5th normal entries: [head | e0..e3 | SHED..SEND | e4.. | AEND]
    chunks = pf.archive_body_chunks(arc); so_chunks = pf.archive_body_chunks(solid)
    cut = [i for i, (t, _) in enumerate(chunks) if t == b"FEND"][3] + 1
    mixed = pf.write_archive_header() + b"".join(pf.write_chunk(t, d) for t, d in chunks[:cut] + so_chunks + chunks[cut:]) + pf.finalize_archive()
    want = [(n, d) for n, d in zip(names[:4], ents[:4])] + [("s/a", ents[0]), ("s/b", ents[4])] + [(n, d) for n, d in zip(names[4:], ents[4:])]
    for win in (None, "1", "3"):
        with gpu_ctx.options(extract_win_mib=(int(win) if win else 1024, 1024)):
            got = pna.extract_archive(gpu_ctx, mixed)
        assert [(n, d) for n, _, d in got] == want, win


def test_archive_with_metadata_chunks(gpu_ctx, pna, pf, codec):
    """Per-entry metadata (what --keep-timestamp / --keep-permission / --keep-xattr add: try_for_each_metadata_facet, lib/src/entry.rs:124-180)
    and user-defined extra chunks go through the device path as blobs of framed chunks; wire order FHED, extra*, fSIZ, facets*, FDAT, FEND
    (lib/src/entry.rs:895-911).  Byte-exact against the oracle's writer; the extract driver skips the ancillary chunks."""
    import struct
    ents = [codec.corpus_file(0, 1100 + i, n) for i, n in enumerate([300000, 5, 0, 70001, 9000])]
    names = [f"meta/{i}.txt" for i in range(len(ents))]
    fac, ext = [], []
    for i in range(len(ents)):
        f = [(b"cTIM", struct.pack(">Q", 1700000000 + i)), (b"mTIM", struct.pack(">Q", 1700000100 + i)), (b"fPRM", b"\x00\x00\x03\xe8\x04user\x00\x00\x03\xe8\x05group\x01\xa4")]
        fac.append(f if i != 2 else [])                               # one entry without facets
        ext.append([(b"abCd", bytes([i, 7, 7]))] if i % 2 else [])    # a private ancillary chunk on every other entry
    blob = lambda chunks: b"".join(pf.write_chunk(t, d) for t, d in chunks)
    arc = pna.create_archive_with_metadata(gpu_ctx, names, ents, facets=[blob(f) for f in fac], extra=[blob(x) for x in ext])
    payloads = gpu_ctx.compress_batch(ents)
    want = pf.write_archive_header() + b"".join(
        pf.write_normal_entry(pf.file_entry_header(2, nm), [pl], len(e), extra=x, facets=f) for nm, pl, e, x, f in zip(names, payloads, ents, ext, fac)
    ) + pf.finalize_archive()
    assert arc == want
    got = pna.extract_archive(gpu_ctx, arc)
    assert [n for n, _, _ in got] == names and [d for _, _, d in got] == ents
    # with the cipher stage: PHSF and the data chunks come behind the facets
    key, phsf = pna.kdf_pbkdf2_sha256(b"password", bytes(range(16)), 1000)
    ivs = os.urandom(16 * len(ents))
    a2 = pna.create_archive_with_metadata(gpu_ctx, names, ents, facets=[blob(f) for f in fac], cipher=pna.Cipher(key, phsf, pna.MODE_CTR, ivs=ivs))
    _, items = pf.read_archive(a2)
    assert [[t for t, _ in it.chunks] for it in items][0] == [b"FHED", b"fSIZ", b"cTIM", b"mTIM", b"fPRM", b"PHSF", b"FDAT", b"FDAT", b"FEND"]
    assert [d for _, _, d in pna.extract_archive(gpu_ctx, a2, b"password")] == ents
    # malformed blobs are refused: a broken CRC, a chunk type the library writes itself
    bad = bytearray(blob(fac[0])); bad[-1] ^= 1
    for b in (bytes(bad), pf.write_chunk(b"FDAT", b"x")):
        with pytest.raises(pna.PnaGpuError) as ei:
            pna.create_archive_with_metadata(gpu_ctx, names, ents, facets=[b] * len(ents))
        assert ei.value.code == -2


def test_extract_driver_hands_out_sanitised_names(gpu_ctx, pna, pf, codec):
    """The read side exposes EntryHeader::path() (lib/src/entry/header.rs:91-94,143-147): names from an untrusted archive are normalised
    and stripped of root / '.' / '..' before the callback sees them; FHED bytes that are not UTF-8, or carry a NUL, are rejected."""
    raw_names = ["../../etc/passwd", "/abs/file", "a/../b.txt", "ok/./name", "..", "x//y"]
    body = b"".join(pf.write_normal_entry(pf.file_entry_header(0, nm), [b"data-%d" % i], 6) for i, nm in enumerate(raw_names))
    arc = pf.write_archive_header() + body + pf.finalize_archive()
    got = pna.extract_archive(gpu_ctx, arc)
    assert [n for n, _, _ in got] == [pf.sanitize_name(n) for n in raw_names] == ["etc/passwd", "abs/file", "b.txt", "ok/name", "", "x/y"]
    assert [d for _, _, d in got] == [b"data-%d" % i for i in range(len(raw_names))]
    for bad in (b"bad\xff\xfename", b"nul\x00name", b"\xc0\xafoverlong", b"\xed\xa0\x80surrogate"):
        hdr = bytes([0, 0, 0, 0, 0, 1]) + bad
        arc2 = pf.write_archive_header() + pf.write_normal_entry(hdr, [b"x"], 1) + pf.finalize_archive()
        with pytest.raises(pna.PnaGpuError) as ei:
            pna.extract_archive(gpu_ctx, arc2)
        assert ei.value.code == -2, bad


def test_write_file_stream_entry(gpu_ctx, pna, pf, codec):
    """Archive::write_file / write_stream_entry (lib/src/archive/write.rs:276-299,730-777): FHED, extra + metadata chunks, one FDAT per
    encoder burst (<= 32 KiB; lib/src/chunk/write.rs:32-47), FEND -- and NO fSIZ (write.rs:830-881).  Byte-exact against the oracle's
    restatement fed with the oracle model's stream; read back by the fixture-pinned reader and by the device extract driver."""
    data = codec.corpus_file(0, 77, 300000)
    extra = pf.write_chunk(b"exTr", b"extra")                       # a private ancillary chunk, as in the reference's test
    fltp = pf.write_chunk(b"fLTP", b"\x01")
    for algo, comp, model in ((pna.ALGO_ZSTD, 2, lambda d: codec.model_compress(d, _params(codec))), (pna.ALGO_DEFLATE, 1, codec.deflate_model_compress)):
        for writes, mcs in (([data], 0), ([data[:1000], data[1000:200000], data[200000:]], 0), ([data], 5000), ([b""], 0), ([b"text"], 0)):
            out = bytearray()
            pna.write_file(gpu_ctx, out.extend, "dir/../text.txt", writes, algo=algo, meta=extra + fltp, max_chunk_size=mcs)
            whole = b"".join(writes)
            stream = model(whole)
            bursts = [stream[i:i + 32768] for i in range(0, len(stream), 32768)]
            want = pf.write_stream_entry(pf.file_entry_header(comp, "text.txt"), bursts, extra=[(b"exTr", b"extra")], facets=[(b"fLTP", b"\x01")],
                                         max_chunk_size=mcs or None)
            assert bytes(out) == want, (algo, len(writes), mcs)
            types = [t for t, _, _ in pf.read_chunks(bytes(out))]
            assert types[:3] == [b"FHED", b"exTr", b"fLTP"] and b"fSIZ" not in types and types[-1] == b"FEND"
            arc = pf.write_archive_header() + bytes(out) + pf.finalize_archive()
            (it,) = pf.read_archive(arc)[1]
            assert it.raw_file_size is None and it.name == "text.txt" and codec.decode_payload(comp, it.data, len(whole) + 64) == whole
            assert pna.extract_archive(gpu_ctx, arc) == [("text.txt", 0, whole)]      # entries without fSIZ are sized by the decoder


def test_append_equals_create(gpu_ctx, pna, pf, codec):
    """`pna append` (cli/src/command/append.rs:504-560): seek to AEND, add entries, finalize.  Appending k entries to an archive of m gives
    the very bytes `pna create` writes for all m + k (per-entry streams and framing are position-independent); multipart tails refuse."""
    ents = [codec.corpus_file(i % 2, 900 + i, n) for i, n in enumerate([300000, 0, 70001, (1 << 20) + 5, 12])]
    names = [f"ap/{i}.txt" for i in range(len(ents))]
    for algo in (pna.ALGO_ZSTD, pna.ALGO_DEFLATE):
        whole = pna.create_archive(gpu_ctx, names, ents, algo=algo)
        for m in (0, 2, 5):
            base = pna.create_archive(gpu_ctx, names[:m], ents[:m], algo=algo)
            got = pna.append_archive(gpu_ctx, base, names[m:], ents[m:], algo=algo)
            assert got == whole, (algo, m)
        assert [(it.name, codec.decode_payload(it.compression, it.data, len(e) + 64)) for it, e in zip(pf.read_archive(whole)[1], ents)] == list(zip(names, ents))
    with pytest.raises(pna.PnaGpuError):
        pna.append_archive(gpu_ctx, open(os.path.join(GOLDEN, "multipart.part1.pna"), "rb").read(), ["x"], [b"y"])
    with pytest.raises(pna.PnaGpuError):
        pna.append_archive(gpu_ctx, whole[:-5], ["x"], [b"y"])


def test_update_composed_from_listing_and_parts(gpu_ctx, pna, pf, codec):
    """`pna update` (cli/src/command/update.rs:611-665): walk the old archive's entries -- an entry whose file did not change is copied as it stands, one
    whose file is newer is (with --sync) dropped or (without: bsdtar's append-only -u) kept --, then the changed and the new files are compressed and
    added behind them in argument order.  Composed here from the library's pieces, as a host would: pna_archive_list_entries for the records'
    places, the kept records byte for byte, pna_gpu_create_archive_part_host (no head, no tail) for the compressed ones, AEND -- against the oracle's
    writer fed with the model's streams, for both codecs and both --sync settings; the result reads back through the oracle reader and the extract
    driver (later record of a name wins on extraction)."""
    old_ents = [codec.corpus_file(i % 2, 9100 + i, n) for i, n in enumerate([300000, 0, 70001, (1 << 20) + 5, 12, 4096])]
    old_names = [f"up/{i}.txt" for i in range(len(old_ents))]
    changed = {1: codec.corpus_file(0, 9201, 50000), 3: codec.corpus_file(1, 9203, 2 << 20)}        # newer on disk than in the archive
    added = [("up/new-a.txt", codec.corpus_file(0, 9300, 123457)), ("up/new-b.txt", b"")]
    for algo in (pna.ALGO_ZSTD, pna.ALGO_DEFLATE):
        base = pna.create_archive(gpu_ctx, old_names, old_ents, algo=algo)
        recs = pna.list_entries(base)
        assert [r[0].decode() for r in recs] == old_names and all(r[1] == 0 for r in recs)
        assert recs[0][2] == len(pf.write_archive_header()) and recs[-1][2] + recs[-1][3] == pna.seek_to_end(base)[0]
        new_names = [old_names[i] for i in sorted(changed)] + [n for n, _ in added]
        new_ents = [changed[i] for i in sorted(changed)] + [d for _, d in added]
        part = pna.create_archive_chunked(gpu_ctx, new_names, new_ents, 0, algo=algo, part=0)            # the records alone: neither header nor AEND
        model = (lambda d: codec.model_compress(d, codec.params_for_level(3))) if algo == pna.ALGO_ZSTD else (lambda d: codec.deflate_model_compress(d))
        want_part = b"".join(pf.write_normal_entry(pf.file_entry_header(2 if algo == pna.ALGO_ZSTD else 1, nm), [model(d)], len(d)) for nm, d in zip(new_names, new_ents))
        assert part == want_part
        for sync in (False, True):
            kept = [base[o:o + ln] for k, (_, _, o, ln) in enumerate(recs) if not (sync and k in changed)]
            got = pf.write_archive_header() + b"".join(kept) + part + pf.finalize_archive()
            _, items = pf.read_archive(got)
            names_out = [it.name for it in items]
            assert names_out == [n for k, n in enumerate(old_names) if not (sync and k in changed)] + new_names
            latest = {}
            for n, _, d in pna.extract_archive(gpu_ctx, got):
                latest[n] = d                                                                            # later wins
            want_latest = dict(zip(old_names, old_ents)); want_latest.update({old_names[i]: d for i, d in changed.items()}); want_latest.update(dict(added))
            assert latest == want_latest, (algo, sync)


def test_device_inflate_lane_per_piece_paths(gpu_ctx, pna, codec):
    """The lane-per-piece inflate (k_imark / k_vinflate / k_vfin) and its hand-over to the wave-per-stream walk: a batch large enough for
    the lane path (>= 1 024 pieces) that mixes this library's sync-flushed streams, small foreign zlib streams (one piece each: fixed,
    dynamic, stored, multi-block), LARGE foreign streams (no sync markers: handed over), a stream with a chance marker pattern in a
    stored block (marker count does not fit: handed over) and zlib's own Z_SYNC_FLUSH pieces of another size (sizes do not fit: handed
    over).  PNA_INFLATE_SERIAL=1 must give the same bytes."""
    import random
    rnd = random.Random(11)
    own_raw = [codec.corpus_file(i % 2, 4000 + i, n) for i, n in enumerate([1 << 20, (1 << 20) + 77, 300000, 131072, 131073, 5000, 0, 1] + [200000] * 120)]
    own = gpu_ctx.compress_batch(own_raw, algo=pna.ALGO_DEFLATE)
    small_raw = [codec.corpus_file(1, 5000 + i, 100 + 997 * (i % 120)) for i in range(800)]
    small = [zlib.compress(r, [0, 1, 6, 9][i % 4]) for i, r in enumerate(small_raw)]
    co = zlib.compressobj(6, zlib.DEFLATED, 15, 9, zlib.Z_FIXED); small_raw.append(small_raw[5]); small.append(co.compress(small_raw[5]) + co.flush())
    big_raw = [codec.corpus_file(0, 6000 + i, 700000 + i) for i in range(3)]
    big = [zlib.compress(r, 6) for r in big_raw]
    tricky_raw = bytes(rnd.getrandbits(8) for _ in range(150000)) + b"\x00\x00\xff\xff" * 5 + bytes(rnd.getrandbits(8) for _ in range(150000))
    tricky = zlib.compress(tricky_raw, 0)                                   # stored blocks: the pattern appears verbatim in the stream
    co = zlib.compressobj(6)
    sf_raw = codec.corpus_file(0, 6100, 400000)
    sf = b"".join(co.compress(sf_raw[i:i + 50000]) + co.flush(zlib.Z_SYNC_FLUSH) for i in range(0, 400000, 50000)) + co.flush()
    raws = own_raw + small_raw + big_raw + [tricky_raw, sf_raw]
    comps = list(own) + small + big + [tricky, sf]
    assert sum(max(1, (len(r) + 131071) // 131072) for r in raws) >= 1024
    got = gpu_ctx.decompress_batch(comps, [len(r) for r in raws], algo=pna.ALGO_DEFLATE)
    assert got == raws
    with gpu_ctx.options(inflate_serial=(1, 0)):
        assert gpu_ctx.decompress_batch(comps, [len(r) for r in raws], algo=pna.ALGO_DEFLATE) == raws
    # corrupt input in a lane batch is refused all the same (after the hand-over): a flipped bit, a wrong size, a bad Adler-32
    for k, mut in ((3, lambda z: z[:100] + bytes([z[100] ^ 4]) + z[101:]), (200, lambda z: z[:-1] + bytes([z[-1] ^ 1]))):
        bad = list(comps); bad[k] = mut(bad[k])
        with pytest.raises(pna.PnaGpuError):
            gpu_ctx.decompress_batch(bad, [len(r) for r in raws], algo=pna.ALGO_DEFLATE)
    with pytest.raises(pna.PnaGpuError):
        gpu_ctx.decompress_batch(comps, [len(r) for r in raws[:-1]] + [len(raws[-1]) - 1], algo=pna.ALGO_DEFLATE)


def test_deflate_solid_stream_decodes_in_pieces(gpu_ctx, pna, pf, codec):
    """A deflate `--solid` archive is ONE zlib stream of unknown size: its sync-flush markers are counted, the pieces decoded lane-parallel
    (open size: the last piece reports its length), the inner records walked -- round 1 decoded such a stream on one wave."""
    n, L = 160, 1 << 20
    ents = [codec.corpus_file(0, 8000 + i, L) for i in range(n)]
    names = [f"sd/{i:03d}.txt" for i in range(n)]
    arc = pna.create_archive(gpu_ctx, names, ents, algo=pna.ALGO_DEFLATE, solid=True)
    got = pna.extract_archive(gpu_ctx, arc)
    assert [nm for nm, _, _ in got] == names and all(d == e for (_, _, d), e in zip(got, ents))
    # the same stream through the oracle's reader and stdlib zlib
    (so,) = pf.read_archive(arc)[1]
    inner = pf.read_solid_inner(zlib.decompress(so.data))
    assert [(e.name, e.data) for e in inner[:3]] == list(zip(names[:3], ents[:3])) and len(inner) == n


def test_far_candidates_and_adoption_edge_cases(gpu_ctx, pna, codec):
    """Inputs built to stress round 2's LZ rules: long repeats at distances on both sides of the LDS window limit (56 064) and up to the
    segment size (far candidates, their 16 + 16 byte steps, the wave-cooperative extension reading the segment from HBM), repeats that start
    at odd positions and one or two bytes after a table hit (backward adoption, also across the 64-position group border where it must
    stop), candidates at positions 0..3 (unusable by rule), repeats that run into block and segment ends.  Bit-exact with the model,
    decodable by libzstd / zlib, for both codecs and every level set."""
    import random
    rnd = random.Random(2024)

    def rb(n):
        return bytes(rnd.getrandbits(8) for _ in range(n))
    cases = {}
    chunk = rb(5000)
    # the same 5 000 bytes at growing distances, at odd and even alignments, with random filler in between
    buf = bytearray()
    for d in (100, 7000, 33000, 56000, 56064, 56065, 56100, 60001, 131072, 262145, 500003):
        buf += chunk[:1 + rnd.randrange(3000, 5000)]
        buf += rb(d % 9973 + 17)
        while len(buf) % 2 != (d & 1):
            buf += b"z"
    cases["repeats"] = bytes(buf)
    text = codec.corpus_file(0, 4242, 1 << 20)
    cases["text+far-copy"] = text[:300000] + rb(70000) + text[1000:250000] + rb(1000) + text[123:200123]
    cases["start-of-segment"] = (text[:40] + rb(200) + text[:40] + rb(60000) + text[:3] + text[1:40] + rb(2000)) * 3
    cases["block-edge"] = rb(131072 - 50) + text[:100] + rb(70000) + text[:100] + rb(131072 - 70000 - 150) + text[:100]
    cases["segment-edge"] = rb((1 << 20) - 30) + text[:60] + text[:60] + rb(5000)
    cases["group-border"] = b"".join(text[i * 61:i * 61 + 61] + bytes([i & 255]) + text[i * 61 + 1:i * 61 + 62] for i in range(3000))
    cases["long-far-run"] = rb(100000) + bytes(200000) + rb(60000) + bytes(200000)
    names = sorted(cases)
    data = [cases[k] for k in names]
    for level in (1, 2, 3, 7, 19):
        outs = gpu_ctx.compress_batch(data, level=level)
        pz = codec.params_for_level(level)
        for k, d, o in zip(names, data, outs):
            assert o == codec.model_compress(d, pz), (k, level)
            assert codec.zstd_decompress(o, len(d)) == d, (k, level)
            if codec.system_libzstd() is not None:
                assert codec.libzstd_decompress_stream(o, len(d)) == d, (k, level)
    assert gpu_ctx.decompress_batch(outs, [len(d) for d in data]) == data
    for level in (1, 4, 6, 9):
        outs = gpu_ctx.compress_batch(data, algo=pna.ALGO_DEFLATE, level=level)
        pd = codec.params_for_level(level, deflate=True)
        for k, d, o in zip(names, data, outs):
            assert o == codec.deflate_model_compress(d, pd), (k, level)
            assert zlib.decompress(o) == d, (k, level)


def test_one_process_several_contexts(gpu_ctx, pna, pf, codec):
    """pna_gpu_create_archive_multi_host: one process, one context per GPU (here: several contexts on the one GPU), contiguous index
    ranges balanced by bytes, parts in index order == the archive of a single context, byte for byte."""
    ents = [codec.corpus_file(i % 2, 1200 + i, n) for i, n in enumerate([300000, 0, 5, (1 << 20) + 3, 70001, 2500000, 12, 1 << 20, 4096, 999999, 1, 65536])]
    names = [f"mc/{i:02d}.txt" for i in range(len(ents))]
    want = pna.create_archive(gpu_ctx, names, ents)
    extra = [headline_context(pna) for _ in range(3)]
    try:
        for k in (2, 3, 4):
            assert pna.create_archive_multi([gpu_ctx] + extra[:k - 1], names, ents) == want, k
        assert pna.create_archive_multi([gpu_ctx] + extra, names[:2], ents[:2]) == pna.create_archive(gpu_ctx, names[:2], ents[:2])   # more contexts than entries
        assert pna.create_archive_multi(extra[:2], [], []) == pna.create_archive(gpu_ctx, [], [])
        assert pna.create_archive_multi(extra[:2], names, ents, algo=pna.ALGO_DEFLATE) == pna.create_archive(gpu_ctx, names, ents, algo=pna.ALGO_DEFLATE)
    finally:
        for c in extra:
            c.close()


def test_decoder_reads_what_the_reference_decoder_reads(gpu_ctx, pna, pf, codec):
    """decompress_reader -> zstd::stream::read::Decoder (lib/src/entry/read.rs:171-190) reads ANY concatenation of frames: frames of any content size, with or
    without Frame_Content_Size, with or without Content_Checksum, skippable frames (magic 0x184D2A5?) between them.  Random concatenations of libzstd frames
    (levels 1 - 19, 1 B - 3 MiB of content) next to entries of this library's own shapes in ONE batch == oracle/zstd_dec.c (and the system libzstd);
    a damaged checksum, a truncated skippable frame and a wrong entry size are refused."""
    import random, struct
    if codec.system_libzstd() is None:
        pytest.skip("system libzstd not available")
    rng = random.Random(20261005)
    def frame(data, level, fcs, chk):
        if fcs and not chk:
            return codec.libzstd_compress(data, level)
        return codec.libzstd_compress_checksum(data, level, extra=(() if fcs else ((200, 0),)) + (() if chk else ((201, 0),)))
    def skippable():
        body = bytes(rng.getrandbits(8) for _ in range(rng.choice((0, 1, 7, 300))))
        return struct.pack("<II", 0x184D2A50 + rng.randrange(16), len(body)) + body
    sizes = [1, 2, 17, 255, 4096, 70000, (1 << 20) - 1, 1 << 20, (1 << 20) + 1, 3 << 20, 150000, 999]
    payloads, raws = [], []
    for e in range(14):
        parts, raw = [], b""
        for k in range(rng.randrange(1, 6)):
            if rng.random() < 0.4:
                parts.append(skippable())
            n = rng.choice(sizes)
            d = codec.corpus_file(rng.randrange(2), 5000 + 16 * e + k, n)
            parts.append(frame(d, rng.choice((1, 3, 5, 9, 12, 19)), e % 3 != 0 and rng.random() < 0.7, rng.random() < 0.5))
            raw += d
        if rng.random() < 0.5:
            parts.append(skippable())
        payloads.append(b"".join(parts)); raws.append(raw)
    # next to them: this library's own entry (1 MiB grid), one libzstd frame per entry (the reference's shape), an empty entry
    own = codec.corpus_file(0, 5990, (2 << 20) + 12345)
    payloads += [gpu_ctx.compress_batch([own])[0], codec.libzstd_compress(own, 3), gpu_ctx.compress_batch([b""])[0]]
    raws += [own, own, b""]
    for p, r in zip(payloads, raws):
        assert codec.zstd_decompress(p, len(r)) == r and codec.libzstd_decompress_stream(p, len(r)) == r       # the checkers agree first
    assert gpu_ctx.decompress_batch(payloads, [len(r) for r in raws]) == raws
    # refusals: a checksum that does not match, a skippable frame cut short, a size that the frames do not add up to
    d = codec.corpus_file(0, 5991, 50000)
    good = skippable() + frame(d, 3, False, True) + frame(d, 5, True, True)
    assert gpu_ctx.decompress_batch([good], [2 * len(d)]) == [d + d]
    bad = bytearray(good); bad[-1] ^= 0x40
    for payload, size in ((bytes(bad), 2 * len(d)), (good + struct.pack("<II", 0x184D2A51, 100) + b"xy", 2 * len(d)), (good, 2 * len(d) - 1), (good, 2 * len(d) + 1)):
        with pytest.raises(pna.PnaGpuError):
            gpu_ctx.decompress_batch([payload], [size])


def test_default_contexts_cut_calls_without_changing_bytes(pna, pf, codec):
    """The library's DEFAULT options (latency mode on, the block size follows the call's input bytes: 16 KiB up to 32 MiB, 32 KiB up to 384 MiB, ...): an
    entry point that cuts its call -- the multi-context create into ranges, the host form of compress_batch into pieces -- gives every part the block size of
    the WHOLE call, so the bytes equal the uncut call's (round-4 advisor finding: each part picked its own).  40 MiB sits between the first two thresholds:
    two ranges of 20 MiB would take 16 KiB blocks where the whole call takes 32 KiB."""
    import torch  # noqa: F401
    ents = [codec.corpus_file(0, 4200 + i, 1 << 20) for i in range(40)]
    names = [f"d/{i:02d}" for i in range(len(ents))]
    ctxs = [pna.Context(0) for _ in range(3)]
    try:
        want = pna.create_archive(ctxs[0], names, ents)
        assert ctxs[0].timing().blk_log == 15
        for k in (2, 3):
            assert pna.create_archive_multi(ctxs[:k], names, ents) == want, k
        small = pna.create_archive(ctxs[0], names[:20], ents[:20])                    # (the premise: a 20 MiB call of its own does take other blocks)
        assert ctxs[0].timing().blk_log == 14 and small[:len(want) // 4] != want[:len(want) // 4]
        # compress_batch from host buffers in pieces of 16 MiB == in one piece
        one = ctxs[0].compress_batch(ents)
        ctxs[1].set_option("batch_piece_mib", 16)
        assert ctxs[1].compress_batch(ents) == one
    finally:
        for c in ctxs:
            c.close()


def test_ordered_gather_over_rccl_single_rank(gpu_ctx, pna, pf, codec):
    """pna_gpu_gather_ordered on a communicator of ONE rank (RCCL initialises on a single device; the N-GPU run is the driver's): the all-gather of
    the sizes and the root's own copy run for real, the archive part arrives unchanged and reads back."""
    import torch
    ents = [codec.corpus_file(0, 3100 + i, 200000 + 1000 * i) for i in range(6)]
    names = [f"g/{i}" for i in range(len(ents))]
    arc = pna.create_archive(gpu_ctx, names, ents)
    local = torch.frombuffer(bytearray(arc), dtype=torch.uint8).cuda()
    out = torch.zeros(len(arc) + 64, dtype=torch.uint8, device="cuda")
    comm = pna.Comm(0, pna.Comm.unique_id(), 1, 0)
    try:
        sizes, total = comm.gather_ordered(local.data_ptr(), len(arc), out.data_ptr(), out.numel())
        assert sizes == [len(arc)] and total == len(arc)
        assert out[:total].cpu().numpy().tobytes() == arc and int(out[total:].sum()) == 0
        assert [(n, d) for n, _, d in pna.extract_archive(gpu_ctx, out[:total].cpu().numpy().tobytes())] == list(zip(names, ents))
        with pytest.raises(pna.PnaGpuError) as ei:
            comm.gather_ordered(local.data_ptr(), len(arc), out.data_ptr(), 100)          # destination too small: the collective verdict, nothing sent
        assert ei.value.code == pna.E_DSTSIZE
        assert comm.gather_ordered(0, 0, out.data_ptr(), out.numel()) == ([0], 0)          # an empty part; the communicator is still in step
        # the posted form: two gathers in flight on the communicator's stream, each behind the stream that produced its part; tickets say which is done
        side = torch.cuda.Stream()
        out2 = torch.zeros_like(out)
        with torch.cuda.stream(side):
            local2 = local.flip(0).contiguous()                                               # (produced on `side`: the gather must wait for it)
        t0 = comm.ticket()
        assert comm.gather_ordered_start(local.data_ptr(), len(arc), out.data_ptr(), out.numel()) == ([len(arc)], len(arc))
        assert comm.gather_ordered_start(local2.data_ptr(), len(arc), out2.data_ptr(), out2.numel(), stream=side.cuda_stream) == ([len(arc)], len(arc))
        assert comm.ticket() == t0 + 2
        comm.gather_wait(t0 + 1)
        assert out[:total].cpu().numpy().tobytes() == arc
        comm.gather_wait()
        assert out2[:total].cpu().numpy().tobytes() == arc[::-1]
    finally:
        comm.close()


def test_zstd_content_checksum_is_verified(gpu_ctx, pna, codec):
    """Frames with a Content_Checksum (RFC 8878 3.1.1; the reference's own writer sets none, other zstd writers may): the device decoder checks the
    XXH64 of what it decoded, as zstd::stream::read::Decoder does behind decompress_reader (lib/src/entry/read.rs:171-190) -- good frames decode,
    a frame whose stored checksum is off by a bit is refused, whichever decode path takes it (lane-parallel; one workgroup per frame)."""
    if codec.system_libzstd() is None:
        pytest.skip("system libzstd (the writer of the test frames) is absent")
    raws = [codec.corpus_file(0, 8100, 300000), b"", b"abc", codec.corpus_file(1, 8101, 31), codec.corpus_file(2, 8102, 70001), codec.corpus_file(0, 8103, (1 << 20) + 33),
            bytes(100000), codec.corpus_file(0, 8104, 32), codec.corpus_file(0, 8105, 4 << 20)]
    comps = [codec.libzstd_compress_checksum(r, 3 + (i % 3)) for i, r in enumerate(raws)]
    assert all((c[4] >> 2) & 1 for c in comps)                                   # the frames do carry the flag
    lens = [len(r) for r in raws]
    assert gpu_ctx.decompress_batch(comps, lens) == raws
    with gpu_ctx.options(zdec_serial=(1, 0)):
        assert gpu_ctx.decompress_batch(comps, lens) == raws
    for k in (0, 3, 5, 8):
        bad = list(comps); bad[k] = bad[k][:-1] + bytes([bad[k][-1] ^ 0x10])
        with pytest.raises(pna.PnaGpuError):
            gpu_ctx.decompress_batch(bad, lens)
        with gpu_ctx.options(zdec_serial=(1, 0)):
            with pytest.raises(pna.PnaGpuError):
                gpu_ctx.decompress_batch(bad, lens)


def test_zstd_frames_with_offsets_beyond_16_mib(gpu_ctx, pna, codec):
    """A foreign frame whose matches reach further back than 16 MiB (libzstd with a 64 MiB window and long-distance matching; the reference's
    `--zstd 20..22` on large entries: lib/src/compress/zstandard.rs:43-57 passes the level through, ultra levels take windows of 32 - 128 MiB):
    the decoder's records hold offsets of 28 bits.  Both decode paths; the frame is checked to hold such an offset by decoding it with a
    window of 16 MiB in the model decoder's terms: the second copy of the first 2 MiB lies 40 MiB behind the first."""
    if codec.system_libzstd() is None:
        pytest.skip("system libzstd (the writer of the test frame) is absent")
    import numpy as np
    rng = np.random.default_rng(77)
    head = rng.integers(0, 256, size=40 << 20, dtype=np.uint8).tobytes()
    raw = head + head[:2 << 20] + codec.corpus_file(0, 8200, 100000)
    comp = codec.libzstd_compress_checksum(raw, 3, extra=((101, 26), (160, 1)))
    assert len(comp) < len(head) + (1 << 20)                                     # the repeat was found: it costs a few hundred bytes, not 2 MiB
    assert codec.libzstd_decompress_stream(comp, len(raw)) == raw
    assert gpu_ctx.decompress_batch([comp], [len(raw)]) == [raw]
    with gpu_ctx.options(zdec_serial=(1, 0)):
        assert gpu_ctx.decompress_batch([comp], [len(raw)]) == [raw]



def _libzstd_one_frame(codec, raw, level=3):
    import numpy as np
    Z = codec.system_libzstd()
    host = np.frombuffer(raw, dtype=np.uint8)
    cap = Z.ZSTD_compressBound(host.size)
    buf = np.empty(cap, dtype=np.uint8)
    n = Z.ZSTD_compress(buf.ctypes.data, cap, raw, host.size, level)
    assert not Z.ZSTD_isError(n)
    return buf[:n].tobytes()


def test_one_large_foreign_zstd_frame(gpu_ctx, pna, codec):
    """What the reference writes for a large file: ONE frame (zstd::stream::write::Encoder, lib/src/compress.rs:32-41) -- here 96 MiB from the
    system libzstd.  The frame gets the descriptors, table slots and record space planned for the entry (k_zscan) and its 768 blocks are decoded
    side by side (k_zparse .. k_zexec); the one-workgroup kernel decodes the same frame when asked to (zdec_serial)."""
    if codec.system_libzstd() is None:
        pytest.skip("system libzstd (the writer of the test frame) is absent")
    raw = b"".join(codec.corpus_file(i % 3, 8300 + i, 1 << 20) for i in range(96))
    comp = _libzstd_one_frame(codec, raw)
    assert gpu_ctx.decompress_batch([comp], [len(raw)]) == [raw]
    t = gpu_ctx.timing()
    small = codec.corpus_file(0, 8299, 70000)
    assert gpu_ctx.decompress_batch([comp, _libzstd_one_frame(codec, small)], [len(raw), len(small)]) == [raw, small]
    bad = bytearray(comp); bad[len(bad) // 2] ^= 0x40
    try:
        assert gpu_ctx.decompress_batch([bytes(bad)], [len(raw)]) != [raw]
    except pna.PnaGpuError:
        pass
    assert t is not None


def test_parallel_executor_runs_in_windows(gpu_ctx, pna, codec):
    """The pointer-jumping executor (k_zexec_par.hip) takes a frame in WINDOWS of whole blocks -- a word counts from its window's start, a source in front of the
    window is a byte of the output already written --, 1 GiB each by default (frames of 2 GiB and more: tests/test_gpu_full_size.py).  With windows of 3 MiB a 40 MiB
    libzstd frame (window 2 - 8 MiB: matches reach across the cuts) crosses a dozen of them, a 20 MiB stdlib-zlib stream with windows of 1 MiB twenty: same bytes as
    with one window, damage still refused or different."""
    raw_d = b"".join(codec.corpus_file(i % 2, 9300 + i, 1 << 20) for i in range(20))
    comp_d = zlib.compress(raw_d, 6)
    cases = [(comp_d, raw_d, pna.ALGO_DEFLATE, 1)]
    if codec.system_libzstd() is not None:
        raw_z = b"".join(codec.corpus_file(i % 3, 9400 + i, 1 << 20) for i in range(40))
        raw_z = raw_z[:20 << 20] + raw_z[1 << 20:9 << 20] + raw_z[20 << 20:]                  # (a repeat 19 MiB back: inside the window of the higher levels)
        cases += [(_libzstd_one_frame(codec, raw_z, 3), raw_z, pna.ALGO_ZSTD, 3), (_libzstd_one_frame(codec, raw_z, 19), raw_z, pna.ALGO_ZSTD, 5)]
    for comp, raw, algo, win in cases:
        assert gpu_ctx.decompress_batch([comp], [len(raw)], algo=algo) == [raw]
        with gpu_ctx.options(zexec_win_mib=(win, 1024)):
            assert gpu_ctx.decompress_batch([comp], [len(raw)], algo=algo) == [raw], (algo, win)
            bad = bytearray(comp); bad[len(bad) * 3 // 4] ^= 0x10
            try:
                assert gpu_ctx.decompress_batch([bytes(bad)], [len(raw)], algo=algo) != [raw]
            except pna.PnaGpuError:
                pass


def test_large_foreign_zlib_streams_are_decoded_in_chunks(gpu_ctx, pna, codec):
    """One LARGE zlib stream of a foreign encoder (stdlib zlib: no sync flush every 128 KiB -- what the reference's flate2 writes for a large deflate entry) has no
    markers to cut it at: block starts are found by trial (k_ispec), the chunks between them walked side by side (k_inflate's chunk mode, count + emit), the records
    executed by pointer jumping.  Same bytes as the wave-per-stream walk (option zexec_par_min_mib = 0) for several levels and kinds of data; streams the scheme does not
    fit (stored blocks: incompressible data) fall back and still decode; damage is refused or decodes differently; small entries beside it are untouched."""
    import random
    rnd = random.Random(17)
    text = b"".join(codec.corpus_file(i % 2, 9100 + i, 1 << 20) for i in range(24))
    runs = bytearray()
    while len(runs) < (12 << 20):
        k = rnd.randrange(5)
        if k == 0: runs += bytes([rnd.randrange(256)]) * rnd.randrange(1, 200000)
        elif k == 1: runs += bytes(rnd.randrange(256) for _ in range(rnd.randrange(2, 9))) * rnd.randrange(10, 30000)
        elif k == 2: runs += text[rnd.randrange(len(text) - 70000):][:rnd.randrange(10, 70000)]
        elif k == 3: blk = bytes(runs[-32768:]); runs += blk * rnd.randrange(1, 4)
        else: runs += bytes(200000)
    noise = codec.corpus_file(2, 77, 3 << 20)
    cases = [("text-6", text, 6, True), ("text-1", text[:16 << 20], 1, True), ("text-9", text[:12 << 20], 9, True), ("runs-6", bytes(runs), 6, None),
             ("text+noise-6", text[:6 << 20] + noise + text[6 << 20:12 << 20], 6, None), ("noise-6", noise * 3, 6, None)]
    small = codec.corpus_file(0, 9099, 50000)
    for name, raw, lvl, must in cases:
        comp = zlib.compress(raw, lvl)
        got = gpu_ctx.decompress_batch([comp], [len(raw)], algo=pna.ALGO_DEFLATE)
        chunks = gpu_ctx.timing().lz_match_launches
        assert got == [raw], name
        if must: assert chunks == 1, (name, chunks)
        with gpu_ctx.options(zexec_par_min_mib=(0, 8)):
            if len(raw) <= (12 << 20):                                   # (the serial walk: ~0.1 s per MiB)
                assert gpu_ctx.decompress_batch([comp], [len(raw)], algo=pna.ALGO_DEFLATE) == [raw], name
                assert gpu_ctx.timing().lz_match_launches == 0
        assert gpu_ctx.decompress_batch([zlib.compress(small, 6), comp], [len(small), len(raw)], algo=pna.ALGO_DEFLATE) == [small, raw], name
    raw = text[:12 << 20]; comp = zlib.compress(raw, 6)
    for k in range(6):
        bad = bytearray(comp); bad[rnd.randrange(16, len(bad) - 8)] ^= 1 << rnd.randrange(8)
        try:
            assert gpu_ctx.decompress_batch([bytes(bad)], [len(raw)], algo=pna.ALGO_DEFLATE) != [raw]
        except pna.PnaGpuError:
            pass
    for cut in (len(comp) - 1, len(comp) - 5, len(comp) // 2):
        with pytest.raises(pna.PnaGpuError):
            gpu_ctx.decompress_batch([comp[:cut]], [len(raw)], algo=pna.ALGO_DEFLATE)


def test_foreign_solid_deflate_archive_is_extracted_in_chunks(gpu_ctx, pna, pf, codec):
    """What `pna create --solid --deflate` of the REFERENCE writes: the inner STORE records as ONE zlib stream of a foreign encoder, its decoded size recorded nowhere
    (built here with the oracle's writer and stdlib zlib).  The extract driver decodes it through the chunk decoder (open size: the count pass yields it) and walks the
    inner records; entries written by a foreign encoder as ordinary large deflate entries (fSIZ known) come out the same way."""
    n = 40
    ents = [codec.corpus_file(i % 2, 9300 + i, (1 << 20) - 7 * i) for i in range(n)]
    names = [f"fs/{i:03d}.txt" for i in range(n)]
    inner = b"".join(pf.write_normal_entry(pf.file_entry_header(pf.COMPRESSION_NO, nm), [d], len(d)) for nm, d in zip(names, ents))
    stream = zlib.compress(inner, 6)
    arc = pf.write_archive_header() + pf.write_solid_entry(pf.COMPRESSION_DEFLATE, pf.flatten_writer([stream])) + pf.finalize_archive()
    got = pna.extract_archive(gpu_ctx, arc)
    assert gpu_ctx.timing().lz_match_launches == 1
    assert [nm for nm, _, _ in got] == names and all(d == e for (_, _, d), e in zip(got, ents))
    big = b"".join(ents[:24])
    arc2 = (pf.write_archive_header() + pf.write_normal_entry(pf.file_entry_header(pf.COMPRESSION_DEFLATE, "big/one.txt"), pf.flatten_writer([zlib.compress(big, 6)]), len(big))
            + pf.write_normal_entry(pf.file_entry_header(pf.COMPRESSION_DEFLATE, "small.txt"), [zlib.compress(ents[30], 9)], len(ents[30])) + pf.finalize_archive())
    got2 = pna.extract_archive(gpu_ctx, arc2)
    assert [(nm, d) for nm, _, d in got2] == [("big/one.txt", big), ("small.txt", ents[30])]


def test_large_frames_are_executed_in_parallel(gpu_ctx, pna, codec):
    """k_zexec_par.hip: a large frame's sequences are executed by pointer jumping (repeat-offset codes resolved per block from a symbolic start history,
    one word per output byte, word[p] = word[word[p]] until every word holds a byte) instead of by one wave in order.  Same bytes as the serial
    executor (option zexec_par_min_mib = 0) for libzstd frames of several levels -- text (short matches, repeat codes in nearly every batch), long runs
    and periodic data (copy chains thousands deep: offsets 1, 2, 7, 64 KiB), incompressible stretches (raw blocks), RLE blocks --, with a content checksum,
    next to small frames in the same call; damage is refused or decodes differently."""
    if codec.system_libzstd() is None:
        pytest.skip("system libzstd (the writer of the test frames) is absent")
    import random
    rnd = random.Random(5)
    text = b"".join(codec.corpus_file(i % 2, 8600 + i, 1 << 20) for i in range(12))
    runs = bytearray()
    while len(runs) < (10 << 20):
        k = rnd.randrange(6)
        if k == 0: runs += bytes([rnd.randrange(256)]) * rnd.randrange(1, 300000)
        elif k == 1: runs += bytes(rnd.randrange(256) for _ in range(rnd.randrange(2, 9))) * rnd.randrange(10, 40000)
        elif k == 2: runs += text[rnd.randrange(len(text) - 70000):][:rnd.randrange(10, 70000)]
        elif k == 3: runs += codec.corpus_file(2, rnd.randrange(1000), rnd.randrange(1, 200000))
        elif k == 4: blk = bytes(runs[-65536:]); runs += blk * rnd.randrange(1, 4)
        else: runs += bytes(300000)
    cases = [("text-l1", text, 1), ("text-l3", text, 3), ("text-l19", text[:9 << 20], 19), ("runs-l3", bytes(runs), 3), ("runs-l1", bytes(runs), 1),
             ("zeros", bytes(20 << 20), 3), ("mixed-l5", bytes(runs[:5 << 20]) + text[:4 << 20], 5)]
    small = codec.corpus_file(0, 8599, 70000)
    for name, raw, lvl in cases:
        comp = codec.libzstd_compress(raw, lvl)
        assert codec.zstd_frame_count(comp, len(raw) + 64) == 1, name
        with gpu_ctx.options(zexec_par_min_mib=(0, 8)):
            want = gpu_ctx.decompress_batch([comp], [len(raw)])
        assert want == [raw], name
        assert gpu_ctx.decompress_batch([comp], [len(raw)]) == [raw], name
        assert gpu_ctx.decompress_batch([codec.libzstd_compress(small, 3), comp, comp[:]], [len(small), len(raw), len(raw)]) == [small, raw, raw], name
    comp = codec.libzstd_compress_checksum(text, 3)
    assert gpu_ctx.decompress_batch([comp], [len(text)]) == [text]
    for k in range(6):
        bad = bytearray(comp); bad[rnd.randrange(16, len(bad))] ^= 1 << rnd.randrange(8)
        try:
            assert gpu_ctx.decompress_batch([bytes(bad)], [len(text)]) != [text]
        except pna.PnaGpuError:
            pass


def test_one_workgroup_decoder_moves_its_bases(gpu_ctx, pna, codec):
    """k_zdec counts positions in 32 bits from bases that follow the frame (frames of 4 GiB and more: test_one_foreign_zstd_frame_beyond_4gib,
    minutes at one workgroup's speed).  The option zdec_dbg = 8 moves the bases every few MiB instead of every few GiB: a 24 MiB libzstd frame (window
    2 MiB) crosses them a dozen times and decodes to the same bytes."""
    if codec.system_libzstd() is None:
        pytest.skip("system libzstd (the writer of the test frame) is absent")
    raw = b"".join(codec.corpus_file(i % 3, 8400 + i, 1 << 20) for i in range(24))
    comp = _libzstd_one_frame(codec, raw)
    with gpu_ctx.options(zdec_serial=(1, 0), zdec_dbg=(8, 0)):
        assert gpu_ctx.decompress_batch([comp], [len(raw)]) == [raw]
        bad = bytearray(comp); bad[-3000] ^= 0x01
        try:
            assert gpu_ctx.decompress_batch([bytes(bad)], [len(raw)]) != [raw]
        except pna.PnaGpuError:
            pass


def test_damaged_large_streams_are_refused_or_differ(gpu_ctx, pna, codec):
    """Random damage to the streams the decoder's large-stream paths take -- a 6 MiB deflate entry of this library's (48 pieces, execution groups, marker scans on
    several workgroups), a 12 MiB libzstd frame (pooled per-entry resources) and a 10 MiB stdlib-zlib stream (the chunk decoder) --: every damaged stream is either refused (PNA_E_INVAL / UNSUPPORTED:
    structure, sizes, Adler-32, Content_Checksum) or decodes to different bytes; none hangs or reads outside its buffers (flate2 / zstd-rs return
    io::Error for the same inputs, lib/src/entry/read.rs:171-190)."""
    import random
    raw_d = b"".join(codec.corpus_file(i % 3, 8500 + i, 1 << 20) for i in range(6))
    comp_d = gpu_ctx.compress_batch([raw_d], algo=pna.ALGO_DEFLATE)[0]
    assert gpu_ctx.decompress_batch([comp_d] * 24, [len(raw_d)] * 24, algo=pna.ALGO_DEFLATE) == [raw_d] * 24       # (24 x 48 pieces: the lane-per-piece path)
    cases = [(comp_d, raw_d, pna.ALGO_DEFLATE)]
    if codec.system_libzstd() is not None:
        raw_z = b"".join(codec.corpus_file(i % 3, 8600 + i, 1 << 20) for i in range(12))
        cases.append((codec.libzstd_compress_checksum(raw_z, 3), raw_z, pna.ALGO_ZSTD))
    raw_f = b"".join(codec.corpus_file(i % 2, 8700 + i, 1 << 20) for i in range(10))
    cases.append((zlib.compress(raw_f, 6), raw_f, pna.ALGO_DEFLATE + 100))           # (+ 100: a FOREIGN zlib stream, alone in its call: the chunk decoder of round 4 -- trial block starts, chain check, fallback)
    seeds = range(2026, 2026 + int(os.environ.get("PNA_DAMAGE_SEEDS", "1")))       # (PNA_DAMAGE_SEEDS=N: a longer soak)
    for comp, raw, algo in cases:
        for seed in seeds:
            rng = random.Random(seed * 7 + algo)
            for trial in range(12):
                bad = bytearray(comp)
                kind = trial % 4
                if kind == 0:
                    bad[rng.randrange(len(bad))] ^= 1 << rng.randrange(8)
                elif kind == 1:
                    a = rng.randrange(len(bad) - 64); bad[a:a + 16] = bytes(rng.randrange(256) for _ in range(16))
                elif kind == 2:
                    bad = bad[:rng.randrange(len(bad) // 2, len(bad) - 1)]
                else:
                    a = rng.randrange(len(bad) - 4096); del bad[a:a + rng.randrange(1, 4096)]
                streams = [bytes(bad)] + ([comp] * 23 if algo == pna.ALGO_DEFLATE else [])
                try:
                    out = gpu_ctx.decompress_batch(streams, [len(raw)] * len(streams), algo=algo % 100)
                    assert out[0] != raw, (algo, seed, trial)
                except pna.PnaGpuError:
                    pass
