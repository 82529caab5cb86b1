"""The parse kernel's load rounds (k_lzp: a tile's words in one round, a group's offsets eight at a time), and the sequence coder's chunks.

Small inputs built for the branches those rounds have: groups of 64 positions with more chosen starts than one turn takes and groups with none, partial
last tiles whose length is no multiple of 4, 256 or 1 024, capped matches that are extended from memory, a match cut from the front at a region border,
and short entries whose words come from the one-wave match kernel.  The CPU part asserts from the model's sequences that the inputs do hold these
cases, so that the GPU part cannot quietly stop covering them; the GPU part compares the streams with the model bit for bit, for every instance of the
kernel (both codecs, the lazy depths of the level sets, words of three and of four bytes), and takes them through the device decoder.
"""
import functools
import random

import pytest

from conftest import headline_context

TILE = 4096
FAR_FROM = 28368            # offsets from here on lie outside the match kernel's window


def _words_input(n, seed=20240611, nwords=1500):
    """A dictionary of 1 500 (nwords) random 6-byte words at stride 8, then -- until n + 5 bytes are there -- 3 000 times a dictionary word + 1 random byte, 3 000
    random bytes, 800 more word + byte pairs; the last 5 bytes cut off.  n = 41 595 is the main input: one turn of each section."""
    rnd = random.Random(seed)
    rb = lambda k: bytes(rnd.getrandbits(8) for _ in range(k))
    words = [rb(6) for _ in range(nwords)]
    out = bytearray()
    for w in words:
        out += w + rb(2)
    pair = lambda: rnd.choice(words) + rb(1)
    while len(out) < n + 5:
        for _ in range(3000):
            out += pair()
        out += rb(3000)
        for _ in range(800):
            out += pair()
    return bytes(out[:n])


MAIN_LEN = 1500 * 8 + 3000 * 7 + 3000 + 800 * 7 - 5       # 41 595: 10 tiles and 635 positions


@functools.lru_cache(maxsize=None)
def _main():
    return _words_input(MAIN_LEN)


@functools.lru_cache(maxsize=None)
def _runs_input():
    """300-byte repeats at distances below and above FAR_FROM -- capped in the words, extended from memory --, two of them starting in the same half-group
    of two regions of one tile (the walk meets them in one turn), one running across region borders."""
    rnd = random.Random(77)
    rb = lambda k: bytes(rnd.getrandbits(8) for _ in range(k))
    R, Q = rb(300), rb(300)
    d = bytearray(rb(11 * TILE + 200 + 300 + 13 + 300 + 517))
    def put(at, piece): d[at:at + len(piece)] = piece
    put(2 * TILE + 256 + 40, R)                             # the sources, at even positions
    put(2 * TILE + 1024 + 40, Q)
    put(3 * TILE + 256 + 40, R)                             # distance 4 096: inside the window; region 1 of tile 3, half-group 1
    put(3 * TILE + 1024 + 40, Q)                            # three regions on, the same half-group
    put(11 * TILE + 200, R)                                 # distances above FAR_FROM, across region borders
    put(11 * TILE + 200 + 313, Q)
    return bytes(d)


@functools.lru_cache(maxsize=None)
def _cut_input():
    """A match that ends 6 positions into a region (250 .. 262 of tile 1) over a longer one that starts at 258 inside that region: the region's own walk
    chose 258, the merge enters at 262 and cuts the front off -- the sequence at 262 takes its offset from the word at 258."""
    rnd = random.Random(91)
    rb = lambda k: bytes(rnd.getrandbits(8) for _ in range(k))
    X = rb(12)
    Y = X[8:] + rb(16)                                      # 20 bytes whose first four are X's last
    d = bytearray(rb(600))
    d[100:112] = X                                          # sources at even positions (the default set inserts those)
    d[300:320] = Y
    d += rb(TILE + 250 - len(d))
    d += X[:8] + Y                                          # 250 .. 261 = X, 258 .. 277 = Y
    d += rb(700)
    return bytes(d)


def _starts(codec, data, level=3):
    """Absolute positions of the model's chosen starts, with their match lengths and offsets."""
    out = []
    base = 0
    for seqs, _lits in codec.model_lz_segment(data, codec.params_for_level(level)):
        pos = base
        for ll, ml, off in seqs:
            pos += ll
            out.append((pos, ml, off))
            pos += ml
        base += 1 << 17
    return out


def test_inputs_hold_the_cases(codec):
    d = _main()
    assert len(d) == MAIN_LEN
    per_group = {}
    for pos, _ml, _off in _starts(codec, d):
        per_group[pos >> 6] = per_group.get(pos >> 6, 0) + 1
    ngroups = (len(d) + 63) >> 6
    assert max(per_group.values()) > 8                                      # more than a turn of eight (and of four)
    assert sum(1 for g in range(ngroups) if g not in per_group) > 0          # groups without a start
    npos = len(d) % TILE
    assert npos != 0 and npos % 4 != 0 and npos % 256 != 0                  # a partial last tile that ends inside a lane's four positions
    # the capped matches: longer than the words can say, near and far
    runs = [(p, ml, off) for p, ml, off in _starts(codec, _runs_input()) if ml >= 200]
    assert any(off < FAR_FROM for _p, _ml, off in runs) and any(off >= FAR_FROM for _p, _ml, off in runs)
    assert len({(p % TILE) // 256 for p, _ml, _off in runs if p // TILE == 3 and (p % 256) // 32 == 1}) >= 2   # two regions, one half-group
    # the front-cut match: a sequence that starts where the one before it ended, 6 positions into a region, with the inner match's offset
    st = _starts(codec, _cut_input())
    assert (TILE + 250, 12, TILE + 150) in st and (TILE + 262, 16, TILE + 258 - 300) in st


@functools.lru_cache(maxsize=None)
def _variants():
    small = [_words_input(4096, seed=1000 + i, nwords=60) for i in range(64)] + [_words_input(12288, seed=2000 + i, nwords=60) for i in range(64)]
    return {"main": [_main()],
            "two blocks": [_words_input((1 << 17) + TILE + 3), _words_input((1 << 17) + TILE + 1021, seed=5)],     # a block of one tile and 3 (1 021) positions
            "runs": [_runs_input()], "cut": [_cut_input()], "small": small}


# ---- the sequence coder (k_seq): chunks of four sequences, the block's last one peeled off, the others requested two chunks ahead
SEQ_COUNTS = (1, 2, 3, 4, 5, 8, 9, 12, 13)


@functools.lru_cache(maxsize=None)
def _counted(n):
    """An entry of one block whose parse has exactly n sequences: 17 000 random bytes (more than the short segments' geometry takes, so that the model of
    one segment is the product's), then n 10-byte repeats of bytes of its first tile, 40 random bytes between them."""
    rnd = random.Random(300 + n)
    rb = lambda k: bytes(rnd.getrandbits(8) for _ in range(k))
    d = bytearray(rb(17000))
    for i in range(n):
        d += d[16 * i + 8:16 * i + 18] + rb(40)
    return bytes(d)


@functools.lru_cache(maxsize=None)
def _dense():
    """One block of 128 KiB with as many sequences as a block takes: behind the dictionary, dictionary words back to back -- a match of six bytes at
    every sixth position, no literals between them."""
    rnd = random.Random(4)
    rb = lambda k: bytes(rnd.getrandbits(8) for _ in range(k))
    words = [rb(6) for _ in range(1500)]
    d = bytearray()
    for w in words:
        d += w + rb(2)
    while len(d) < (1 << 17):
        d += rnd.choice(words)
    return bytes(d[:1 << 17])


def test_sequence_counts(codec):
    p = codec.params_for_level(3)
    for n in SEQ_COUNTS:
        (seqs, _lits), = codec.model_lz_segment(_counted(n), p)
        assert len(seqs) == n, n
    (seqs, _lits), = codec.model_lz_segment(_dense(), p)
    # a block takes at most 2^17 / 6 = 21 845 sequences (22 528 slots); behind the 12 000 bytes of dictionary 19 845 words fit, and the finder misses some:
    # three quarters of the block's bound is asked for -- 4 096 chunks of four
    assert len(seqs) >= 16384, len(seqs)


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["lane per segment", "lane per block"])
def test_sequence_coder_chunks(pna, codec, form):
    """k_seq<true> (every entry one block) and k_seq<false> (an entry of two blocks in the batch, statistics per segment): blocks of 1 .. 13 sequences
    -- the peeled last chunk with one to four sequences in it, then none, one, two, three more chunks, so that the requests two chunks ahead meet the
    block's front at every distance -- and a block as full of sequences as blocks get."""
    data = [_counted(n) for n in SEQ_COUNTS] + [_dense()]
    if form == "lane per block":
        data = data + [_variants()["two blocks"][0]]
    p = codec.params_for_level(3)
    with headline_context(pna) as ctx:
        ctx.set_option("lz_split_min", 0)
        ctx.set_option("hist_by_block", 0)
        outs = ctx.compress_batch(data)
        bad = [i for i, (d, o) in enumerate(zip(data, outs)) if o != codec.model_compress(d, p)]
        assert not bad, (form, bad)
        assert ctx.decompress_batch(outs, [len(d) for d in data]) == data


@pytest.fixture(scope="module")
def variants():
    return _variants()


@pytest.fixture(scope="module")
def split_ctx(pna):
    import torch  # noqa: F401  (shares its HIP runtime with the extension)
    ctx = headline_context(pna)
    ctx.set_option("lz_split_min", 0)
    yield ctx
    ctx.close()


@functools.lru_cache(maxsize=None)
def _want(key, i, algo, level):
    from oracle import codec
    d = _variants()[key][i]
    if algo == "deflate":
        return codec.deflate_model_compress(d, codec.params_for_level(level, deflate=True))
    return codec.model_compress(d, codec.params_for_level(level))


@pytest.mark.gpu
@pytest.mark.parametrize("algo,level", [("zstd", 1), ("zstd", 2), ("zstd", 3), ("zstd", 7), ("deflate", 6)])
def test_streams_equal_the_model_and_decode(split_ctx, pna, codec, variants, algo, level):
    """Every instance of the parse kernel behind the split form: CT (deflate), the lazy depths of the level sets, words of three bytes."""
    a = pna.ALGO_DEFLATE if algo == "deflate" else pna.ALGO_ZSTD
    for key, data in variants.items():
        outs = split_ctx.compress_batch(data, algo=a, level=level)
        bad = [i for i, o in enumerate(outs) if o != _want(key, i, algo, level)]
        assert not bad, (key, algo, level, bad[:6])
        assert split_ctx.decompress_batch(outs, [len(d) for d in data], algo=a) == data, (key, algo, level)


@pytest.mark.gpu
@pytest.mark.parametrize("level", [3, 7])
def test_four_byte_words(pna, codec, variants, level):
    """lz_split = 2: the short entries' words take four bytes in front of the same parse kernel (its W3 = false instances)."""
    with headline_context(pna) as ctx:
        ctx.set_option("lz_split_min", 0)
        ctx.set_option("lz_split", 2)
        for key, data in variants.items():
            outs = ctx.compress_batch(data, level=level)
            bad = [i for i, o in enumerate(outs) if o != _want(key, i, "zstd", level)]
            assert not bad, (key, level, bad[:6])
            assert ctx.decompress_batch(outs, [len(d) for d in data]) == data, (key, level)
