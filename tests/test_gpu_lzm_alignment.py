"""The match step of k_lzm's default-set instances compares a candidate in the LANE'S alignment (near_match in k_lz_split.hip): one XOR stream per lane and
candidate, read from byte j on for position q0 + j; the other instances and k_lzms shift both sides.  What can go wrong in either depends on j = q & 3, on the candidate's alignment (q0 - o) & 3, on where the match
ends (inside the first 16 bytes, at the seam, in the second 16, in the ninth dword behind them, past the cap) and on how many bytes before the position
agree.  These inputs plant exactly such copies into incompressible filler; every stream must be the model's (oracle/codec.py), bit for bit.

A plant (q, o, L, B): the bytes q - B .. q + L - 1 are those at q - o - B .. q - o + L - 1, the bytes right before and right behind differ.  The
un-marked test checks on the CPU that the model really finds each plant as one sequence of B + L bytes at q - B -- the filler adds nothing longer --
and that every value of the matrix is among those it finds."""
import random

import pytest

from conftest import headline_context

LENGTHS = (5, 6, 15, 16, 17, 31, 32, 33, 36)        # below the minimum, both sides of the seam of the two 16-byte steps, the cap of 32, the ninth dword
BACKS = (0, 3, 4, 7, 8, 15)                          # the caps of the three sets (3, 7, 15 back bytes) and one more each
ALIGN = tuple((j, a) for j in range(4) for a in range(4))      # j = q & 3, a = (q0 - o) & 3 = -o & 3
ROOM = 16                                            # a plant's position lies ROOM + j bytes into its slot: 15 back bytes and the byte that differs in front


def _plant(buf, q, c, L, B):
    assert 0 <= c - B - 1 and c + L < q - B - 1 and q + L <= len(buf)
    buf[q - B:q + L] = buf[c - B:c + L]
    buf[q - B - 1] = buf[c - B - 1] ^ 0x5A
    if q + L < len(buf):
        buf[q + L] = buf[c + L] ^ 0xA5


def _build(n, seed, cases, src0, dst0, src_step, dst_step, group=0, group_step=0):
    """n bytes of filler with one plant per case (j, a, L, B): sources from src0 on, every src_step bytes, positions from dst0 on, every dst_step;
    group != 0: in groups of that many, a group's first source and position group_step behind those of the group before."""
    buf = bytearray(random.Random(seed).randbytes(n))
    plants = []
    for i, (j, a, L, B) in enumerate(cases):
        g, k = (i // group, i % group) if group else (0, i)
        sb, db = src0 + group_step * g + src_step * k, dst0 + group_step * g + dst_step * k
        assert sb % 4 == 0 and db % 4 == 0 and ROOM + 3 + 36 + 1 <= min(src_step, dst_step)
        q, c = db + ROOM + j, sb + ROOM + ((j + a) & 3)
        assert q & 3 == j and (q - c + a) & 3 == 0
        _plant(buf, q, c, L, B)
        plants.append((q, q - c, L, B))
    return bytes(buf), plants


def _near_segments():
    """Three tiles and a tail each (the last tile partial): sources in tile 0, positions in tile 1, 63 plants a segment -- the whole cross product."""
    cases = [(j, a, L, B) for (j, a) in ALIGN for L in LENGTHS for B in BACKS]
    return [_build(3 * 4096 + 300, 1000 + k, cases[k:k + 63], 64, 4096 + 64, 64, 64) for k in range(0, len(cases), 63)]


def _far_segment():
    """About 48 KiB: the sixteen alignments with the candidate at 8, 9, 10, 11 (its back bytes reach the segment's first: B = c - 1 <= 7) from one tile, so
    that none of them is another's nearer candidate, then alignments x lengths with the back counts in turn; every offset beyond the 28 368 bytes that
    the 32 KiB window looks back."""
    n = 48 * 1024 + 300
    buf = bytearray(random.Random(2000).randbytes(n))
    plants = []
    for i, (r, c) in enumerate((r, c) for r in range(4) for c in (8, 9, 10, 11)):
        q, L, B = 28828 + 112 * i + r, LENGTHS[1 + i % 8], min(c - 1, 7)       # (28 828: no group of 64 positions, where adoption stops, begins inside the back bytes)
        _plant(buf, q, c, L, B)
        plants.append((q, q - c, L, B))
    for i, (j, a, L) in enumerate((j, a, L) for (j, a) in ALIGN for L in LENGTHS):
        q, c, B = 30720 + 112 * i + ROOM + j, 64 + 64 * i + ROOM + ((j + a) & 3), BACKS[i % 6]
        _plant(buf, q, c, L, B)
        plants.append((q, q - c, L, B))
    assert all(o > 28368 + 64 for _, o, _, _ in plants)
    return bytes(buf), plants


def _short_entries():
    """4 096 bytes (one plant per alignment, lengths and back counts in turn) and 16 KiB (alignments x lengths): k_lzms, whose sub-tiles of 256
    positions see the inserts of the sub-tiles before them."""
    small = [(j, a, LENGTHS[i % 9], BACKS[i % 6]) for i, (j, a) in enumerate(ALIGN)]
    mid = [(j, a, L, BACKS[i % 6]) for i, (j, a, L) in enumerate((j, a, L) for (j, a) in ALIGN for L in LENGTHS)]
    # (16 KiB: eight sources, then their eight positions 448 bytes on -- the next sub-tile or the one after --, so that few of the 2 048 slots' later inserts lie between)
    return [_build(4096, 3000, small, 64, 2048 + 64, 64, 64), _build(16384, 3001, mid, 64, 64 + 448, 56, 56, group=8, group_step=896)]


def _end_segments():
    """Blocks of 8 KiB (two tiles): a copy that runs across the block's end at 8 192 and at 16 384, and one that runs to the segment's last byte, from
    every j over the four segments; the last tile is partial."""
    out = []
    for k in range(4):
        n = 20480 + 300 + k
        buf = bytearray(random.Random(4000 + k).randbytes(n))
        plants = []
        for end, j, c in ((8192, k, 1000), (16384, (k + 2) & 3, 12000)):
            q = end - 24 + j                                        # 21 .. 24 bytes before the end, 40 bytes alike: the match ends with the block
            _plant(buf, q, c, 40, 2)
            plants.append((q, q - c, end - q, 2))
        q = n - 19                                                  # q & 3 = k + 1: the copy ends with the segment
        _plant(buf, q, 14000, 19, 1)
        plants.append((q, q - 14000, 19, 1))
        out.append((bytes(buf), plants))
    return out


def _low_entries(n, dst0, sets):
    """Candidates at the segment's start, where a - 8 (STRONG = 2: a - 16) is negative for j > 0 and the step's base address wraps to the window's last dword
    (k_lzm: the data comes from the mirror) or into the bytes in front of the segment (k_lzms): c = 8 .. 11 with every back byte there is, c = 16 .. 19
    with 15.  One entry per j and set: its four positions lie in one sub-tile, so none is another's candidate."""
    out = []
    for cs, B in sets:
        for j in range(4):
            buf = bytearray(random.Random(5000 + 4 * cs[0] + j).randbytes(n))
            plants = []
            for i, c in enumerate(cs):
                q = dst0 + 64 * i + 20 + j                          # (20: no group of 64 positions, where adoption stops, begins inside the back bytes)
                _plant(buf, q, c, 20, min(c - 1, B))
                plants.append((q, q - c, 20, min(c - 1, B)))
            out.append((bytes(buf), plants))
    return out


LOW_SETS = (((8, 9, 10, 11), 7), ((16, 17, 18, 19), 15))


@pytest.fixture(scope="module")
def cases():
    return {"near": _near_segments(), "far": [_far_segment()], "short": _short_entries(), "ends": _end_segments(),
            "low_near": _low_entries(3 * 4096 + 300, 4096 + 1024, LOW_SETS), "low_short": _low_entries(4096, 512, LOW_SETS)}


_MODEL = {}


def _model(codec, data, level, blk_log=0, small_seg=None):
    key = (data, level, blk_log, small_seg)
    if key not in _MODEL:
        p = codec.params_for_level(level, blk_log=blk_log)
        if small_seg is not None:
            p.small_seg = small_seg
        _MODEL[key] = codec.model_compress(data, p)
    return _MODEL[key]


def _found(codec, data, plants, level, blk_log=0, small_seg=None):
    """The plants that the model's LZ stage emits as exactly one sequence (q - B, B + L, o)."""
    p = codec.params_for_level(level, blk_log=blk_log)
    if small_seg is not None:
        p.small_seg = small_seg
    # the parameters the segment really runs with (zstd_model.c pna_seg_params): the small geometry for at most 16 KiB
    slots = p.small_slots if p.small_seg and len(data) <= p.small_seg else (p.mid_slots if p.small_seg and p.mid_seg and len(data) <= p.mid_seg else 0)
    if slots:
        p.hash_log, p.tab3, p.mtile = slots, 0, p.small_tile
    blk = (1 << blk_log) if blk_log else (1 << 17)
    seqs = {}
    for b, (ss, _) in enumerate(codec.model_lz_segment(data, p)):
        pos = b * blk
        for ll, ml, off in ss:
            pos += ll
            seqs[pos] = (ml, off)
            pos += ml
    return [pl for pl in plants if seqs.get(pl[0] - pl[3]) == (pl[2] + pl[3], pl[1])], seqs


# the plants (entry of the group, q, o, L, B) that the model does NOT emit as their own sequence: an insert lost in the packed table's contest of a tile (or overwritten in the
# short segments' small table) leaves a plant to a neighbouring position's shorter match.  The inputs are seeded: another set means that the inputs or the model have moved.
MISSED = {
    "near": {(0, 8016, 4095, 6, 0), (2, 6864, 4093, 6, 0), (3, 5456, 4093, 33, 15), (3, 6289, 4096, 6, 0), (5, 5137, 4094, 6, 0), (7, 7442, 4095, 6, 0), (9, 6290, 4097, 6, 0),
             (10, 5715, 4096, 6, 0), (11, 4819, 4099, 5, 3), (12, 4563, 4098, 6, 0), (12, 7699, 4097, 5, 3)},
    "far": {(0, 30848, 30704, 6, 3), (0, 34881, 32432, 6, 3), (0, 37569, 33582, 33, 3), (0, 38914, 34160, 6, 3), (0, 41602, 35314, 33, 3)},
    "short": set(), "ends": set(),
    "low_near": {(7, 5143, 5127, 20, 15), (7, 5207, 5190, 20, 15)},
    "low_short": {(2, 534, 526, 20, 7), (2, 598, 589, 20, 7)},
}


def test_the_model_finds_the_plants(codec, cases):
    """On the CPU, with the parameters each segment really runs with: at the default level the model emits every plant of six bytes or more as its own
    sequence but for the few listed in MISSED, nothing the filler made by chance is a match at all, and the plants found cover the matrix
    JOINTLY: every length from every j and with every alignment, every back count from every j."""
    for group, small_seg, blk_log in (("near", 0, 0), ("far", None, 0), ("short", None, 0), ("ends", None, 13), ("low_near", 0, 0), ("low_short", None, 0)):
        want, got, longest, missed = [], [], 0, set()
        for i, (data, plants) in enumerate(cases[group]):
            f, seqs = _found(codec, data, plants, 3, blk_log, small_seg)
            want += [pl for pl in plants if pl[2] + pl[3] >= 6]
            got += f
            missed |= {(i,) + pl for pl in plants if pl[2] + pl[3] >= 6 and pl not in f}
            planted = {x for q, _, L, B in plants for x in range(q - B - 1, q + L)}
            longest = max([longest] + [ml for pos, (ml, _) in seqs.items() if pos not in planted])
        print(group, len(got), "of", len(want), "plants found; longest sequence outside them", longest, "; missed", sorted(missed))
        assert missed == MISSED[group], group
        if group == "ends":                                            # (behind a block's end the rest of the copy is a sequence of its own)
            assert {q & 3 for q, _, _, _ in got} == {0, 1, 2, 3}
            continue
        assert longest < 6, group                                      # the filler made no match by chance
        if group in ("low_near", "low_short"):                        # the base address wraps for j > 0: candidates at 8 .. 10, and at 16 .. 18 for the sets with 15 back bytes
            for j in (1, 2, 3):
                assert any(q & 3 == j and q - o <= 10 for q, o, _, _ in got) and any(q & 3 == j and 16 <= q - o <= 18 for q, o, _, _ in got), (group, j)
            continue
        # jointly: every length (the ninth dword's 33 and 36 among them) and every back count from every j and with every alignment of the candidate
        assert {(q & 3, -o & 3) for q, o, _, _ in got} == set(ALIGN), group
        assert {(q & 3, L) for q, _, L, _ in got} >= {(j, L) for j in range(4) for L in LENGTHS[1:]}, group
        assert {(-o & 3, L) for _, o, L, _ in got} >= {(a, L) for a in range(4) for L in LENGTHS[1:]}, group
        if group == "near":
            assert {(q & 3, B) for q, _, _, B in got} == {(j, B) for j in range(4) for B in BACKS}, group
            assert {(q & 3, -o & 3, L) for q, o, L, _ in got} >= {(j, a, L) for j, a in ALIGN for L in LENGTHS[1:]}, group
        else:
            assert {B for _, _, _, B in got} >= set(BACKS), group
    far_low = [pl for pl in _found(codec, *cases["far"][0], 3)[0] if pl[0] - pl[1] < 12]
    assert {q - o for q, o, _, _ in far_low} == {8, 9, 10, 11} and {q & 3 for q, _, _, _ in far_low} == {0, 1, 2, 3}
    # a plant of five bytes without back bytes is no match
    assert all(pl not in _found(codec, d, p, 3, 0, 0)[0] for d, p in cases["near"] for pl in p if pl[2] + pl[3] < 6)


def _check(pna, codec, ctx, entries, level, small_seg=None):
    outs = ctx.compress_batch(entries, algo=pna.ALGO_ZSTD, level=level)
    t = ctx.timing()
    blk_log = 0 if t.blk_log == 17 else t.blk_log
    for i, (e, o) in enumerate(zip(entries, outs)):
        assert o == _model(codec, e, level, blk_log, small_seg), (i, len(e), level, t.blk_log)
        assert codec.zstd_decompress(o, len(e)) == e, (i, len(e), level)
    return t


# zstd 3: the default set (STRONG = 1, 7 back bytes); 2: the light set (STRONG = 0, 3 back bytes); 7: the high set (STRONG = 2, 15 back bytes, 16 KiB window);
# 1: the fast set, which enters EVERY position into its table -- with even positions only, q and o have the same parity and half the alignments are a neighbour's
NEAR_LEVELS = (3, 2, 7, 1)


@pytest.mark.gpu
@pytest.mark.parametrize("level", NEAR_LEVELS)
def test_near_candidates(pna, codec, cases, level):
    """Segments of three tiles, those with candidates at the segment's start among them, through k_lzm (small_geometry = 0: the large geometry for segments of at most 16 KiB; the model's small_seg = 0)."""
    import torch  # noqa: F401
    with headline_context(pna) as ctx:
        ctx.set_option("small_geometry", 0)
        t = _check(pna, codec, ctx, [d for d, _ in cases["near"] + cases["low_near"]], level, small_seg=0)
        assert t.lz_match_launches > 0


@pytest.mark.gpu
def test_far_candidates(pna, codec, cases):
    """One segment whose candidates lie beyond the window, first in the batch: its first byte is the source buffer's first."""
    import torch  # noqa: F401
    with headline_context(pna) as ctx:
        t = _check(pna, codec, ctx, [cases["far"][0][0], cases["near"][0][0]], 3)
        assert t.lz_match_launches > 0


@pytest.mark.gpu
def test_block_and_segment_ends(pna, codec, cases):
    """8 KiB blocks: matches clamped at a block's end and at the segment's, in the general (non-FULL) tile body."""
    import torch  # noqa: F401
    with pna.Context(0) as ctx:
        ctx.set_option("blk_log", 13)
        t = _check(pna, codec, ctx, [d for d, _ in cases["ends"]], 3)
        assert t.blk_log == 13


@pytest.mark.gpu
@pytest.mark.parametrize("level", NEAR_LEVELS)
def test_short_segments(pna, codec, cases, level):
    """4 096 bytes and 16 KiB, and 4 096-byte entries with candidates at their start: one wave per segment (k_lzms)."""
    import torch  # noqa: F401
    with headline_context(pna) as ctx:
        _check(pna, codec, ctx, [d for d, _ in cases["short"] + cases["low_short"]], level)
