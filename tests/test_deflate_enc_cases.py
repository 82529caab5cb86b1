"""The crafted deflate-encoder inputs (deflate_enc_cases.py) on the CPU: every model stream inflates with zlib, passes the independent analyser
(the second implementation of the code build and the tokeniser must rebuild the very header the model wrote), and each family reaches the corner
it was made for -- so that the GPU test over the same cases (test_gpu_deflate_encode_branches.py) is known to run those corners on the device."""
import zlib

import pytest

import deflate_enc_cases as dc

CASES = dc.cases()
NAMES = [n for n, _, _ in CASES]
PLAIN = {n: p for n, p, _ in CASES}
LEVELS = {n: lv for n, _, lv in CASES}


def _records(prefix):
    """[(name, level, segment record)] of the cases whose name starts with `prefix`"""
    return [(n, lv, r) for n in NAMES if n.startswith(prefix) for lv in LEVELS[n] for r in dc.facts(n, lv)[1]]


def _dyn(prefix):
    return [(n, lv, r) for n, lv, r in _records(prefix) if r["ll"] is not None]


@pytest.mark.parametrize("name", NAMES)
def test_model_stream_inflates_and_rebuilds_from_its_counts(name):
    plain = PLAIN[name]
    assert len(plain) <= dc.SEG + 4096 or name.startswith("H."), "cases stay small"
    for level in LEVELS[name]:
        stream, recs = dc.facts(name, level)              # analyse() inside: replica lengths, tokens, code-length code, header sizes == the header
        assert zlib.decompress(stream) == plain, level
        assert int.from_bytes(stream[-4:], "big") == zlib.adler32(plain), level
        assert len(stream) <= dc.model_bound(len(plain)), level
        assert stream[:2] == (b"\x78\x01" if level == 0 else b"\x78\x9c"), level
        assert sum(r["size"] for r in recs) == len(plain)
        if level == 0:
            assert all(set(r["plan"]) == {"S"} for r in recs), "level 0: stored blocks only"


def test_a_deep_codes():
    recs = _dyn("A.")
    assert any(r["ll"]["down"] >= 1 for _, _, r in recs) and any(r["d"]["down"] >= 1 for _, _, r in recs)
    assert any(r["ll"]["up"] >= 8 for _, _, r in recs)
    assert any(r["ll"]["clamp"] and len(PLAIN[n]) <= 1 << 17 for n, _, r in recs)
    assert max(r["ll"]["maxdepth"] for _, _, r in recs) >= 20
    assert any(r["d"]["clamp"] and r["d"]["up"] >= 2 for _, _, r in recs)


def test_b_code_length_code_at_seven_bits():
    recs = _dyn("B.")
    assert all(r["cl"]["clamp"] and r["cl"]["maxdepth"] == 8 and max(r["cl_lens"]) == 7 for _, _, r in recs)
    assert any(r["cl"]["up"] >= 2 for _, _, r in recs) and any(r["cl"]["down"] >= 1 for _, _, r in recs)
    assert any(r["cl"]["up"] >= 1 and r["cl"]["down"] == 0 for _, _, r in recs)
    assert any(r["cl"]["clamp"] and len(PLAIN[n]) <= 32768 for n, _, r in recs), "one of them fits the wave-per-entry form"


def test_c_ties():
    by = {(n, lv): r for n, lv, r in _dyn("C.")}
    # every literal the same count: each merge of two leaves makes an inner node that ties with nothing smaller, the next level ties all the way
    assert by["C.permutations_x16_twice", 6]["ll"]["ties"] > 0 and by["C.equal_pairs_twice", 6]["ll"]["ties"] >= 128
    assert sum(1 for c in by["C.permutations_x16_twice", 6]["llc"][:256] if c == 16) >= 200        # (the copy's first bytes stay literals: a few counts of 17, 18)
    assert sum(1 for c in by["C.equal_pairs_twice", 6]["llc"][:256] if c == 2) >= 250
    assert by["C.powers_of_two", 6]["ll"]["ties"] > 0         # 1 + 1 = 2 ties with the leaf 2, 2 + 2 = 4 with the leaf 4 ...: an inner node against a leaf that is still queued
    assert sum(1 for c in by["C.equal_but_one", 6]["llc"][:256] if c) == 101
    for name, k in (("C.two_symbols", 2), ("C.three_symbols", 3), ("C.four_symbols", 4)):
        assert sum(1 for c in by[name, 6]["llc"][:256] if c) == k
    assert any(r["ll"]["n"] == 283 and r["hlit"] == 29 for r in by.values())
    # 283 is the most there can be: the LZ stage emits no match shorter than 6 (min_match 6, cut_min 6), so the symbols 257 .. 259 never occur
    assert max(r["ll"]["n"] for _, _, r in _dyn("")) == 283
    assert min(min(r["mlens"]) for _, _, r in _dyn("") if r["mlens"]) == 6
    hdr = max(r["hdr_bits"] for _, _, r in _dyn(""))
    print("largest header: %d bits" % hdr)
    assert hdr == by["C.largest_header", 6]["hdr_bits"] == LARGEST_HDR_BITS


LARGEST_HDR_BITS = 846        # measured; of at most 14 + 57 + 316 * 7 = 2 283


def test_d_degenerate_distance_codes():
    by = {(n, lv): r for n, lv, r in _records("D.")}
    r = by["D.no_match", 6]
    assert r["d"]["n"] == 0 and r["hdist"] == 0 and r["d_lens"] == [0] * 30 and r["seq"][-1] == 0 and len(r["seq"]) == 258
    r = by["D.one_distance", 6]
    assert r["d"]["n"] == 1 and sorted(r["d_lens"]) == [0] * 29 + [1]
    r = by["D.two_distances", 6]
    assert r["d"]["n"] == 2 and sorted(r["d_lens"]) == [0] * 28 + [1, 1]
    r = by["D.distance_32768", 6]
    assert r["hdist"] == 29 and 32768 in r["dists"]
    for level in (0, 1, 6, 9):
        assert dc.facts("D.entry_of_0", level)[0] == (bytes.fromhex("7801010000ffff00000001") if level == 0 else bytes.fromhex("789c030000000001"))
        for n in (1, 2, 5):
            assert by["D.entry_of_%d" % n, level]["plan"] == "S"            # too short to pay for a table: one stored block


def test_e_zero_run_edges():
    reached = set()
    for n, lv, r in _dyn("E."):
        assert len(PLAIN[n]) <= 2048
        reached |= dc.branches([r])
        # the runs as the tokens tell them: a run of R zeros is R // 138 tokens "18 x 138" and the greedy rest
        it = iter(r["tokens"])
        for a, ln in r["runs"]:
            want = [(18, 138)] * (ln // 138) + ([(18, ln % 138)] if ln % 138 >= 11 else [(17, ln % 138)] if ln % 138 >= 3 else [(0, 1)] * (ln % 138))
            got = []
            while len(got) < len(want):
                t = next(it)
                if t[0] in (0, 17, 18):
                    got.append(t)
            assert got == want, (n, a, ln)
    for ln in dc.RUN_LENGTHS:
        assert "run_%d" % ln in reached, ln
    for b in dc.BORDERS:
        if b not in ("start_257", "run_in_distances"):             # (those two need matches: family D)
            assert b in reached, b


def _f_tables():
    lens, dists = set(), set()
    for _, _, r in _dyn("F."):
        lens |= set(r["mlens"]); dists |= set(r["dists"])
    return lens, dists


# distance codes 0 .. 23 (1 .. 4 096 bytes back): a source must lie before the 4 096-byte tile of the position that finds it, so these are found in the
# first positions of a tile only.  Code: the ends of its range that the F cases reach, at any of the levels 1, 6, 9.
NEAR_ENDS_REACHED = {0: (1,), 1: (2,), 2: (3,), 3: (4,), 4: (5, 6), 5: (7, 8), 6: (9, 12), 7: (13, 16), 8: (17, 24), 9: (25, 32), 10: (33, 48), 11: (49, 64),
                     12: (65, 96), 13: (97, 128), 14: (129, 192), 15: (193, 256), 16: (257, 384), 17: (385, 512), 18: (513, 768), 19: (769, 1024),
                     20: (1025, 1536), 21: (1537, 2048), 22: (2049, 3072), 23: (3073, 4096)}          # (measured: every end)


def test_f_symbols_and_extra_bits():
    lens, dists = _f_tables()
    assert min(lens) == 6 and max(lens) == 258 and not lens & {3, 4, 5}        # 3 .. 5 would come from front cuts only, and cut_min is 6 here
    for code in range(3, 29):
        lo, hi = dc.len_range(code)
        assert lo in lens and hi in lens, (code, lo, hi)
    assert lens >= set(range(6, 259))
    codes = {c for c in range(30) for d in dists if dc.dist_range(c)[0] <= d <= dc.dist_range(c)[1]}
    assert codes == set(range(30))
    for code in range(24, 30):
        lo, hi = dc.dist_range(code)
        assert lo in dists and hi in dists, (code, lo, hi)
    table = {c: tuple(e for e in sorted(set(dc.dist_range(c))) if e in dists) for c in range(24)}
    print("near distance ends reached:", table)
    assert table == NEAR_ENDS_REACHED


def test_g_block_plan_and_writer():
    by = {(n, lv): r for n, lv, r in _records("G.")}
    assert by["G.stored_3_pieces", 6]["pieces"] == [[65535, 65535, 2]]
    assert by["G.alternating", 6]["plan"] == "SDSDSD"
    assert by["G.final_stored", 6]["plan"] == "DS" and by["G.final_dynamic", 6]["plan"] == "SD"
    assert by["G.last_block_1_byte", 6]["plan"] == "DS" and by["G.last_block_1_byte", 6]["pieces"] == [[1]]
    r = by["G.dense_tile", 6]
    print("densest tile: %d literal bits" % r["lit_bits"][100])
    assert r["lit_bits"][100] >= 30000 and r["lit_bits"][100] == max(r["lit_bits"].values()) == DENSEST_TILE_BITS
    # where the end-of-block code ends inside its byte: all eight places, behind which the writer puts the 3-bit empty stored header and aligns
    assert {k for _, _, rr in _records("") for k in rr["eob_bits"]} == set(range(8))
    assert len({k for _, _, rr in _records("G.") for k in rr["eob_bits"]}) >= 6
    for n in (0, 1, 65535, 65536, 1 << 17, (1 << 17) + 1, 3 * (1 << 17) + 7):
        stream, recs = dc.facts("G.level0_%d" % n, 0)
        assert stream[:2] == b"\x78\x01" and len(stream) == (11 if n == 0 else 2 + n + 5 * sum(len(p) for r in recs for p in r["pieces"]) + 5 * (-(-n // (1 << 17)) - 1) + 4)


DENSEST_TILE_BITS = 30720          # 2 048 literals of 15 bits: all the staging area of k_dblock is sized for


def test_h_adler():
    """the trailer the analyser read is zlib's sum; the sizes sit around the 5 552 bytes that may be summed before a reduction, the modulus 65 521 and the
    block and segment sizes, of the bytes with the largest sums"""
    for n, lv, r in _records("H."):
        assert r["adler"] == zlib.adler32(PLAIN[n]), (n, lv)
    assert {len(PLAIN[n]) for n in NAMES if n.startswith("H.ff_")} >= {1, 5552, 5553, 65521, 1 << 17, (1 << 20) + 1, (3 << 20) + 17}
    assert len(_records("H.ff_3145745")) == 4 and len(_records("H.ff_00_blocks_2mib")) == 2              # entries of several segments: sums combined over all their blocks


def test_every_branch_is_reached_by_some_case():
    reached = {}
    for n in NAMES:
        for lv in LEVELS[n]:
            for b in dc.branches(dc.facts(n, lv)[1]):
                reached.setdefault(b, (n, lv))
    for b in dc.BRANCHES:
        assert b in reached, b
    deepest = max((r["ll"]["maxdepth"], n) for n, _, r in _dyn(""))
    ups = max((max(r[k]["up"] for k in ("ll", "d", "cl")), n) for n, _, r in _dyn(""))
    downs = max((max(r[k]["down"] for k in ("ll", "d", "cl")), n) for n, _, r in _dyn(""))
    print("deepest", deepest, "most up", ups, "most down", downs)
    assert (deepest[0], ups[0], downs[0]) == MEASURED_DEPTH_UP_DOWN


MEASURED_DEPTH_UP_DOWN = (20, 37, 7)          # measured: A.geo_1.1_x256, C.largest_header, F.near
