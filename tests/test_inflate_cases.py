"""tests/inflate_cases.py against the system zlib: every accept case inflates to its plain bytes and ends with the stream, every reject case is refused,
and the properties the device test (tests/test_gpu_inflate_conformance.py) leans on hold.  No case may be dropped: a stream zlib disagrees with is a
mistake of the writer."""
import zlib

import pytest

import inflate_cases as C

ACCEPT = [c[0] for c in C.accept_cases()]


def by_name(name):
    return next(c for c in C.accept_cases() if c[0] == name)


def inflates_to(stream, plain):
    d = zlib.decompressobj()
    out = d.decompress(stream)
    return out == plain and d.eof and not d.unused_data and not d.unconsumed_tail


@pytest.mark.parametrize("name", ACCEPT)
def test_zlib_accepts(name):
    _, stream, plain, _ = by_name(name)
    assert inflates_to(stream, plain)
    assert C.play([]) == b"" and zlib.adler32(plain) == int.from_bytes(stream[-4:], "big")


def test_zlib_accepts_the_large_stream():
    _, stream, plain, props = C.large_case()
    assert inflates_to(stream, plain)
    kinds = [k for k, _ in props["blocks"]]
    assert len(plain) >= 1 << 20 and len(stream) >= 8 * 16384 and len(plain) <= 3 << 19
    assert kinds.count("dynamic") >= 41 and kinds[-1] == "dynamic" and kinds.count("stored") >= 8
    assert set(props["stored_phases"]) == set(range(8))
    assert [b % 8 for k, b in props["blocks"] if k == "stored"] == props["stored_phases"]


def test_zlib_accepts_the_large_streams_of_one_kind_of_block_start():
    cases = C.large_family_cases()
    assert [c[0] for c in cases] == ["large-deep-only", "large-one-dist-code-only", "large-stored-starts-only"]
    for (name, stream, plain, props), kinds in zip(cases, ({"dynamic"}, {"dynamic"}, {"stored", "fixed"})):
        assert inflates_to(stream, plain), name
        assert 1 << 20 <= len(plain) <= 3 << 19 and len(stream) >= 8 * 16384, (name, len(plain), len(stream))
        assert {k for k, _ in props["blocks"]} == kinds and len(props["blocks"]) >= 25, name
    assert sorted(set(cases[2][3]["stored_phases"])) == list(range(8))


@pytest.mark.parametrize("name", [c[0] for c in C.reject_cases()])
def test_zlib_refuses(name):
    _, stream, plain, _ = next(c for c in C.reject_cases() if c[0] == name)
    assert plain is None
    with pytest.raises(zlib.error):
        zlib.decompress(stream)


def test_every_listed_refusal_is_there():
    assert {c[0] for c in C.reject_cases()} == {
        "ll-incomplete", "ll-oversubscribed", "dist-incomplete", "dist-oversubscribed", "clc-incomplete", "clc-oversubscribed", "hlit-30", "hlit-31",
        "hdist-30", "hdist-31", "repeat-first", "repeat-overshoots", "no-end-of-block", "match-without-dist-code", "one-dist-code-unused-bit",
        "fixed-symbol-286", "fixed-dist-symbol-30", "fixed-dist-past-start", "dynamic-dist-past-start", "stored-bad-nlen", "stored-past-end",
        "block-type-3", "no-end-of-block-code-in-stream", "cinfo-8"}
    assert all(len(c[1]) <= 64 for c in C.reject_cases())


def test_random_streams():
    cases = C.random_cases()
    assert len(cases) == 200 and cases == C.random_cases.__wrapped__()            # seeded: the same streams on every run
    kinds = set()
    for name, stream, plain, props in cases:
        assert inflates_to(stream, plain), name
        assert len(plain) <= 8192 and 1 <= len(props["blocks"]) <= 4, name
        kinds |= {k for k, _ in props["blocks"]}
    assert kinds == {"stored", "fixed", "dynamic"}


def test_the_writer_s_parts():
    assert C.canon(C.FIXED_LL)[256] == (0, 7) and C.canon(C.FIXED_LL)[0] == (0b00001100, 8) and C.canon(C.FIXED_LL)[144] == (0b000010011, 9)   # RFC 1951, 3.2.6
    assert C.len_code(258) == (285, 0, 0) and C.len_code(258, True) == (284, 5, 31) and C.len_code(257) == (284, 5, 30) and C.len_code(3) == (257, 0, 0)
    assert C.dist_code(32768) == (29, 13, 8191) and C.dist_code(1) == (0, 0, 0) and C.dist_code(24577) == (29, 13, 0)
    assert C.play([1, 2, (5, 2), (3, 6)]) == bytes([1, 2, 1, 2, 1, 2, 1, 2, 1, 2])
    assert C.cl_symbols([5] * 8 + [0] * 150 + [0, 3, 3], "greedy") == [(5, 0, 0), (16, 2, 3), (5, 0, 0), (18, 7, 127), (18, 7, 2), (3, 0, 0), (3, 0, 0)]
    w = C.BitWriter()
    w.put(1, 1); w.put(0b10, 2); w.put(0x1F, 5); w.put(1, 1)
    w.align()
    assert bytes(w.out) == bytes([0b11111101, 1])


# ---- what the device test leans on
@pytest.mark.parametrize("name", ["deep-greedy", "deep-norepeat", "deep-258-as-284+31", "window-256-dist-32768"])
def test_deep_code(name):
    _, stream, plain, p = by_name(name)
    ll, dl = C.deep_codes()
    assert len(ll) == 286 and len(dl) == 30 and C.kraft(ll) == 32768 and C.kraft(dl) == 32768
    assert p["lprefix"] >= 100 and p["dprefix"] >= 8 and p["lmax"] == 15 and p["dmax"] == 15 and {12, 13, 14, 15} <= set(p["llens"])
    assert p["hclen"] == 19
    assert (p["cross"] == 16) == (name != "deep-norepeat")             # a run of symbol 16 over the last literal / length and the first distance lengths
    toks = C.deep_tokens()
    assert {t for t in toks if type(t) is int} == set(range(256))
    lens, dists = {t[0] for t in toks if type(t) is tuple}, {t[1] for t in toks if type(t) is tuple}
    assert set(C.LBASE) | set(C.LTOP) <= lens and set(C.DBASE) | set(C.DTOP) <= dists and 258 in lens and 32768 in dists
    assert 32768 < len(plain) < 34 * 1024
    assert (stream[0] == 0x08) == (name == "window-256-dist-32768") and int.from_bytes(stream[:2], "big") % 31 == 0
    assert (by_name("deep-258-as-284+31")[1] != by_name("deep-greedy")[1]) and by_name("deep-258-as-284+31")[2] == by_name("deep-greedy")[2]


def test_single_code_sets_and_code_length_codes():
    assert by_name("eob-only")[2] == b"" and by_name("eob-only")[3]["cross"] == 17 and by_name("no-dist-code")[3]["cross"] == 18
    assert by_name("eob-only")[3]["first"] == 18
    assert by_name("hclen-5")[3]["hclen"] == 5 and by_name("clc-7-bits")[3]["hclen"] == 12
    for name in ("one-dist-code", "one-dist-code-sym3", "two-dist-codes", "no-dist-code", "hclen-5", "clc-7-bits"):
        assert len(by_name(name)[2]) >= 1500, name


def test_literal_runs():
    for n in (C.LL_SPLIT - 1, C.LL_SPLIT, C.LL_SPLIT + 1):
        plain = by_name("ll-split-%d" % n)[2]
        assert len(plain) == n + 5 and plain[n - 1] == plain[n] == plain[n + 2] and plain[-2:] == b"\x07\x08"
    m = by_name("ll-split-mixed")
    assert len(m[2]) == 2 * 65535 + 6 and m[2][-6:] == bytes([1, 2, 2, 2, 2, 9]) and [k for k, _ in m[3]["blocks"]] == ["stored", "stored", "dynamic"]
    assert len(by_name("piece-131072-literals")[2]) == C.BLK and len(by_name("piece-131069+3")[2]) == C.BLK
    assert len(by_name("stored-65535")[2]) == 65535


def test_stored_phases_and_reseats():
    assert [by_name("stored-phase-%d" % k)[3]["phase"] for k in range(8)] == list(range(8))
    for k in range(8):
        _, stream, plain, p = by_name("stored-phase-%d" % k)
        assert [kind for kind, _ in p["blocks"]] == ["fixed", "stored", "stored"] and p["blocks"][1][1] % 8 == k and plain.endswith(b"end")
    assert [by_name("reseat-d%d" % d)[3]["data_end"] for d in (0, 1, 2, 3, 4, 1023)] == [1024, 1023, 1022, 1021, 1020, 1025]
    for d in (0, 1, 2, 3, 4, 1023):
        p = by_name("reseat-d%d" % d)[3]
        assert p["blocks"][1] == ("dynamic", 8 * p["data_end"]) and (p["data_end"] + d) % 1024 == 0
    for edge in (1024, 2048):
        p = by_name("big-header-at-ring-edge-%d" % edge)[3]
        assert edge - 8 <= p["start_bit"] // 8 < edge and p["header_bits"] >= 8 * 270 and p["hclen"] == 19 and p["cross"] == 0


def test_piece_layouts():
    for name, nmark in (("own-layout-3-pieces", 2), ("chance-marker", 3)):
        _, stream, plain, p = by_name(name)
        assert p["pieces"] == [C.BLK] * 3 and len(plain) == 3 * C.BLK and C.markers(stream) == nmark
        # the pieces as the decoder cuts them: behind every empty stored block the output stands at a multiple of the piece size
        d, cuts, pos = zlib.decompressobj(), [], 0
        for at in (i + 4 for i in range(len(stream)) if stream[i:i + 4] == b"\x00\x00\xff\xff"):
            pos += len(d.decompress(stream[len(cuts) and cuts[-1][0]:at]))
            cuts.append((at, pos))
        sizes = [c[1] for c in cuts]
        assert sizes == ([C.BLK, 2 * C.BLK] if nmark == 2 else [C.BLK, C.BLK + 100 + 40000 + 4, 2 * C.BLK]), sizes
    assert C.markers(b"\x00\x00\xff\xff\x00\x00\xff\xff\x00") == 2
