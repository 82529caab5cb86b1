"""The .xz encoder core (csrc/xz_enc_core.h: a chunk's sequences -> LZMA decisions -> the range encoder; chunk and block headers, Index, footer -- the
code the device kernels run) on the CPU, over the sequences of the oracle's LZ model at 64 KiB and 8 KiB blocks: liblzma decodes every stream, and so
does xz_core.h's decoder.  Built with g++ alone by tests/xz_enc_core/Makefile, once as a shared object that xz_enc_cases loads, once as a stand-alone
program under -fsanitize=address,undefined that runs the same cases with buffers of exactly the bounds (never loaded into this process)."""
import ctypes
import lzma
import os
import subprocess

import pytest

import xz_enc_cases as E

NAMES = [n for n, _ in E.inputs()]


@pytest.mark.parametrize("blk_log", [16, 13])
@pytest.mark.parametrize("name", NAMES)
def test_stream(name, blk_log):
    data = dict(E.inputs())[name]
    stream = E.cpu_stream(name, 6, blk_log)
    assert lzma.decompress(stream, format=lzma.FORMAT_XZ) == data
    lib = E.core()
    buf, got = ctypes.create_string_buffer(max(len(data), 1)), ctypes.c_size_t()
    assert lib.xze_host_decode(stream, len(stream), buf, len(data), ctypes.byref(got)) == 0
    assert buf.raw[:got.value] == data
    recs, check = E.index_records(stream)
    assert len(recs) == (len(data) + E.SEG - 1) // E.SEG
    assert [u for _, u in recs] == [min(E.SEG, len(data) - s) for s in range(0, len(data), E.SEG)]
    assert check == lzma.CHECK_CRC64
    assert len(stream) <= lib.xze_host_bound(len(data))
    if not data:
        assert len(stream) == 32


def _controls(stream):
    """the LZMA2 control bytes of a stream's first block"""
    pos, out = 24, []
    while True:
        c = stream[pos]
        out.append(c)
        if c == 0:
            return out
        if c < 0x80:
            pos += 3 + ((stream[pos + 1] << 8) | stream[pos + 2]) + 1
        else:
            assert c >= 0xC0 and stream[pos + 5] == 93                  # state reset + properties lc 3, lp 0, pb 2 on every LZMA chunk
            pos += 6 + ((stream[pos + 3] << 8) | stream[pos + 4]) + 1


def test_chunk_kinds():
    """what the cases are there for: stored chunks of both kinds, LZMA chunks of both kinds, both in one block; a block header without sizes, 1 MiB dictionary"""
    assert _controls(E.cpu_stream("random70000"))[:3] == [0x01, 0x02, 0x00]
    mixed = _controls(E.cpu_stream("random_then_text"))
    assert mixed[0] == 0x01 and 0x02 in mixed and 0xC0 in mixed
    assert _controls(E.cpu_stream("text65536")) == [0xE0, 0x00]
    assert _controls(E.cpu_stream("text65537")) == [0xE0, 0x02, 0x00]   # (one byte: stored)
    assert _controls(E.cpu_stream("text65536", 6, 13)) == [0xE0] + [0xC0] * 7 + [0x00]
    assert E.cpu_stream("text5k")[12:20] == bytes([2, 0, 0x21, 1, 16, 0, 0, 0])
    lens = [(q >> 20) & 0x3FFFF for q in E.model_sequences("zeros2m1", 6, 16)[1]]
    assert max(lens) == 273                                              # (the LZ stage's matches end at LZMA's longest length)


def _no_chunk_beyond_stored(stream):
    """no chunk takes more than its stored form (3 + its input), which is what the bound counts; returns the chunks"""
    cs = E.chunks(stream)
    for control, usize, cost in cs:
        assert cost <= 3 + usize and (control >= 0x80) == (cost < 3 + usize), (hex(control), usize, cost)
    return cs


@pytest.mark.parametrize("blk_log", [16, 13])
@pytest.mark.parametrize("name", NAMES)
def test_no_chunk_costs_more_than_stored(name, blk_log):
    _no_chunk_beyond_stored(E.cpu_stream(name, 6, blk_log))


def test_near_stored_is_at_the_edge():
    """what "near_stored" is there for, over the LZ model's parse at 8 KiB blocks: stored chunks, LZMA chunks, and LZMA chunks within 3 bytes of their
    stored form -- the ones that cost MORE than it if the 6-byte header is not counted against the 3-byte one"""
    cs = _no_chunk_beyond_stored(E.cpu_stream("near_stored", 6, 13))
    assert len(cs) == 128
    assert sum(1 for c, _, _ in cs if c < 0x80) >= 16 and sum(1 for c, _, _ in cs if c >= 0x80) >= 16
    assert any(c >= 0x80 and cost >= u for c, u, cost in cs)


def test_literal_parse_at_the_edge():
    """all-literal parses whose LZMA forms pass through every size around the chunk's own, 8 KiB (128 equal chunks in one block: a byte too many per chunk
    leaves the bound) and 64 KiB: every stream fits its bound, no chunk costs more than stored, both kinds occur and the sweep meets the last LZMA size"""
    for size in (8192, 65536):
        kinds, closest = set(), 0
        for data, blk_log in E.at_the_edge():
            if 1 << blk_log != size:
                continue
            stream = E.literal_stream(data, blk_log)
            assert stream, "the stream did not fit xze_bound"
            assert len(stream) <= E.core().xze_host_bound(len(data))
            assert lzma.decompress(stream, format=lzma.FORMAT_XZ) == data
            for control, usize, cost in _no_chunk_beyond_stored(stream):
                kinds.add(control >= 0x80)
                if control >= 0x80:
                    closest = max(closest, cost - usize)
        assert kinds == {False, True} and closest == 2, (size, kinds, closest)   # (6 + out with out + 3 < clen: clen + 2 at most)


def test_levels_round_trip():
    data = dict(E.inputs())["text1m12345"]
    sizes = [len(E.cpu_stream("text1m12345", lv)) for lv in (0, 3, 6, 9)]
    for lv in (0, 3, 6, 9):
        assert lzma.decompress(E.cpu_stream("text1m12345", lv)) == data
    assert sizes[0] > sizes[2]                                           # (the fast set finds less than the high set)


def _decodes(stream, data):
    """liblzma and xz_core.h's decoder give the data back; the stream fits the bound and no chunk of it costs more than stored"""
    lib = E.core()
    assert stream, "the stream did not fit xze_bound"
    assert len(stream) <= lib.xze_host_bound(len(data))
    assert lzma.decompress(stream, format=lzma.FORMAT_XZ) == data
    buf, got = ctypes.create_string_buffer(max(len(data), 1)), ctypes.c_size_t()
    assert lib.xze_host_decode(stream, len(stream), buf, len(data), ctypes.byref(got)) == 0
    assert buf.raw[:got.value] == data
    _no_chunk_beyond_stored(stream)


def test_hand_made_parses():
    """parses the LZ stage never writes -- every length around the 273 cap and its multiples, distances of every slot, a pool of four distances -- and
    parses with one wrong sequence: valid streams all the same"""
    for data, blk_log, counts, packed in E.hand_made_cases():
        _decodes(E.stream_of_parse(data, blk_log, counts, packed), data)
    for what, data, blk_log, counts, packed, _, _ in E.broken_sequence_cases():
        _decodes(E.stream_of_parse(data, blk_log, counts, packed), data)


def test_census():
    """What the inputs are there for, each at least once, by the event decoder of xz_enc_cases (which rebuilds the bytes as well).  As measured:
    rep_cycle (level 6, 64 KiB blocks): rep0 121, rep1 450, rep2 479, rep3 325, replen_low 188, replen_mid 377, replen_high 810, lit_matched 2 501;
    far (level 9): slot39 301 (slot38 0), len273 299, rep0 521;
    the 21 hand-made parses together: every key but shortrep, the rarest slot15 1, slot6 2, slot9 3, slot11 3, slot10 4 -- rep0 33 652, rep1 5 980, rep2 5 141,
    rep3 4 375, lenstate0 2 184, lenstate1 2 210, lenstate2 2 151, slot0 .. slot3 1 228 / 1 368 / 1 239 / 1 502, slot38 806, slot39 481, len273 27 228, stored 4;
    the six broken parses: 1 527, 1 869, 1 735, 1 602, 1 924 and 8 192 literals between the wrong sequence and its chunk's end, nothing else."""
    d = dict(E.inputs())["rep_cycle"]
    ev = E.events(E.cpu_stream("rep_cycle", 6, 16))
    assert ev.data == d
    for k in ("rep0", "rep1", "rep2", "rep3", "replen_low", "replen_mid", "replen_high", "lit_matched"):
        assert ev[k] >= 1, (k, dict(ev))
    ev = E.events(E.cpu_stream_of(E.far(), 9, 16))
    assert ev.data == E.far()
    assert ev["slot38"] + ev["slot39"] >= 1 and ev["len273"] >= 1, dict(ev)
    total = E.Events()
    for data, blk_log, counts, packed in E.hand_made_cases():
        ev = E.events(E.stream_of_parse(data, blk_log, counts, packed))
        assert ev.data == data
        total.update(ev)
    assert sorted(total) == sorted(k for k in E.EVENT_KEYS if k != "shortrep") and all(total[k] >= 1 for k in total), dict(total)
    assert total["shortrep"] == 0                                       # (the coder never writes one)
    for what, data, blk_log, counts, packed, pos, end in E.broken_sequence_cases():
        ev = E.events(E.stream_of_parse(data, blk_log, counts, packed))
        assert ev.data == data
        inside = [(at, kind) for at, kind, _ in ev.trace if pos <= at < end]
        assert inside == [(at, "lit") for at in range(pos, end)], what   # (an LZMA chunk, so every byte of it has its event)
        assert any(kind != "lit" for at, kind, _ in ev.trace if end <= at < end + 8192), what      # (... and the next chunk is parsed as given)


def test_split_above_273():
    """single matches of 274, 275, 546, 547, 63 579 and 65 000 bytes: pieces of 273 with a rest of 2 .. 273, or of 272 + 2 where 273 would leave one byte
    -- the first piece a match at the sequence's distance, the others repeats of it (rep0) --, and each sequence's pieces add up to its length"""
    data, blk_log, counts, packed, matches = E.split_case()
    stream = E.stream_of_parse(data, blk_log, counts, packed)
    _decodes(stream, data)
    ev = E.events(stream)
    assert ev.data == data
    pieces = {}
    for at, kind, n in ev.trace:
        if kind != "lit":
            start = max(p for p, _ in matches if p <= at)
            pieces.setdefault(start, []).append((at, kind, n))
    assert ev["shortrep"] == 0 and sorted(pieces) == [p for p, _ in matches]
    for start, ml in matches:
        got = pieces[start]
        want = [273] * (ml // 273) + ([ml % 273] if ml % 273 else [])
        if want[-1] == 1:
            want[-2:] = [272, 2]
        assert [n for _, _, n in got] == want, (ml, got[-3:])
        assert [at for at, _, _ in got] == [start + sum(want[:i]) for i in range(len(want))] and sum(n for _, _, n in got) == ml
        assert [kind for _, kind, _ in got] == ["match"] + ["rep0"] * (len(want) - 1), ml
        assert min(n for _, _, n in got) >= 2
    assert [n for _, _, n in pieces[matches[0][0]]] == [272, 2] and [n for _, _, n in pieces[matches[1][0]]] == [273, 2]
    assert [n for _, _, n in pieces[matches[3][0]]] == [273, 272, 2]


def test_sanitizer_program(tmp_path):
    out = E.built()
    lines = []
    for name in NAMES:
        for blk_log in (16, 13):
            p = str(tmp_path / ("%s_%d.case" % (name, blk_log)))
            E.case_file(p, name, 6, blk_log)
            lines.append(p)
    for i, (data, blk_log) in enumerate(E.at_the_edge()):
        p = str(tmp_path / ("edge_%d.case" % i))
        E.literal_case_file(p, data, blk_log)
        lines.append(p)
    parses = [c for c in E.hand_made_cases()] + [c[1:5] for c in E.broken_sequence_cases()] + [E.split_case()[:4]]
    parses.append((E.far(), 16) + tuple(E.model_sequences_of(E.far(), 9, 16)))
    for i, (data, blk_log, counts, packed) in enumerate(parses):
        p = str(tmp_path / ("parse_%d.case" % i))
        E.parse_case_file(p, data, blk_log, counts, packed)
        lines.append(p)
    man = tmp_path / "manifest"
    man.write_text("\n".join(lines) + "\n")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([os.path.join(out, "xz_enc_host_san"), str(man)], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "%d cases, 0 bad" % len(lines) in r.stdout
