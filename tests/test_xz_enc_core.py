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
    man =tmp_path / "manifest"
    man.write_text("\n".join(lines) + "\n")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([os.path.join(out, "xz_enc_host_san"), str(man)], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "%d cases, 0 bad" % len(lines) in r.stdout
