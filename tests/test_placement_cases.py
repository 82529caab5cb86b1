"""The case list of tests/test_gpu_decode_placement.py, checked without a device: every foreign stream decodes to its plain bytes with an independent CPU
decoder, every layout's streams and rooms are disjoint and inside their buffers, the residue sweep reaches every residue for every entry.  A broken case
list cannot make the device tests pass."""
import zlib

import pytest

import placement_cases as P


def test_plain_inputs():
    names = [n for n, _ in P.plains()]
    assert len(set(names)) == len(names)
    lens = [len(d) for _, d in P.plains()]
    assert lens[:len(P.TEXT_LENGTHS)] == list(P.TEXT_LENGTHS)
    assert lens[len(P.TEXT_LENGTHS):] == [70001, 50003, 33331, 300001, P.MIB + 4099]
    assert P.plain("zeros70001") == bytes(70001)
    per = P.plain("period7")
    assert per[7:] == per[:-7] and len(set(per[:7])) > 1


@pytest.mark.parametrize("level", [1, 3, 19])
@pytest.mark.parametrize("checksum", [False, True])
def test_libzstd_frames_decode(codec, level, checksum):
    if not P.have_libzstd():
        pytest.skip("system libzstd (the writer of the foreign frames) is absent")
    for name, s, d in P.zstd_foreign(level, checksum):
        assert P.zstd_cpu_decode(s, len(d)) == d, name
        assert s[:4] == bytes.fromhex("28b52ffd") and bool(s[4] & 4) == checksum, name     # Frame_Header_Descriptor bit 2: Content_Checksum_flag


def test_zstd_frame_list_decodes(codec):
    if not P.have_libzstd():
        pytest.skip("system libzstd (the writer of the foreign frames) is absent")
    name, s, d = P.zstd_frame_list()
    assert P.zstd_cpu_decode(s, len(d)) == d
    assert s.count(bytes.fromhex("28b52ffd")) >= 3 and bytes.fromhex("532a4d18") in s and bytes.fromhex("522a4d18") in s


@pytest.mark.parametrize("writer", sorted(P.DEFLATE_WRITERS))
def test_zlib_streams_decode(codec, writer):
    for name, s, d in P.deflate_foreign(writer):
        assert zlib.decompress(s) == d, name
    if writer == "stored":
        assert all(len(s) >= len(d) for _, s, d in P.deflate_foreign(writer))
    if writer == "w9":
        assert all(s[0] >> 4 == 1 for _, s, _ in P.deflate_foreign(writer))                 # CINFO 1: a window of 512 bytes


def test_large_zlib_stream(codec):
    name, s, d = P.deflate_large()
    assert zlib.decompress(s) == d and len(d) == P.MIB + P.MIB // 2
    assert len(s) >= 128 << 10                                                            # 8 x SPEC_CHUNK: what the chunk decoder requires


def test_xz_streams_decode(codec):
    names = set()
    for name, s, d in P.xz_streams():
        assert P.xz_cpu_decode(s) == d, name
        assert len(d) <= P.XZ_MAX
        names.add(name)
    assert len(names) == len(P.xz_streams())
    checks = {name: s[7] for name, s, _ in P.xz_streams()}                                 # stream flags: the check type
    assert checks["text300001_none"] == 0 and checks["text300001_crc32"] == 1 and checks["text300001_crc64"] == 4


def test_damage_is_refused_by_the_cpu_decoders(codec):
    t = P.plain("text65537")
    assert P.deflate_cpu_refuses(P.flip_middle(dict((n, s) for n, s, _ in P.deflate_foreign("z6"))["text65537_z6"]))
    from xz_cases import liblzma_refuses
    assert liblzma_refuses(P.flip_middle(dict((n, s) for n, s, _ in P.xz_streams())["text65537_p6"]))
    if P.have_libzstd():
        assert P.zstd_cpu_refuses(P.flip_middle(dict((n, s) for n, s, _ in P.zstd_foreign(3, True))["text65537_l3_chk"]), len(t))


def _case_lengths():
    """(src_len, raw_len) of batches shaped like the device test's: every plain input once (streams a little shorter or longer than their content)"""
    raw = [len(d) for _, d in P.plains()]
    return [len(s) for _, s, _ in P.deflate_foreign("z6")], raw


def _disjoint_inside(off, length, size, front):
    spans = sorted((a, a + n) for a, n in zip(off, length) if n)
    assert all(a >= front and b <= size for a, b in spans)
    assert all(x[1] <= y[0] for x, y in zip(spans, spans[1:]))
    assert all(front <= a <= size for a in off)                                            # (empty ranges too lie inside)


def _check_layout(L):
    _disjoint_inside(L.src_off, L.src_len, L.src_size - P.SRC_SLACK, P.GUARD)
    _disjoint_inside(L.dst_off, L.raw_len, L.dst_size - P.GUARD, P.GUARD)
    assert L.src_size == max(a + n for a, n in zip(L.src_off, L.src_len)) + P.SRC_SLACK      # exactly the documented slack behind the last stream
    assert L.dst_size == max(a + n for a, n in zip(L.dst_off, L.raw_len)) + P.GUARD
    # the guard ranges are exactly the complement of the rooms
    covered = sum(b - a for a, b in L.guards) + sum(L.raw_len)
    assert covered == L.dst_size and L.guards[0][0] == 0 and L.guards[0][1] >= P.GUARD and L.guards[-1] == (L.dst_size - P.GUARD, L.dst_size)
    assert sum(b - a for a, b in L.src_gaps) + sum(L.src_len) == L.src_size and L.src_gaps[-1] == (L.src_size - P.SRC_SLACK, L.src_size)


def test_layouts_are_disjoint_and_inside():
    sl, rl = _case_lengths()
    for rs, rd in P.RESIDUES:
        for make in (P.tight, P.gapped):
            L = make(sl, rl, rs, rd)
            _check_layout(L)
            assert L.src_off[0] % 16 == rs and L.dst_off[0] % 16 == rd
        L = P.permuted(sl, rl, rd)
        _check_layout(L)
        assert any(a > b for a, b in zip(L.dst_off, L.dst_off[1:]))                        # not monotonic
    T = P.tight(sl, rl, 1, 5)
    assert all(T.dst_off[i + 1] == T.dst_off[i] + rl[i] for i in range(len(rl) - 1))       # rooms touch
    assert all(T.src_off[i + 1] == T.src_off[i] + sl[i] for i in range(len(sl) - 1))
    assert rl[0] == 0 and T.dst_off[0] == T.dst_off[1]                                     # the empty entry shares its offset with its successor
    G = P.gapped(sl, rl, 1, 5)
    assert [G.dst_off[i + 1] - G.dst_off[i] - rl[i] for i in range(len(rl) - 1)] == [1 + (7 * k) % 15 for k in range(1, len(rl))]
    assert sorted(P.permutation(len(rl))) == list(range(len(rl))) and P.permutation(len(rl)) != list(range(len(rl)))


def test_residue_sweep_reaches_every_residue_for_every_length():
    sl, rl = _case_lengths()
    for make in (P.tight, P.gapped):
        dres = [set() for _ in rl]
        sres = [set() for _ in sl]
        for rs, rd in P.RESIDUES:
            L = make(sl, rl, rs, rd)
            for i in range(len(rl)):
                dres[i].add(L.dst_off[i] % 16)
                sres[i].add(L.src_off[i] % 4)
        assert all(r == set(range(16)) for r in dres) and all(r == set(range(4)) for r in sres)
    assert len(set(P.FEW_RESIDUES)) == 5 and all(0 <= rs < 16 and 0 <= rd < 16 for rs, rd in P.FEW_RESIDUES)
