"""`pna diff` at full size: an entry beyond 4 GiB that differs only behind 2^32 (the pieces' 64-bit base), and the 10 000 x 1 MiB headline archive
compared with its own inputs."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MIB = 1 << 20


def test_difference_beyond_4gib(big_ctx, pna, pf, codec):
    """one stored entry of 4 GiB + 64 KiB, the file differing only at offset 2^32 + 5 -- and, in a second pass, only in its last byte"""
    n = (4 << 30) + (64 << 10)
    base = np.frombuffer(codec.corpus_file(0, 11, 64 * MIB), np.uint8)
    raw = np.tile(base, n // len(base) + 1)[:n]
    step = 1 << 30                                                   # FDAT chunks of 1 GiB (a chunk's length is a 32-bit field)
    arc = bytearray(pf.write_archive_header())
    arc += pf.write_chunk(b"FHED", pf.file_entry_header(0, "big/one")) + pf.write_chunk(b"fSIZ", pf.fsiz_bytes(n))
    for o in range(0, n, step):
        arc += pf.write_chunk(b"FDAT", raw[o:o + step].tobytes())
    arc += pf.write_chunk(b"FEND") + pf.finalize_archive()
    arc = bytes(arc)
    other = raw.copy()
    for off in ((1 << 32) + 5, n - 1):
        other[off] ^= 0x21
        ne = np.flatnonzero(raw[off - 4096:off + 1] != other[off - 4096:off + 1])
        assert len(ne) == 1 and off - 4096 + int(ne[0]) == off
        recs, s = pna.diff_archive(big_ctx, arc, lambda i, p, k, st: (pna.DIFF_FS_FILE, (other.ctypes.data, n)))
        assert [(r.name, r.status, r.first_diff, r.size) for r in recs] == [("big/one", pna.DIFF_CONTENTS_DIFFER, off, n)], off
        other[off] ^= 0x21
    recs, s = pna.diff_archive(big_ctx, arc, lambda i, p, k, st: (pna.DIFF_FS_FILE, (other.ctypes.data, n)))
    assert [(r.status, r.first_diff) for r in recs] == [(pna.DIFF_SAME, None)] and pna.diff_stats(big_ctx)[1] == n


def test_headline_archive_equals_its_inputs(big_ctx, pna, codec):
    """10 000 x 1 MiB zstd-3 compared with the files it was made from: every entry SAME; one changed byte in three of them found"""
    n, L = 10000, MIB
    base = [codec.corpus_file(0, k, L) for k in range(64)]
    names = [f"enwik/part{i:07d}.txt" for i in range(n)]
    arc = pna.create_archive(big_ctx, names, [base[i % 64] for i in range(n)], algo=pna.ALGO_ZSTD, level=3)
    recs, s = pna.diff_archive(big_ctx, arc, lambda i, p, k, st: (pna.DIFF_FS_FILE, base[i % 64]))
    assert s["rc"] == 0 and s["same"] == n and s["total"] == n and [r.name for r in recs] == names
    assert all(r.status == pna.DIFF_SAME and r.size == L and r.first_diff is None for r in recs)
    assert pna.diff_stats(big_ctx)[:2] == (n, n * L)
    want = {0: 0, 4999: L // 2 + 1, n - 1: L - 1}
    changed = {}
    for i, off in want.items():
        b = bytearray(base[i % 64]); b[off] ^= 0x80; changed[i] = bytes(b)
    recs, s = pna.diff_archive(big_ctx, arc, lambda i, p, k, st: (pna.DIFF_FS_FILE, changed.get(i, base[i % 64])))
    assert s["differ"] == 3 and s["same"] == n - 3
    assert {i: r.first_diff for i, r in enumerate(recs) if r.status != pna.DIFF_SAME} == want
