"""`pna create --solid` with Compression::Deflate from host memory: the serialised inner entries stream through windows of solid_win_mib MiB
(pna_gpu_create_solid_archive_host; SolidArchive::add_entry feeds one ZlibEncoder, lib/src/archive/write.rs:575-580).  Every window is whole
1 MiB segments: the zlib header only in front of the stream's first segment, BFINAL and the Adler-32 trailer only on its last, the Adler-32
carried from window to window on the device.  The windowed archive must equal the one-shot device archive byte for byte."""
import zlib

import pytest

pytestmark = pytest.mark.gpu

LEVELS = (0, 1, 6, 9)


def _device_one_shot(ctx, pna, names, ents, level):
    import torch
    offs, pos = [], 0
    for e in ents:
        offs.append(pos); pos = (pos + len(e) + 15) & ~15
    src = torch.zeros(pos + 8192, dtype=torch.uint8, device="cuda")
    for o, e in zip(offs, ents):
        if e:
            src[o:o + len(e)] = torch.frombuffer(bytearray(e), dtype=torch.uint8).cuda()
    lens = [len(e) for e in ents]
    cap = pna.solid_archive_bound(pna.ALGO_DEFLATE, names, lens)
    dst = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    total = ctx.create_solid_archive_device(names, src.data_ptr(), offs, lens, dst.data_ptr(), cap, algo=pna.ALGO_DEFLATE, level=level)
    return dst[:total].cpu().numpy().tobytes()


def _plain(pf, names, ents):
    """the serialised inner stream, from the oracle's writer (STORE records, lib/src/entry.rs:888-913)"""
    return b"".join(pf.write_normal_entry(pf.file_entry_header(0, pf.sanitize_name(nm)), [e] if e else [], len(e)) for nm, e in zip(names, ents))


def _zlib_reads(pf, arc, want_plain, level):
    """zlib (the C library) over the concatenated SDAT bodies: the whole inner stream, then the stream's end -- the chained Adler-32 checked by zlib"""
    _, items = pf.read_archive(arc)
    assert len(items) == 1
    body = items[0].data
    assert body[:2] == (b"\x78\x01" if level == 0 else b"\x78\x9c")
    d = zlib.decompressobj()
    out = d.decompress(body) + d.flush()
    assert d.eof and d.unused_data == b"" and out == want_plain


def _sized_last(pf, names, ents, target):
    """the last entry's length that makes the serialised stream exactly `target` bytes long"""
    head = len(_plain(pf, names[:-1], ents[:-1]))
    ln = target - head - 100
    for _ in range(8):
        rec = len(pf.write_normal_entry(pf.file_entry_header(0, pf.sanitize_name(names[-1])), [b"x"], ln)) - 1 + ln
        if head + rec == target:
            return ln
        ln += target - head - rec
    raise AssertionError("no length fits")


def test_deflate_solid_archive_streams_through_windows(gpu_ctx, pna, pf, codec):
    big = codec.corpus_file(0, 8001, 2600000)
    checked = 0
    try:
        for win in (1, 2):
            gpu_ctx.set_option("solid_win_mib", win)
            for level in LEVELS:
                deltas = range(24) if (win == 1 and level == 6) else range(0, 24, 7)
                for delta in deltas:
                    # the first entry's record ends `delta` bytes around the 1 MiB edge: its CRC field, FEND and the next entry's FHED straddle the edge in turn
                    first = codec.corpus_file(1, 8100 + delta, (1 << 20) - 70 - delta)
                    ents = [first, b"", big, b"", codec.corpus_file(0, 8002, 4096), codec.corpus_file(1, 8003, (1 << 20) + 5)] + ([] if delta % 3 else [b""])
                    names = [f"d/{i}.bin" for i in range(len(ents))]
                    got = pna.create_archive(gpu_ctx, names, ents, algo=pna.ALGO_DEFLATE, level=level, solid=True)
                    assert got == _device_one_shot(gpu_ctx, pna, names, ents, level), (win, level, delta)
                    if delta == 7:
                        _zlib_reads(pf, got, _plain(pf, names, ents), level)
                        checked += 1
                    if delta == 14 and level in (0, 9):
                        assert [(n, d) for n, _, d in pna.extract_archive(gpu_ctx, got)] == list(zip(names, ents))
            # the stream's end: exactly on a window edge, one byte past one, and a stream of one window
            W = win << 20
            for target in (3 * W, 3 * W + 1, 700000):
                ents = [codec.corpus_file(0, 8200, 300000), b"", codec.corpus_file(1, 8201, 1 << 16)]
                names = [f"e/{i}" for i in range(len(ents))] + ["e/last"]
                ents.append(codec.corpus_file(0, 8202 + target % 7, _sized_last(pf, names, ents + [b""], target)))
                assert len(_plain(pf, names, ents)) == target
                for level in LEVELS:
                    got = pna.create_archive(gpu_ctx, names, ents, algo=pna.ALGO_DEFLATE, level=level, solid=True)
                    assert got == _device_one_shot(gpu_ctx, pna, names, ents, level), (win, target, level)
                    _zlib_reads(pf, got, _plain(pf, names, ents), level)
                    checked += 1
        gpu_ctx.set_option("solid_win_mib", 1)
        many = [codec.corpus_file(1, 8300 + i, 3000 + 37 * (i % 50)) for i in range(900)]     # many small inner entries: hundreds of chunks per window
        nm = [f"m/{i}" for i in range(len(many))]
        for level in (0, 6):
            got = pna.create_archive(gpu_ctx, nm, many, algo=pna.ALGO_DEFLATE, level=level, solid=True)
            assert got == _device_one_shot(gpu_ctx, pna, nm, many, level), level
            _zlib_reads(pf, got, _plain(pf, nm, many), level)
        assert [(n, d) for n, _, d in pna.extract_archive(gpu_ctx, got)] == list(zip(nm, many))
        assert pna.create_archive(gpu_ctx, [], [], algo=pna.ALGO_DEFLATE, solid=True) == _device_one_shot(gpu_ctx, pna, [], [], -1000)
    finally:
        gpu_ctx.set_option("solid_win_mib", 256)
    assert checked >= 16


def test_deflate_solid_windows_in_latency_mode(pna, pf, codec):
    """The library's defaults (latency mode on: small streams take small blocks and LZ units): a window is planned as the whole stream, so every
    window size gives the one-shot archive -- streams around the sizes where the block size changes with the input (32 / 64 MiB)."""
    import torch  # noqa: F401  (shares its HIP runtime with the extension)
    ctx = pna.Context(0)
    try:
        for total_mib in (3, 40, 70):
            ents = [codec.corpus_file(i % 2, 8400 + i, (1 << 20) - 1000 * i) for i in range(total_mib)] + [codec.corpus_file(0, 8499, 50000)]
            names = [f"l/{i}" for i in range(len(ents))]
            want = _device_one_shot(ctx, pna, names, ents, 6)
            for win in (1, 8):
                ctx.set_option("solid_win_mib", win)
                got = pna.create_archive(ctx, names, ents, algo=pna.ALGO_DEFLATE, level=6, solid=True)
                assert got == want, (total_mib, win)
            _zlib_reads(pf, want, _plain(pf, names, ents), 6)
    finally:
        ctx.close()
