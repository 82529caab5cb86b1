"""The zstd decoder's header walk and literal scratch count in 64 bits (a single frame takes the parallel path whatever its compressed size and however many
literals it carries: tests/test_gpu_full_size_zstd_4gib_compressed.py has the sizes at which the old 32-bit counters wrapped).  Here, at small sizes, what that
change touches:
  * frames read from and decoded to offsets above 4 GiB of their buffers,
  * the routing: with the parallel executor off (zexec_par_min_mib = 0) and the one-workgroup kernel refused (zdec_fallback_max_mib = 1), and with the default
    options, frames of 1, 9 and 70 MiB of content in the shapes the suite uses elsewhere decode to what oracle/zstd_dec.c reads.
Positions were widened, not re-based: the wave-per-block parse starts at its own block (a 64-bit position from the header walk) and counts 32 bits from there,
which a block's 128 KiB never exceed, so there is no re-base distance to shrink and no test hook for one."""
import struct

import pytest

pytestmark = pytest.mark.gpu

MIB, GIB = 1 << 20, 1 << 30


def _need_hbm(torch, gib):
    free, _ = torch.cuda.mem_get_info()
    assert free >= gib * GIB, f"the case needs {gib} GiB of free HBM, found {free / GIB:.0f} GiB: an MI355X has 288 GB"


def test_frames_at_offsets_above_4gib(big_ctx, pna, codec):
    """A 3 MiB libzstd frame and a 3 MiB entry of this library (three frames of the 1 MiB grid, and the same as ONE frame) behind 4 GiB of a source
    allocation, decoded behind 4 GiB of a destination allocation: ZFrame::src_off / dst_off, ZBlock::body and the literal scratch position are absolute."""
    import numpy as np
    import torch
    if codec.system_libzstd() is None:
        pytest.skip("system libzstd (the writer of the foreign frame) is absent")
    _need_hbm(torch, 24)
    ctx = big_ctx
    raws = [codec.corpus_file(0, 8800, 3 * MIB), codec.corpus_file(1, 8801, 3 * MIB), codec.corpus_file(2, 8802, 3 * MIB)]
    grid = ctx.compress_batch([raws[1]])[0]
    ctx.set_option("single_frame", 1)
    one = ctx.compress_batch([raws[2]])[0]
    ctx.set_option("single_frame", 0)
    payloads = [codec.libzstd_compress(raws[0], 3), grid, one]
    ctx.set_option("zdec_fallback_max_mib", 1)
    span = 4 * GIB + 32 * MIB
    src = torch.empty(span, dtype=torch.uint8, device="cuda")          # (untouched but for the payloads)
    dst = torch.empty(span, dtype=torch.uint8, device="cuda")
    so = [4 * GIB + 4099, 4 * GIB + 8 * MIB + 1, 4 * GIB + 16 * MIB + 7]
    do = [4 * GIB + 123, 4 * GIB + 5 * MIB + 3, 4 * GIB + 11 * MIB + 64]
    for p, o in zip(payloads, so):
        src[o:o + len(p)] = torch.from_numpy(np.frombuffer(p, dtype=np.uint8).copy()).cuda()
    dst[4 * GIB:].zero_()
    ctx.decompress_batch_device(src.data_ptr(), so, [len(p) for p in payloads], dst.data_ptr(), do, [len(r) for r in raws])
    for r, o in zip(raws, do):
        assert dst[o:o + len(r)].cpu().numpy().tobytes() == r
    # ... and through the parallel executor (a frame of 3 MiB takes it with the threshold lowered)
    ctx.set_option("zexec_par_min_mib", 1)
    dst[4 * GIB:].zero_()
    ctx.decompress_batch_device(src.data_ptr(), so, [len(p) for p in payloads], dst.data_ptr(), do, [len(r) for r in raws])
    for r, o in zip(raws, do):
        assert dst[o:o + len(r)].cpu().numpy().tobytes() == r


def _skippable(k):
    body = bytes((7 * i + k) & 0xFF for i in range((0, 1, 7, 300)[k % 4]))
    return struct.pack("<II", 0x184D2A50 + (k % 16), len(body)) + body


def _frame(codec, data, level, fcs, chk):
    if fcs and not chk:
        return codec.libzstd_compress(data, level)
    return codec.libzstd_compress_checksum(data, level, extra=(() if fcs else ((200, 0),)) + (() if chk else ((201, 0),)))


@pytest.fixture(scope="module")
def routing_ctxs(pna):
    import torch  # noqa: F401  (shares its HIP runtime with the extension)
    gated, plain = pna.Context(0), pna.Context(0)
    gated.set_option("zexec_par_min_mib", 0)
    gated.set_option("zdec_fallback_max_mib", 1)
    yield gated, plain
    gated.close()
    plain.close()


@pytest.mark.parametrize("mib", [1, 9, 70])
def test_routing_of_ordinary_frames(routing_ctxs, pna, codec, mib):
    """Multi-frame grid, single frame (this library's and libzstd's), foreign concatenations, skippable frames, frames with checksum and without content
    size: every payload in one batch, with the parallel executor off and the one-workgroup kernel refused, then with the default options."""
    gated, plain = routing_ctxs
    n = mib * MIB
    raw = b"".join(codec.corpus_file(i % 2, 8900 + 100 * mib + i, MIB) for i in range(mib))
    payloads = {"grid": plain.compress_batch([raw])[0]}
    plain.set_option("single_frame", 1)
    payloads["single"] = plain.compress_batch([raw], level=1)[0]
    plain.set_option("single_frame", 0)
    assert payloads["single"][:4] == bytes.fromhex("28b52ffd")
    if codec.system_libzstd() is not None:
        payloads["foreign single, checksum"] = _frame(codec, raw, 1, True, True)
        cuts = sorted({0, n} | {min(n, c) for c in (300000, MIB + 1, 3 * MIB, 3 * MIB + 17, n // 2, n - 5)})
        parts = []
        for k, (a, b) in enumerate(zip(cuts, cuts[1:])):
            if k % 2 == 0:
                parts.append(_skippable(k))
            parts.append(_frame(codec, raw[a:b], (1, 3, 5)[k % 3], k % 3 != 1, k % 2 == 1))
        parts.append(_skippable(5))
        payloads["foreign concatenation"] = b"".join(parts)
        payloads["foreign single, no content size"] = _frame(codec, raw, 3, False, False)
    first = next(iter(payloads))
    want = codec.zstd_decompress(payloads[first], n)                    # the reference decoder, once: every payload holds the same bytes
    assert want == raw
    names, bodies = list(payloads), list(payloads.values())
    for ctx, what in ((gated, "executor off, fallback refused"), (plain, "default options")):
        got = ctx.decompress_batch(bodies, [n] * len(bodies))
        for name, g in zip(names, got):
            assert g == want, (what, name)
