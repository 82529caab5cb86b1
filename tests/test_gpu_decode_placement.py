"""The device decoders at any byte placement (include/pna_gpu.h, PLACEMENT at pna_gpu_decompress_batch_device): streams and rooms packed without padding at
every residue mod 16, touching, with gaps of odd sizes, in permuted order, between guard bands -- through pna_gpu_decompress_batch_device, the three open
decoders and pna_gpu_open_size_device.  tests/placement_cases.py has the inputs, the foreign writers' streams and the layouts (tests/test_placement_cases.py
checks them on the CPU); the streams of this library's own encoder are made here and checked with the CPU decoders.  What is asserted of every call:
  A1  the room of entry i holds its plain input,
  A2  every byte of the destination buffer outside the rooms (4 096 in front, 4 096 behind, every gap) still holds its fill -- 0xA5, and 0x00 in a second run,
  A3  the source buffer is bit-identical after the call,
  A4  the same with the bytes around the streams (gaps, the 15 bytes of slack behind the last one) 0x00 and 0xFF,
  A5  the permuted layout in shuffled entry order gives every entry the bytes it gets decoded alone.
Every form of the decoders is shown to have run by pna_gpu_last_decode_forms (the counters a decode call leaves there) or by the option in force."""
import ctypes
import random
import zlib

import pytest

import placement_cases as P

pytestmark = pytest.mark.gpu

FILLS = ((0xA5, 0x00), (0x00, 0xFF))                # (destination fill, fill around the streams): A2's two runs are A4's two runs


# ---- one call between guard bands
def _owner(L, names, at):
    for i, (o, n) in enumerate(zip(L.dst_off, L.raw_len)):
        if o <= at < o + n:
            return "byte %d of the room of entry %d (%s, dst_off %d = %d mod 16, %d bytes)" % (at - o, i, names[i], o, o % 16, n)
    near = min(range(len(L.dst_off)), key=lambda i: min(abs(at - L.dst_off[i]), abs(at - L.dst_off[i] - L.raw_len[i])))
    return "a guard byte, %d behind the room of entry %d (%s, dst_off %d = %d mod 16, %d bytes)" % (at - L.dst_off[near] - L.raw_len[near], near, names[near],
                                                                                             L.dst_off[near], L.dst_off[near] % 16, L.raw_len[near])


def run_call(call, items, L, dst_fill, src_fill, expect_error=None, unspecified=()):
    """One decode call over `items` [(name, stream, plain)] placed as L says: call(d_src, d_dst) does it.  Checks A1 (unless an error is expected), A2, A3;
    unspecified: ranges of the destination buffer inside rooms that may hold anything.  Returns the destination buffer's bytes (numpy)."""
    import numpy as np
    import torch
    names = [n for n, _, _ in items]
    hsrc = np.full(L.src_size, src_fill, dtype=np.uint8)
    want = np.full(L.dst_size, dst_fill, dtype=np.uint8)
    guard = np.zeros(L.dst_size, dtype=bool)                           # the layout's own guard ranges (tests/test_placement_cases.py checks them)
    for a, b in L.guards:
        guard[a:b] = True
    for (_, s, d), so, do in zip(items, L.src_off, L.dst_off):
        hsrc[so:so + len(s)] = np.frombuffer(s, dtype=np.uint8)
        want[do:do + len(d)] = np.frombuffer(d, dtype=np.uint8)
    d_src = torch.from_numpy(hsrc).cuda()
    d_dst = torch.full((L.dst_size,), dst_fill, dtype=torch.uint8, device="cuda")
    err = None
    try:
        call(d_src.data_ptr(), d_dst.data_ptr())
    except Exception as e:                                              # (PnaGpuError: judged below, after the buffers are looked at)
        err = e
    if getattr(err, "code", None) == -5:                                # PNA_E_HIP: the device has faulted; nothing more is run on it
        pytest.exit("HIP error in %s: %s" % (L.name, err), returncode=3)
    torch.cuda.synchronize()
    got = d_dst.cpu().numpy()
    bad = []                                                            # every assertion is looked at: a call may break several
    if not np.array_equal(d_src.cpu().numpy(), hsrc):
        bad.append("A3: the source buffer was written")
    outside = (got != dst_fill) & guard
    if outside.any():
        at = int(np.flatnonzero(outside)[0])
        bad.append("A2: %d bytes outside the rooms were written, the first is %s" % (int(outside.sum()), _owner(L, names, at)))
    if expect_error is not None:
        if err is None or getattr(err, "code", None) != expect_error:
            bad.append("the call did not fail with %d: %r" % (expect_error, err))
    elif err is not None:
        bad.append("the call failed: %s" % err)
    else:
        diff = got != want
        for a, b in unspecified:
            diff[a:b] = False
        if diff.any():
            at = int(np.flatnonzero(diff)[0])
            bad.append("A1: %d bytes differ from the plain input, the first is %s" % (int(diff.sum()), _owner(L, names, at)))
    assert not bad, "%s, fill %#x / %#x: %s" % (L.name, dst_fill, src_fill, "; ".join(bad))
    return got


def run_batch(ctx, algo, items, L, dst_fill, src_fill, order=None, expect_error=None, shift=(0, 0)):
    """shift: the base addresses handed to the call lie that many bytes inside the buffers (bases that are not aligned), the offsets count from there"""
    idx = list(range(len(items))) if order is None else order

    def call(d_src, d_dst):
        ctx.decompress_batch_device(d_src + shift[0], [L.src_off[i] - shift[0] for i in idx], [L.src_len[i] for i in idx],
                                    d_dst + shift[1], [L.dst_off[i] - shift[1] for i in idx], [L.raw_len[i] for i in idx], algo=algo)
    return run_call(call, items, L, dst_fill, src_fill, expect_error)


def lens(items):
    return [len(s) for _, s, _ in items], [len(d) for _, _, d in items]


def sweep(ctx, algo, items, residues, shown=None):
    """tight and gapped layouts at the given residues, both fills; shown(decode_forms): the form's indicator, looked at after every call"""
    sl, rl = lens(items)
    failed = []
    for rs, rd in residues:
        for make in (P.tight, P.gapped):
            for dst_fill, src_fill in FILLS:
                try:
                    run_batch(ctx, algo, items, make(sl, rl, rs, rd), dst_fill, src_fill)
                except AssertionError as e:                             # (the other layouts still run: where a store goes astray depends on the layout)
                    failed.append(str(e))
                    continue
                if shown:
                    shown(ctx.decode_forms())
    assert not failed, "\n".join(failed)


def alone_and_permuted(ctx, algo, items, rd=5, shown=None):
    """A5: every entry decoded alone (a stream that occurs several times: once), then all of them in the permuted layout in shuffled entry order, both
    fills: the same bytes per entry.  shown(decode_forms): the form's indicator behind the permuted calls (an entry alone may take another form: a call
    of one stream never has the 1 024 pieces of the lane-per-piece decoder)"""
    sl, rl = lens(items)
    alone = {}
    for k, it in enumerate(items):
        if it[0] in alone:
            continue
        L1 = P.tight([sl[k]], [rl[k]], (k + 1) % 4, (3 * k + 1) % 16)
        got = run_batch(ctx, algo, [it], L1, 0xA5, 0x00)
        alone[it[0]] = got[L1.dst_off[0]:L1.dst_off[0] + rl[k]].tobytes()
    L = P.permuted(sl, rl, rd)
    order = list(range(len(items)))
    random.Random(99).shuffle(order)
    for dst_fill, src_fill in FILLS:
        got = run_batch(ctx, algo, items, L, dst_fill, src_fill, order=order)
        if shown:
            shown(ctx.decode_forms())
        for k in range(len(items)):
            assert got[L.dst_off[k]:L.dst_off[k] + rl[k]].tobytes() == alone[items[k][0]], items[k][0]


# ---- the streams of this library's own encoder
@pytest.fixture(scope="module")
def own_zstd(gpu_ctx, pna, codec):
    """(grid frames, single frame) per plain input, checked with the oracle decoder (and libzstd when present)"""
    plains = P.plains()
    grid = gpu_ctx.compress_batch([d for _, d in plains])
    gpu_ctx.set_option("single_frame", 1)
    try:
        single = gpu_ctx.compress_batch([d for _, d in plains])
    finally:
        gpu_ctx.set_option("single_frame", 0)
    g = [(n + "_grid", s, d) for (n, d), s in zip(plains, grid)]
    o = [(n + "_single", s, d) for (n, d), s in zip(plains, single)]
    for name, s, d in g + o:
        assert P.zstd_cpu_decode(s, len(d)) == d, name
    assert g[-1][1].count(bytes.fromhex("28b52ffd")) >= 2 and len(g[-1][2]) > P.MIB     # two frames of the grid
    return g, o


@pytest.fixture(scope="module")
def own_deflate(gpu_ctx, pna, codec):
    plains = P.plains()
    out = gpu_ctx.compress_batch([d for _, d in plains], algo=pna.ALGO_DEFLATE)
    items = [(n + "_own", s, d) for (n, d), s in zip(plains, out)]
    for name, s, d in items:
        assert zlib.decompress(s) == d, name
    return items


@pytest.fixture(scope="module")
def zstd_default(own_zstd):
    g, o = own_zstd
    return g + o + (P.zstd_foreign(3, False) if P.have_libzstd() else [])


def _interleave(*lists):
    out = []
    for k in range(max(len(x) for x in lists)):
        out += [x[k] for x in lists if k < len(x)]
    return out


@pytest.fixture(scope="module")
def deflate_default(own_deflate):
    return _interleave(own_deflate, P.deflate_foreign("z1"), P.deflate_foreign("z6"), P.deflate_foreign("z9"))


def _pieces(items):
    return sum(max(1, (len(d) + (1 << 17) - 1) >> 17) for _, _, d in items)


# ================================================================================== zstd
@pytest.mark.parametrize("rd", range(16))
def test_zstd_default_form_every_residue(gpu_ctx, pna, zstd_default, rd):
    """wave per frame and per block: grid frames, single frames and libzstd -3 frames of every plain input in one call"""
    def shown(t):
        assert t.zstd_workgroup_frames == 0 and t.zstd_executor_frames == 0 and t.zstd_listed_entries == 0   # nothing left to the one-workgroup kernel, the executor or the frame list
    sweep(gpu_ctx, pna.ALGO_ZSTD, zstd_default, [(rd % 4, rd)], shown)


def test_zstd_default_form_alone_and_permuted(gpu_ctx, pna, zstd_default):
    alone_and_permuted(gpu_ctx, pna.ALGO_ZSTD, zstd_default)


def test_zstd_one_workgroup_per_frame(gpu_ctx, pna, zstd_default):
    """zdec_serial = 1: every frame through k_zdec, the one-workgroup kernel with its own literal slots and copies"""
    nonempty = sum(1 for _, _, d in zstd_default if d)

    def shown(t):
        assert t.zstd_workgroup_frames >= nonempty and t.zstd_executor_frames == 0, (t.zstd_workgroup_frames, nonempty)
    with gpu_ctx.options(zdec_serial=(1, 0)):
        sweep(gpu_ctx, pna.ALGO_ZSTD, zstd_default, P.FEW_RESIDUES, shown)
        alone_and_permuted(gpu_ctx, pna.ALGO_ZSTD, zstd_default, rd=9, shown=shown)


def test_zstd_parallel_executor_windows(gpu_ctx, pna, own_zstd):
    """zexec_par_min_mib = 1 with windows of 1 MiB (the smallest): the frames of 1 MiB and more are executed by pointer jumping, two windows each,
    k_zx_emit's byte branch at rooms that are not 4-byte aligned; small neighbours touch them on both sides"""
    g, o = own_zstd
    big = [g[-1], o[-1]]
    if P.have_libzstd():
        big += [P.zstd_foreign(lv, chk)[-1] for lv, chk in ((1, False), (3, True), (19, False))]
    assert all(len(d) >= P.MIB for _, _, d in big)
    small = [x for x in g if len(x[2]) in (0, 1, 17, 255, 4097)]
    items = _interleave(big, small)
    n_big = len(big)                                                    # one frame of >= 1 MiB each (the grid's second frame holds 4 099 bytes)

    def shown(t):
        assert t.zstd_executor_frames == n_big and t.zstd_workgroup_frames == 0, (t.zstd_executor_frames, n_big)
    with gpu_ctx.options(zexec_par_min_mib=(1, 8), zexec_win_mib=(1, 1024)):
        sweep(gpu_ctx, pna.ALGO_ZSTD, items, P.FEW_RESIDUES, shown)
        alone_and_permuted(gpu_ctx, pna.ALGO_ZSTD, items, rd=13, shown=shown)


@pytest.mark.parametrize("level,checksum", [(1, False), (19, False), (1, True), (3, True), (19, True)])
def test_zstd_libzstd_frames(gpu_ctx, pna, level, checksum):
    """libzstd's frames at the other levels, with and without Content_Checksum: k_zxxh reads the decoded bytes from rooms at odd offsets (its aligned
    and its unaligned read); a frame whose stored checksum is wrong is refused, so the check has run"""
    if not P.have_libzstd():
        pytest.skip("system libzstd (the writer of the foreign frames) is absent")
    items = P.zstd_foreign(level, checksum)
    sweep(gpu_ctx, pna.ALGO_ZSTD, items, P.FEW_RESIDUES)
    alone_and_permuted(gpu_ctx, pna.ALGO_ZSTD, items, rd=11)
    if checksum:
        k = [n for n, _, _ in items].index("text4097_l%d_chk" % level)
        s = items[k][1]
        bad = list(items)
        bad[k] = (items[k][0], s[:-1] + bytes([s[-1] ^ 1]), items[k][2])
        assert P.zstd_cpu_refuses(bad[k][1], 4097)
        sl, rl = lens(bad)
        for rs, rd in ((1, 1), (2, 8)):
            run_batch(gpu_ctx, pna.ALGO_ZSTD, bad, P.tight(sl, rl, rs, rd), 0xA5, 0xFF, expect_error=pna.E_INVAL)


def test_zstd_foreign_frame_list(gpu_ctx, pna, own_zstd):
    """three libzstd frames with skippable frames between them: the frames are listed (k_zlist) and decoded as a batch of their own into the entry's room"""
    if not P.have_libzstd():
        pytest.skip("system libzstd (the writer of the foreign frames) is absent")
    g, _ = own_zstd
    small = [x for x in g if len(x[2]) in (0, 3, 33, 4095)]
    items = small[:2] + [P.zstd_frame_list()] + small[2:]

    def shown(t):
        assert t.zstd_listed_entries == 1, t.zstd_listed_entries
    sweep(gpu_ctx, pna.ALGO_ZSTD, items, P.FEW_RESIDUES, shown)
    alone_and_permuted(gpu_ctx, pna.ALGO_ZSTD, items, rd=15, shown=shown)


# ================================================================================== deflate
@pytest.mark.parametrize("rd", range(16))
def test_deflate_default_form_every_residue(gpu_ctx, pna, deflate_default, rd):
    """fewer than 1 024 pieces in the call: the wave-per-stream walk (its reader starts src_off & 3 bytes into an aligned word), a wave per stream's records"""
    assert _pieces(deflate_default) < 1024

    def shown(t):
        assert t.inflate_lane_pieces == 0 and t.inflate_chunk_streams == 0
    sweep(gpu_ctx, pna.ALGO_DEFLATE, deflate_default, [(rd % 4, rd)], shown)


def test_deflate_default_form_alone_and_permuted(gpu_ctx, pna, deflate_default):
    alone_and_permuted(gpu_ctx, pna.ALGO_DEFLATE, deflate_default)


@pytest.mark.parametrize("writer", ["fixed", "huff", "stored", "w9"])
def test_deflate_other_writers(gpu_ctx, pna, writer):
    """fixed-code blocks, literals only, stored blocks (copied from the source into the literal scratch), a 512-byte window"""
    sweep(gpu_ctx, pna.ALGO_DEFLATE, P.deflate_foreign(writer), P.FEW_RESIDUES)
    alone_and_permuted(gpu_ctx, pna.ALGO_DEFLATE, P.deflate_foreign(writer), rd=7)


@pytest.fixture(scope="module")
def deflate_many(own_deflate):
    """the small cases repeated to 1 100 streams and more, this library's 1 MiB + 4 099 entry among them: 1 024 pieces and more, lane per piece"""
    small = [x for x in own_deflate if len(x[2]) <= 65537]
    z6 = [x for x in P.deflate_foreign("z6") if len(x[2]) <= 65537]
    items = []
    while len(items) < 1100:
        items += _interleave(small, z6)
    items.insert(len(items) // 2, own_deflate[-1])
    items.insert(7, own_deflate[-2])                                    # (300 001 bytes: three pieces)
    assert _pieces(items) >= 1024
    return items


def test_deflate_lane_per_piece_and_execution_groups(gpu_ctx, pna, deflate_many):
    """k_imark / k_vinflate / k_vfin over every piece of the call, the records executed by execution groups (k_zexec_groups)"""
    n_own = sum(1 for n, _, _ in deflate_many if n.endswith("_own"))

    def shown(t):
        assert t.inflate_lane_pieces == _pieces(deflate_many), (t.inflate_lane_pieces, _pieces(deflate_many))
        assert t.inflate_lane_streams >= n_own, (t.inflate_lane_streams, n_own, len(deflate_many))   # at least every stream of this library's layout stayed with the lanes
    sweep(gpu_ctx, pna.ALGO_DEFLATE, deflate_many, P.FEW_RESIDUES, shown)
    alone_and_permuted(gpu_ctx, pna.ALGO_DEFLATE, deflate_many, rd=7, shown=shown)


def test_deflate_serial_option(gpu_ctx, pna, deflate_many):
    """inflate_serial = 1: the wave-per-stream walk over a call of 1 100 streams"""
    def shown(t):
        assert t.inflate_lane_pieces == 0 and t.inflate_lane_streams == 0
    with gpu_ctx.options(inflate_serial=(1, 0)):
        sweep(gpu_ctx, pna.ALGO_DEFLATE, deflate_many, P.FEW_RESIDUES, shown)
        alone_and_permuted(gpu_ctx, pna.ALGO_DEFLATE, deflate_many, rd=2, shown=shown)


def test_deflate_foreign_stream_in_chunks(gpu_ctx, pna, own_deflate):
    """a foreign 1.5 MiB stream with zexec_par_min_mib = 1: block starts by trial in a misaligned stream (k_ispec), a wave per chunk, pointer jumping"""
    small = [x for x in own_deflate if len(x[2]) in (0, 5, 31, 4097)]
    items = small[:2] + [P.deflate_large()] + small[2:]

    def shown(t):
        assert t.inflate_chunk_streams == 1, t.inflate_chunk_streams
    with gpu_ctx.options(zexec_par_min_mib=(1, 8)):
        sweep(gpu_ctx, pna.ALGO_DEFLATE, items, P.FEW_RESIDUES, shown)
        alone_and_permuted(gpu_ctx, pna.ALGO_DEFLATE, items, rd=3, shown=shown)


# ================================================================================== xz
@pytest.mark.parametrize("rd", range(16))
def test_xz_batch_every_residue(gpu_ctx, pna, rd):
    """the whole xz list in one call: k_lzma2 copies matches and uncompressed chunks with 64 lanes straight into rooms that touch"""
    sweep(gpu_ctx, pna.ALGO_XZ, P.xz_streams(), [(rd % 4, rd)])


def test_xz_alone_and_permuted(gpu_ctx, pna):
    alone_and_permuted(gpu_ctx, pna.ALGO_XZ, P.xz_streams())


# ================================================================================== base addresses that are not aligned
@pytest.mark.parametrize("codec_name", ["zstd", "deflate", "xz"])
def test_base_addresses_need_no_alignment(gpu_ctx, pna, zstd_default, deflate_default, codec_name):
    """d_src and d_dst themselves 1, 7 and 13 bytes off an aligned address, the offsets counted from there: the same rooms, the same guards"""
    algo, items = {"zstd": (pna.ALGO_ZSTD, zstd_default), "deflate": (pna.ALGO_DEFLATE, deflate_default), "xz": (pna.ALGO_XZ, P.xz_streams())}[codec_name]
    sl, rl = lens(items)
    for shift, (rs, rd) in zip(((1, 7), (13, 1), (7, 13)), P.FEW_RESIDUES[1:4]):
        for dst_fill, src_fill in FILLS:
            run_batch(gpu_ctx, algo, items, P.tight(sl, rl, rs, rd), dst_fill, src_fill, shift=shift)


# ================================================================================== the open decoders, the sizes
def _zstd_open(ctx, d_src, src_off, src_len, d_dst, dst_off, dst_cap):
    f = ctx._L.pna_gpu_zstd_decompress_open_device
    f.restype = ctypes.c_int
    f.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64,
                  ctypes.POINTER(ctypes.c_uint64), ctypes.c_void_p]
    raw = ctypes.c_uint64()
    ctx._check(f(ctx._h, ctypes.c_void_p(d_src), src_off, src_len, ctypes.c_void_p(d_dst), dst_off, dst_cap, ctypes.byref(raw), None))
    return raw.value


def _open_items(codec_name, own_zstd, own_deflate):
    if codec_name == "zstd":
        g, o = own_zstd
        return _interleave(g, o[-3:], P.zstd_foreign(3, True) if P.have_libzstd() else [])
    if codec_name == "deflate":
        return _interleave(own_deflate, P.deflate_foreign("z6"))
    return [x for x in P.xz_streams() if x[0].endswith("_p6") or x[0].startswith("mb4") or x[0].endswith("crc32")]


@pytest.mark.parametrize("codec_name", ["zstd", "deflate", "xz"])
@pytest.mark.parametrize("extra", [False, True])
def test_open_decoders(gpu_ctx, pna, own_zstd, own_deflate, codec_name, extra):
    """one stream per call into a room of exactly its size, then into rooms 1 .. 15 bytes larger (the bytes behind the size found are unspecified): the rooms
    touch, so every call also has to leave its neighbours' decoded bytes alone"""
    items = _open_items(codec_name, own_zstd, own_deflate)
    dec = {"zstd": lambda *a: _zstd_open(gpu_ctx, *a), "deflate": gpu_ctx.inflate_open_device, "xz": gpu_ctx.xz_open_device}[codec_name]
    sl, _ = lens(items)
    rooms = [len(d) + (1 + (4 * i) % 15 if extra else 0) for i, (_, _, d) in enumerate(items)]
    for rs, rd in P.FEW_RESIDUES[2:]:
        L = P.tight(sl, rooms, rs, rd)

        def call(d_src, d_dst):
            for i, (name, s, d) in enumerate(items):
                got = dec(d_src, L.src_off[i], len(s), d_dst, L.dst_off[i], rooms[i])
                assert got == len(d), (name, got)
        for dst_fill, src_fill in FILLS:
            run_call(call, items, L, dst_fill, src_fill, unspecified=[(o + len(d), o + r) for o, r, (_, _, d) in zip(L.dst_off, rooms, items)])


@pytest.mark.parametrize("codec_name", ["zstd", "deflate", "xz"])
def test_open_size_at_every_source_residue(gpu_ctx, pna, own_zstd, own_deflate, codec_name):
    """pna_gpu_open_size_device gives the same (size, exact) wherever the stream lies"""
    import numpy as np
    import torch
    algo = {"zstd": pna.ALGO_ZSTD, "deflate": pna.ALGO_DEFLATE, "xz": pna.ALGO_XZ}[codec_name]
    items = [x for x in _open_items(codec_name, own_zstd, own_deflate) if len(x[2]) in (0, 1, 17, 4097, 65537, 300001, P.MIB + 4099)]
    if codec_name == "deflate":
        items.append(P.deflate_large())                                 # measured in chunks between block starts found by trial
    for name, s, d in items:
        for src_fill in (0x00, 0xFF):
            stride = (len(s) + 16 + P.SRC_SLACK + 15) & ~15
            host = np.full(P.GUARD + 16 * stride, src_fill, dtype=np.uint8)
            offs = [P.GUARD + r * stride + r for r in range(16)]
            for o in offs:
                host[o:o + len(s)] = np.frombuffer(s, dtype=np.uint8)
            d_src = torch.from_numpy(host).cuda()
            got = {gpu_ctx.open_size_device(d_src.data_ptr(), o, len(s), algo=algo) for o in offs}
            assert len(got) == 1, (name, got)
            size, exact = next(iter(got))
            assert size == len(d) if exact else size >= len(d), (name, size, exact)
            assert exact or codec_name == "zstd", name
            assert np.array_equal(d_src.cpu().numpy(), host), name


# ================================================================================== refused calls
@pytest.mark.parametrize("codec_name", ["zstd", "deflate", "xz"])
def test_damaged_stream_in_a_tight_batch(gpu_ctx, pna, own_zstd, own_deflate, codec_name):
    """one stream with a bit flipped at its middle, in the middle of a tight batch: the CPU decoder refuses it, the call is PNA_E_INVAL, nothing outside the
    rooms is written, the source is untouched, and the undamaged batch decodes on the same context afterwards"""
    from xz_cases import liblzma_refuses
    algo = {"zstd": pna.ALGO_ZSTD, "deflate": pna.ALGO_DEFLATE, "xz": pna.ALGO_XZ}[codec_name]
    if codec_name == "zstd":
        items = list(own_zstd[0]) if not P.have_libzstd() else _interleave(own_zstd[0], P.zstd_foreign(3, True))
        victim = "text65537_l3_chk" if P.have_libzstd() else "text65537_grid"
        refuses = lambda s: P.zstd_cpu_refuses(s, 65537)
    elif codec_name == "deflate":
        items, victim, refuses = _interleave(own_deflate, P.deflate_foreign("z6")), "text65537_z6", P.deflate_cpu_refuses
    else:
        items, victim, refuses = [x for x in P.xz_streams() if x[0].endswith("_p6")], "text65537_p6", liblzma_refuses
    k = [n for n, _, _ in items].index(victim)
    assert 0 < k < len(items) - 1
    bad = list(items)
    bad[k] = (victim, P.flip_middle(items[k][1]), items[k][2])
    assert refuses(bad[k][1])
    sl, rl = lens(items)
    for rs, rd in ((3, 13), (1, 1)):
        L = P.tight(sl, rl, rs, rd)
        for dst_fill, src_fill in FILLS:
            run_batch(gpu_ctx, algo, bad, L, dst_fill, src_fill, expect_error=pna.E_INVAL)
            run_batch(gpu_ctx, algo, items, L, dst_fill, src_fill)
