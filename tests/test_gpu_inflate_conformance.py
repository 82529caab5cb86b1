"""The device inflate decoders on hand-built deflate streams (tests/inflate_cases.py; tests/test_inflate_cases.py ties every one of them to the system
zlib on the CPU): the wave-per-stream walk (k_inflate), the lane-per-piece decoder (k_vinflate, whole streams and pieces), the chunk decoder (k_ispec +
k_inflate's chunk mode) and the open-size decoder.  The expected bytes are always the case's plain bytes; every call lies between guard bands
(test_gpu_decode_placement.run_call: rooms, guards, source untouched), and every route is shown by pna_gpu_last_decode_forms.  Nothing here has a
tolerance: byte equality, a route counter, or an error code."""
import io

import pytest

import inflate_cases as C
import placement_cases as P
from test_gpu_decode_placement import lens, run_batch, run_call

pytestmark = pytest.mark.gpu


def items_of(cases):
    return [(n, s, d) for n, s, d, _ in cases]


def accept(*names):
    by = {c[0]: c for c in C.accept_cases()}
    return items_of(by[n] for n in names)


def tiny_random(limit=600):
    return [c for c in items_of(C.random_cases()) if len(c[2]) <= limit]


def decode(ctx, pna, items, rs=1, rd=5, **kw):
    sl, rl = lens(items)
    return run_batch(ctx, pna.ALGO_DEFLATE, items, P.tight(sl, rl, rs, rd), 0xA5, 0x00, **kw)


SINGLE = ("one-dist-code", "one-dist-code-sym3", "two-dist-codes", "no-dist-code", "eob-only")
RING = tuple("reseat-d%d" % d for d in (0, 1, 2, 3, 4, 1023)) + ("big-header-at-ring-edge-1024", "big-header-at-ring-edge-2048")


# ================================================================================== wave per stream
def test_wave_per_stream_every_accept_case(gpu_ctx, pna):
    """inflate_serial = 1, one call over every accept case but the large stream (the three-piece streams included: 1.8 MiB of output)"""
    items = items_of(C.accept_cases())
    with gpu_ctx.options(inflate_serial=(1, 0)):
        decode(gpu_ctx, pna, items)
        t = gpu_ctx.decode_forms()
    assert t.inflate_lane_pieces == 0 and t.inflate_lane_streams == 0 and t.inflate_chunk_streams == 0


def test_wave_per_stream_random_streams(gpu_ctx, pna):
    with gpu_ctx.options(inflate_serial=(1, 0)):
        decode(gpu_ctx, pna, items_of(C.random_cases()), rs=3, rd=13)
        t = gpu_ctx.decode_forms()
    assert t.inflate_lane_pieces == 0 and t.inflate_chunk_streams == 0


@pytest.mark.parametrize("rs", range(4))
def test_reseat_and_ring_edge_at_every_source_residue(gpu_ctx, pna, rs):
    """every re-seat and ring-edge stream starts rs bytes behind a 4-byte boundary of the source buffer: the reader is re-seated behind the stored block
    at every p & 3, next to a ring half's end"""
    items = accept(*RING)
    sl, rl = lens(items)
    so, pos = [], P.GUARD + rs
    for n in sl:
        so.append(pos)
        pos = ((pos + n + 3) & ~3) + rs
    do = [P.GUARD + 7 + sum(rl[:k]) for k in range(len(rl))]
    L = P.Layout("residue %d" % rs, so, sl, do, rl, pos + P.SRC_SLACK, do[-1] + rl[-1] + P.GUARD)
    assert all(o % 4 == rs for o in so)
    for dst_fill, src_fill in ((0xA5, 0x00), (0x00, 0xFF)):
        run_batch(gpu_ctx, pna.ALGO_DEFLATE, items, L, dst_fill, src_fill)
    t = gpu_ctx.decode_forms()
    assert t.inflate_lane_pieces == 0 and t.inflate_chunk_streams == 0


# ================================================================================== lane per piece
def test_lane_per_piece_whole_streams(gpu_ctx, pna):
    """every accept case of at most 128 KiB of output and the 200 random streams, then the smallest random streams again until the call has 1 024 streams
    (repeating all of them would decode 7 MiB): every one is a piece of its own and must STAY with the lanes -- a stream k_vfin hands to the serial walk
    decodes all the same, so the count is what shows that the lanes decode the rare branches.  No case is exempt: k_vinflate takes every block type, and a
    stream of at most one piece has no marker count to fit."""
    items = [c for c in items_of(C.accept_cases()) if len(c[2]) <= C.BLK] + items_of(C.random_cases())
    tiny = tiny_random()
    assert len(tiny) >= 8
    k = 0
    while len(items) < 1024:
        items.append(tiny[k % len(tiny)])
        k += 1
    decode(gpu_ctx, pna, items, rs=2, rd=8)
    t = gpu_ctx.decode_forms()
    assert t.inflate_lane_pieces == len(items) and t.inflate_chunk_streams == 0, (t.inflate_lane_pieces, len(items))
    assert t.inflate_lane_streams == len(items), (t.inflate_lane_streams, len(items))


def test_lane_per_piece_pieces_of_another_writer(gpu_ctx, pna):
    """two streams in this library's piece layout that this library did not write: pieces 2 and 3 copy from the piece in front (one execution group:
    k_vfin), and in the second a stored block holds 00 00 FF FF, so its marker count does not fit and the serial walk takes it"""
    big = accept("own-layout-3-pieces", "chance-marker")
    tiny = tiny_random()
    items = [tiny[k % len(tiny)] for k in range(1024 - 6)]
    items.insert(300, big[0])
    items.insert(700, big[1])
    decode(gpu_ctx, pna, items, rs=3, rd=1)
    t = gpu_ctx.decode_forms()
    assert t.inflate_lane_pieces == 1024 and t.inflate_lane_streams == len(items) - 1, (t.inflate_lane_pieces, t.inflate_lane_streams, len(items))


# ================================================================================== chunks
def test_chunk_decoder_and_serial_walk_on_the_large_stream(gpu_ctx, pna):
    """zexec_par_min_mib = 1: block starts by trial among deep, single-code and stored headers at every bit phase, a wave per chunk; then the same stream
    through the wave-per-stream walk"""
    items = items_of([C.large_case()])
    with gpu_ctx.options(zexec_par_min_mib=(1, 8)):
        decode(gpu_ctx, pna, items, rs=1, rd=3)
        t = gpu_ctx.decode_forms()
    assert t.inflate_chunk_streams == 1 and t.inflate_lane_pieces == 0, t.inflate_chunk_streams
    decode(gpu_ctx, pna, items, rs=2, rd=9)
    t = gpu_ctx.decode_forms()
    assert t.inflate_chunk_streams == 0 and t.inflate_lane_pieces == 0


@pytest.mark.parametrize("k", range(3))
def test_chunk_decoder_finds_every_kind_of_block_start(gpu_ctx, pna, k):
    """a large stream whose block starts are all of one kind -- deep dynamic headers with repeat symbols, headers with a single one-bit distance code,
    stored headers at every bit phase behind fixed-code blocks --: the trial parser must find them, or the stream would go to the serial walk"""
    items = items_of([C.large_family_cases()[k]])
    with gpu_ctx.options(zexec_par_min_mib=(1, 8)):
        decode(gpu_ctx, pna, items, rs=k + 1, rd=2 * k + 1)
        t = gpu_ctx.decode_forms()
    assert t.inflate_chunk_streams == 1 and t.inflate_lane_pieces == 0, (items[0][0], t.inflate_chunk_streams)


# ================================================================================== open size
def test_open_decoder_finds_the_size(gpu_ctx, pna):
    items = accept("deep-greedy", "deep-norepeat", "deep-258-as-284+31", *SINGLE, "ll-split-mixed", *("stored-phase-%d" % k for k in range(8)))
    sl, _ = lens(items)
    rooms = [len(d) + 1 + (4 * i) % 15 for i, (_, _, d) in enumerate(items)]
    L = P.tight(sl, rooms, 3, 13)

    def call(d_src, d_dst):
        for i, (name, s, d) in enumerate(items):
            got = gpu_ctx.inflate_open_device(d_src, L.src_off[i], len(s), d_dst, L.dst_off[i], rooms[i])
            assert got == len(d), (name, got, len(d))
    run_call(call, items, L, 0xA5, 0xFF, unspecified=[(o + len(d), o + r) for o, r, (_, _, d) in zip(L.dst_off, rooms, items)])


# ================================================================================== refusals
def test_wave_per_stream_refuses_what_zlib_refuses(gpu_ctx, pna):
    """every reject case alone: PNA_E_INVAL, nothing outside the room written; then a good stream on the same context"""
    with gpu_ctx.options(inflate_serial=(1, 0)):
        for name, s, _, props in C.reject_cases():
            decode(gpu_ctx, pna, [(name, s, bytes(props["raw"]))], rs=1, rd=1, expect_error=pna.E_INVAL)
        decode(gpu_ctx, pna, accept("deep-greedy", "eob-only", "stored-phase-3"))


def test_verify_gives_every_refused_stream_its_own_verdict(gpu_ctx, pna):
    """one archive of 1 024 small good streams with every reject case among them: the lanes refuse a stream without disturbing the 63 neighbours of its wave"""
    good = tiny_random() + accept(*SINGLE, *("stored-phase-%d" % k for k in range(8)))
    rejects = C.reject_cases()
    entries, bad = [], set()
    step = 1024 // len(rejects)
    for k in range(1024):
        if k % step == 5 and k // step < len(rejects):
            name, s, _, props = rejects[k // step]
            bad.add(len(entries))
            entries.append(("bad/%s" % name, s, props["raw"]))
        name, s, d = good[k % len(good)]
        entries.append(("good/%04d-%s" % (k, name), s, len(d)))
    assert len(bad) == len(rejects)
    arc = pna.Archive(io.BytesIO())
    for name, s, raw in entries:
        arc.add_file(name, pna.Compression.Deflate, raw, s)
    try:
        recs, summ = pna.verify_archive(gpu_ctx, arc.finalize().getvalue())
    except pna.PnaGpuError as e:
        if e.code == pna.E_HIP:                                         # the device has faulted; nothing more is run on it
            pytest.exit("HIP error in verify_archive: %s" % e, returncode=3)
        raise
    assert summ["rc"] == 0 and [r[0] for r in recs] == [e[0] for e in entries]
    assert gpu_ctx.decode_forms().inflate_lane_pieces >= 1024           # the lanes had every stream first
    assert [i for i, r in enumerate(recs) if r[2] != pna.VERIFY_OK] == sorted(bad)
    assert all(recs[i][2] == pna.VERIFY_BAD_STREAM for i in bad), [(recs[i][0], recs[i][2]) for i in bad if recs[i][2] != pna.VERIFY_BAD_STREAM]
