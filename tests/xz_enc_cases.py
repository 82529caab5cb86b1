"""The inputs that tests/test_xz_enc_core.py (CPU) and tests/test_gpu_xz_encode.py, tests/test_gpu_xz_encode_forms.py (device) compress to .xz, and the CPU
side of the comparison: the encoder core (csrc/xz_enc_core.h, built with g++ alone by tests/xz_enc_core/Makefile) over the sequences of the oracle's LZ
model -- the very sequences the device's LZ stage hands its coder, so the device's streams must equal these byte for byte.  For the CPU core alone:
parses made by hand (what the LZ stage never writes, and sequences that are wrong), and events(), a decoder that tells what the coder decided."""
import collections
import ctypes
import functools
import lzma
import os
import random
import struct
import subprocess
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(tempfile.gettempdir(), "pna_xz_enc_core_%d" % os.getuid())
SEG = 1 << 20
NEAR_T0 = 60                 # near_stored: the sweep of the "near_stored" input starts at this many zeros (its pieces turn from stored to LZMA chunks near the 75th)
XZ_TO_ZSTD_LEVEL = {0: 1, 1: 3, 2: 3, 3: 3, 4: 6, 5: 6, 6: 6, 7: 10, 8: 10, 9: 10}     # the LZ set of an xz level = that of this zstd level


@functools.lru_cache(maxsize=None)
def inputs():
    """[(name, bytes)]: the chunk edge, stored and LZMA chunks in one block, matches at the 273 cap, rep0, several blocks, all four repeat distances"""
    from oracle import codec
    rnd = random.Random(5)
    text = codec.corpus_file(0, 3, (1 << 20) + 12345)
    return [("empty", b""), ("one", b"x"), ("three", text[:3]), ("forty", text[:40]), ("text5k", text[:5000]),
            ("text65536", text[:65536]), ("text65537", text[:65537]), ("random70000", rnd.randbytes(70000)),
            ("random_then_text", rnd.randbytes(200000) + text[:100000]), ("abab", b"ab" * 70000),
            ("zeros2m1", bytes((2 << 20) + 1)), ("text1m12345", text), ("near_stored", near_stored(NEAR_T0, 128)), ("rep_cycle", rep_cycle())]


def rep_cycle(n: int = 150000, seed: int = 3) -> bytes:
    """copies that take turns among two, three and four distances, a few fresh bytes between them: the LZ stage finds the copies, and the coder meets every
    one of its four latest distances again -- rep0 .. rep3, with lengths on both sides of 18 (the repeat lengths' high tree)"""
    rnd = random.Random(seed)
    d = bytearray(rnd.randbytes(24000))
    pools = [(3001, 7013), (3001, 7013, 12007), (3001, 7013, 12007, 20011)]
    i = 0
    while len(d) < n:
        pool = pools[(len(d) // 20000) % 3]
        d += rnd.randbytes(rnd.choice((1, 2, 6)))
        dist = pool[i % len(pool)]
        i += 1
        d += d[len(d) - dist:len(d) - dist + rnd.choice((5, 8, 12, 17, 18, 30, 60, 200))]
    return bytes(d[:n])


@functools.lru_cache(maxsize=None)
def far(seed: int = 4) -> bytes:
    """1 MiB for level 9 (the only LZ set whose offsets span a whole segment; at level 6 every chunk of this is stored): random bytes whose last 150 000 are
    500-byte copies of the first 150 000, three fresh bytes between them -- distances beyond 2^19 (slots 38 and 39) and matches at the 273 cap"""
    rnd = random.Random(seed)
    head = rnd.randbytes(150000)
    tail = b"".join(head[o:o + 500] + rnd.randbytes(3) for o in range(0, 149500, 500))
    return head + rnd.randbytes(SEG - len(head) - len(tail)) + tail


def near_stored(t0: int, n: int, size: int = 8192, seed: int = 11) -> bytes:
    """n pieces of `size` bytes that barely compress: random bytes, then t0, t0 + 1, ... zeros.  One zero more shortens a piece's LZMA form by about a
    byte, so over the sweep the form passes through every size around the piece's own: the chunks at the edge between LZMA and stored, where the
    6-byte header of the one and the 3-byte header of the other decide (xze_chunk, xze_bound)"""
    rnd = random.Random(seed)
    return b"".join(rnd.randbytes(size - (t0 + k)) + bytes(t0 + k) for k in range(n))


def built():
    subprocess.run(["make", "-s", "-C", os.path.join(HERE, "xz_enc_core"), "OUT=" + OUT, "lib", "san"], check=True)
    return OUT


@functools.lru_cache(maxsize=None)
def core():
    lib = ctypes.CDLL(os.path.join(built(), "libxz_enc_host.so"))
    lib.xze_host_bound.restype = ctypes.c_size_t
    lib.xze_host_bound.argtypes = [ctypes.c_size_t]
    lib.xze_host_stream.restype = ctypes.c_size_t
    lib.xze_host_stream.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t]
    lib.xze_host_decode.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t)]
    return lib


def lz_params(level: int, blk_log: int):
    """the oracle's LZ parameters of an xz level: the zstd level's set of the table above, matches of at most 273 bytes"""
    from oracle import codec
    p = codec.params_for_level(XZ_TO_ZSTD_LEVEL[level], blk_log=blk_log)
    p.max_len = 273
    return p


def model_sequences_of(data: bytes, level: int = 6, blk_log: int = 16, **model):
    """(nseq per LZ block, packed sequences) of any bytes, segment by segment; **model: parameters of the oracle's LZ model (mtile)"""
    return _model_sequences(bytes(data), level, blk_log, tuple(sorted(model.items())))


@functools.lru_cache(maxsize=64)
def _model_sequences(data: bytes, level: int, blk_log: int, model: tuple):
    from oracle import codec
    p = lz_params(level, blk_log)
    for k, v in model:
        setattr(p, k, v)
    counts, packed = [], []
    L = codec.lib()
    L.pna_seg_params.restype = ctypes.POINTER(codec.ZstdParams)
    L.pna_seg_params.argtypes = [ctypes.POINTER(codec.ZstdParams), ctypes.c_uint32, ctypes.POINTER(codec.ZstdParams)]
    for s0 in range(0, len(data), SEG):
        seg, tmp = data[s0:s0 + SEG], codec.ZstdParams()
        ps = codec.ZstdParams.from_buffer_copy(L.pna_seg_params(ctypes.byref(p), len(seg), ctypes.byref(tmp)).contents)   # (a short segment: the small geometry)
        for seqs, _ in codec.model_lz_segment(seg, ps):
            counts.append(len(seqs))
            packed += [off | (ml << 20) | (ll << 38) for ll, ml, off in seqs]
    return counts, packed


def model_sequences(name: str, level: int, blk_log: int):
    """model_sequences_of a named input"""
    return model_sequences_of(dict(inputs())[name], level, blk_log)


def stream_of_parse(data: bytes, blk_log: int, counts, packed) -> bytes:
    """the encoder core's stream over any parse: counts[b] sequences for LZ block b, packed as the LZ stage packs them; empty: it did not fit the bound"""
    lib = core()
    cap = lib.xze_host_bound(len(data))
    out = ctypes.create_string_buffer(cap)
    ns = (ctypes.c_uint32 * max(len(counts), 1))(*counts)
    sq = (ctypes.c_uint64 * max(len(packed), 1))(*packed)
    n = lib.xze_host_stream(bytes(data), len(data), blk_log, sq, ns, out, cap)
    return out.raw[:n]


def cpu_stream_of(data: bytes, level: int = 6, blk_log: int = 16, **model) -> bytes:
    """the encoder core's stream over the model's sequences of any bytes"""
    return _cpu_stream(bytes(data), level, blk_log, tuple(sorted(model.items())))


@functools.lru_cache(maxsize=256)
def _cpu_stream(data: bytes, level: int, blk_log: int, model: tuple) -> bytes:
    counts, packed = _model_sequences(data, level, blk_log, model)
    out = stream_of_parse(data, blk_log, counts, packed)
    assert out, (len(data), level, blk_log, model)
    return out


def cpu_stream(name: str, level: int = 6, blk_log: int = 16) -> bytes:
    """cpu_stream_of a named input"""
    return cpu_stream_of(dict(inputs())[name], level, blk_log)


def literal_stream(data: bytes, blk_log: int) -> bytes:
    """the encoder core's stream over a parse without matches (every LZ block: no sequence, all literals); empty: it did not fit the bound"""
    lib = core()
    cap = lib.xze_host_bound(len(data))
    out = ctypes.create_string_buffer(cap)
    nblk = sum((min(SEG, len(data) - s) + (1 << blk_log) - 1) >> blk_log for s in range(0, len(data), SEG))
    ns = (ctypes.c_uint32 * max(nblk, 1))()
    sq = (ctypes.c_uint64 * 1)()
    n = lib.xze_host_stream(data, len(data), blk_log, sq, ns, out, cap)
    return out.raw[:n]


def chunks(stream: bytes):
    """[(control byte, uncompressed size, bytes the chunk takes in the stream)] of every block of a stream, in order"""
    recs, _ = index_records(stream)
    pos, out = 12, []
    for unpadded, _ in recs:
        p = pos + 12
        while stream[p]:
            c, u = stream[p], ((stream[p + 1] << 8) | stream[p + 2]) + 1
            if c < 0x80:
                out.append((c, u, 3 + u))
                p += 3 + u
            else:
                z = ((stream[p + 3] << 8) | stream[p + 4]) + 1
                out.append((c, u + ((c & 0x1F) << 16), 6 + z))
                p += 6 + z
        pos += (unpadded + 3) & ~3
    return out


def case_file(path: str, name: str, level: int, blk_log: int):
    """the input of the stand-alone program: u64 n, u32 blk_log, u32 nblocks | u32 nseq[nblocks] | u64 seqs[] | the bytes"""
    parse_case_file(path, dict(inputs())[name], blk_log, *model_sequences(name, level, blk_log))


def parse_case_file(path: str, data: bytes, blk_log: int, counts, packed):
    """the same for any bytes and any parse of them (stream_of_parse)"""
    with open(path, "wb") as f:
        f.write(struct.pack("<QII", len(data), blk_log, len(counts)))
        f.write(struct.pack("<%dI" % len(counts), *counts))
        f.write(struct.pack("<%dQ" % len(packed), *packed))
        f.write(data)


def literal_case_file(path: str, data: bytes, blk_log: int):
    """the same for a parse without matches (literal_stream)"""
    nblk = sum((min(SEG, len(data) - s) + (1 << blk_log) - 1) >> blk_log for s in range(0, len(data), SEG))
    with open(path, "wb") as f:
        f.write(struct.pack("<QII", len(data), blk_log, nblk) + bytes(4 * nblk) + data)


def at_the_edge():
    """[(bytes, blk_log)] for literal_stream: 128 equal chunks of 8 KiB, and one of 64 KiB, whose all-literal LZMA forms are a few bytes around the
    chunk's own size -- if a chunk might cost more than its stored form, 128 of them leave the entry's bound"""
    return [(near_stored(t, 1) * 128, 13) for t in range(140, 156)] + [(near_stored(t, 1, 65536), 16) for t in range(935, 965)]


def index_records(stream: bytes):
    """[(unpadded size, uncompressed size)] of a stream's Index, and its check type"""
    assert stream[:6] == b"\xfd7zXZ\x00" and stream[-2:] == b"YZ"
    isize = (int.from_bytes(stream[-8:-4], "little") + 1) * 4
    ix = stream[len(stream) - 12 - isize:len(stream) - 12]
    assert ix[0] == 0
    pos = 1

    def vli():
        nonlocal pos
        v = sh = 0
        while True:
            b = ix[pos]
            pos += 1
            v |= (b & 0x7F) << sh
            sh += 7
            if not b & 0x80:
                return v
    n = vli()
    return [(vli(), vli()) for _ in range(n)], stream[7]


# ---- what a stream's LZMA coder decided, event by event
EVENT_KEYS = (["stored", "lit_plain", "lit_matched", "rep0", "rep1", "rep2", "rep3", "shortrep", "len_low", "len_mid", "len_high", "replen_low", "replen_mid",
               "replen_high", "len273"] + ["lenstate%d" % i for i in range(4)] + ["slot%d" % i for i in range(40)])


class Events(collections.Counter):
    """events(): the counts, and beside them `data` (the bytes the stream decodes to) and `trace` ([(position in data, kind, bytes)] in order; kind:
    "lit", "match", "rep0" .. "rep3", "shortrep"; stored chunks leave no entry)"""
    data = b""
    trace = ()


def events(stream: bytes) -> "Events":
    """A small LZMA2 event decoder written from the format (the .xz file format 1.1.0 and the LZMA specification of the LZMA SDK), independent of xz_core.h:
    walks the blocks by the Index, decodes every chunk and counts what the coder chose -- EVENT_KEYS: stored chunks, plain and matched literals, the four
    repeat distances, short repeats, the three trees of the match and of the repeat lengths, the four pos-slot contexts, the distance slots, pieces of 273.
    It knows what this encoder writes and refuses anything else: lc 3, lp 0, pb 2, the state and the probabilities new at every LZMA chunk, the dictionary
    kept within a block (a 1 MiB dictionary: distances below 2^20, slots 0 .. 39).  About 10^5 events a second."""
    recs, _ = index_records(stream)
    ev = Events()
    whole, trace, pos = bytearray(), [], 12
    for unpadded, usize in recs:
        hdr = (stream[pos] + 1) * 4
        p, out = pos + hdr, bytearray()
        while stream[p]:
            c, u = stream[p], ((stream[p + 1] << 8) | stream[p + 2]) + 1
            assert c in (1, 2) or c >= 0xC0, hex(c)
            assert (c in (1, 0xE0 | (c & 0x1F))) == (not out), hex(c)   # the block's first chunk, and no other, resets the dictionary
            if c < 0x80:
                out += stream[p + 3:p + 3 + u]
                p += 3 + u
                ev["stored"] += 1
                continue
            u += (c & 0x1F) << 16
            z = ((stream[p + 3] << 8) | stream[p + 4]) + 1
            assert stream[p + 5] == 93
            _lzma_chunk(stream, p + 6, p + 6 + z, u, out, ev, trace, len(whole))
            p += 6 + z
        assert len(out) == usize and p + 1 <= pos + unpadded - 8
        whole += out
        pos += (unpadded + 3) & ~3
    ev.data, ev.trace = bytes(whole), trace
    return ev


def _lzma_chunk(buf, p, end, usize, out, ev, trace, base):
    """one LZMA chunk buf[p, end) of usize bytes, decoded behind `out` (the block so far = the dictionary)"""
    is_match, is_rep, is_rep0, is_rep1, is_rep2, is_rep0_long = [1024] * 192, [1024] * 12, [1024] * 12, [1024] * 12, [1024] * 12, [1024] * 192
    pos_slot, pos_special, pos_align, lit = [1024] * 256, [1024] * 128, [1024] * 16, [1024] * (8 * 0x300)
    len_m = ([1024] * 2, [1024] * 32, [1024] * 32, [1024] * 256)            # choice bits, low[pos_state], mid[pos_state], high
    len_r = ([1024] * 2, [1024] * 32, [1024] * 32, [1024] * 256)
    assert buf[p] == 0
    rng, code = 0xFFFFFFFF, int.from_bytes(buf[p + 1:p + 5], "big")
    p += 5

    def bit(pr, i):
        nonlocal rng, code, p
        v = pr[i]
        bound = (rng >> 11) * v
        if code < bound:
            rng, b = bound, 0
            pr[i] = v + ((2048 - v) >> 5)
        else:
            rng -= bound
            code -= bound
            b = 1
            pr[i] = v - (v >> 5)
        if rng < 0x1000000:
            rng <<= 8
            code = (code << 8) | buf[p]
            p += 1
        return b

    def tree(pr, at, n):
        m = 1
        for _ in range(n):
            m = (m << 1) | bit(pr, at + m)
        return m - (1 << n)

    def rev_tree(pr, at, n):
        m, v = 1, 0
        for i in range(n):
            b = bit(pr, at + m)
            m = (m << 1) | b
            v |= b << i
        return v

    def direct(n):
        nonlocal rng, code, p
        v = 0
        for _ in range(n):
            rng >>= 1
            b = 1 if code >= rng else 0
            code -= rng * b
            v = (v << 1) | b
            if rng < 0x1000000:
                rng <<= 8
                code = (code << 8) | buf[p]
                p += 1
        return v

    def length(L, name, ps):
        if not bit(L[0], 0):
            ev[name + "_low"] += 1
            return 2 + tree(L[1], ps * 8, 3)
        if not bit(L[0], 1):
            ev[name + "_mid"] += 1
            return 10 + tree(L[2], ps * 8, 3)
        ev[name + "_high"] += 1
        return 18 + tree(L[3], 0, 8)

    state, rep0, rep1, rep2, rep3 = 0, 0, 0, 0, 0
    stop = len(out) + usize
    while len(out) < stop:
        at = len(out)
        ps = at & 3
        if not bit(is_match, state * 16 + ps):
            lb, sym = 0x300 * ((out[-1] if out else 0) >> 5), 1
            if state >= 7:
                ev["lit_matched"] += 1
                mb = out[at - rep0 - 1]
                while sym < 0x100:
                    mbit = (mb >> 7) & 1
                    mb = (mb << 1) & 0xFF
                    b = bit(lit, lb + ((1 + mbit) << 8) + sym)
                    sym = (sym << 1) | b
                    if mbit != b:
                        break
            else:
                ev["lit_plain"] += 1
            while sym < 0x100:
                sym = (sym << 1) | bit(lit, lb + sym)
            out.append(sym & 0xFF)
            trace.append((base + at, "lit", 1))
            state = 0 if state < 4 else (state - 3 if state < 10 else state - 6)
            continue
        if bit(is_rep, state):
            if not bit(is_rep0, state):
                if not bit(is_rep0_long, state * 16 + ps):
                    ev["shortrep"] += 1
                    assert rep0 < at
                    out.append(out[at - rep0 - 1])
                    trace.append((base + at, "shortrep", 1))
                    state = 9 if state < 7 else 11
                    continue
                kind = "rep0"
            else:
                if not bit(is_rep1, state):
                    kind, d = "rep1", rep1
                else:
                    if not bit(is_rep2, state):
                        kind, d = "rep2", rep2
                    else:
                        kind, d, rep3 = "rep3", rep3, rep2
                    rep2 = rep1
                rep1, rep0 = rep0, d
            ev[kind] += 1
            n = length(len_r, "replen", ps)
            state = 8 if state < 7 else 11
        else:
            kind = "match"
            rep3, rep2, rep1 = rep2, rep1, rep0
            n = length(len_m, "len", ps)
            state = 7 if state < 7 else 10
            ls = min(n - 2, 3)
            ev["lenstate%d" % ls] += 1
            slot = tree(pos_slot, ls * 64, 6)
            ev["slot%d" % slot] += 1
            if slot < 4:
                rep0 = slot
            else:
                nb = (slot >> 1) - 1
                rep0 = (2 | (slot & 1)) << nb
                if slot < 14:
                    rep0 += rev_tree(pos_special, rep0 - slot, nb)
                else:
                    rep0 += direct(nb - 4) << 4
                    rep0 += rev_tree(pos_align, 0, 4)
        assert rep0 < at and n <= stop - at, (kind, rep0, at, n)          # inside the dictionary, inside the chunk
        if n == 273:
            ev["len273"] += 1
        trace.append((base + at, kind, n))
        src = at - rep0 - 1
        if rep0 + 1 >= n:
            out += out[src:src + n]
        else:
            out += (bytes(out[src:]) * (n // (rep0 + 1) + 1))[:n]
    assert p == end and code == 0, (p, end, code)                          # the chunk's bytes, all of them, and a finished range coder


# ---- parses made by hand: what the LZ stage never hands the coder
HM_LENGTHS = (2, 3, 4, 5, 6, 9, 10, 17, 18, 19, 100, 272, 273, 274, 275, 545, 546, 547, 548, 1000, 5000, 70000)
HM_DISTANCES = tuple(range(1, 9)) + (15, 16, 17, 96, 127, 128, 129, 1000, 4095, 4096, 4097, 65535, 65536, 65537, 300000, 0xFFFFF)
HM_SIZES = (100, 8192, 8193, 70000, 300000, SEG + 777, 2 * SEG + 5)


def pack_seq(ll: int, ml: int, dist: int) -> int:
    return dist | (ml << 20) | (ll << 38)


def random_parse(size: int, blk_log: int, seed: int):
    """(data, [[(position in its segment, ll, ml, dist)] per block]): a random parse and the bytes it describes -- per LZ block, runs of
    0 .. 20 fresh bytes and copies with lengths of HM_LENGTHS (the long ones one time in ten; clipped to the block) at distances of HM_DISTANCES
    (clipped to the position in the segment), 60 % of them from a pool of four distances that changes slowly; the rest of a block: literals"""
    rnd = random.Random(seed)
    data, blocks = bytearray(), []
    pool = [rnd.choice(HM_DISTANCES) for _ in range(4)]
    for s0 in range(0, size, SEG):
        sl = min(SEG, size - s0)
        for c0 in range(0, sl, 1 << blk_log):
            end, pos, seqs = min(sl, c0 + (1 << blk_log)), c0, []
            while pos < end:
                ll = min(max(rnd.choice((0, 0, 1, 1, 2, 3, 6, 20)), 0 if pos else 1), end - pos)
                if rnd.random() < 0.02:
                    pool[rnd.randrange(4)] = rnd.choice(HM_DISTANCES)
                dist = min(rnd.choice(pool) if rnd.random() < 0.6 else rnd.choice(HM_DISTANCES), pos + ll)
                ml = min(rnd.choice(HM_LENGTHS if rnd.random() < 0.1 else HM_LENGTHS[:HM_LENGTHS.index(545)]), end - pos - ll)
                if ml < 2:
                    data += rnd.randbytes(end - pos)
                    break
                data += rnd.randbytes(ll)
                src = len(data) - dist
                data += data[src:src + ml] if dist >= ml else (bytes(data[src:]) * (ml // dist + 1))[:ml]
                seqs.append((pos, ll, ml, dist))
                pos += ll + ml
            blocks.append(seqs)
    assert len(data) == size
    return bytes(data), blocks


def _packed(blocks):
    return [len(b) for b in blocks], [pack_seq(ll, ml, dist) for b in blocks for _, ll, ml, dist in b]


@functools.lru_cache(maxsize=None)
def hand_made_cases():
    """[(data, blk_log, nseq per block, packed sequences)] for the CPU core only: every size of HM_SIZES at 8, 16 and 64 KiB blocks"""
    out = []
    for i, size in enumerate(HM_SIZES):
        for j, blk_log in enumerate((13, 14, 16)):
            data, blocks = random_parse(size, blk_log, 1000 + 3 * i + j)
            out.append((data, blk_log) + tuple(_packed(blocks)))
    return out


def split_case():
    """(data, blk_log, nseq per block, packed sequences, [(position, ml)]): single matches longer than 273 bytes -- 274, 275, 546, 547 and the first chunk's
    rest in the first chunk, 65 000 in the second --, each behind three fresh bytes and at a distance of its own, so a match's first piece is no repeat"""
    rnd = random.Random(77)
    data, blocks, at = bytearray(rnd.randbytes(300)), [[], []], []
    for blk, ml, dist in ((0, 274, 290), (0, 275, 150), (0, 546, 700), (0, 547, 33), (0, 0, 1200), (1, 65000, 300)):
        data += rnd.randbytes(3)
        ml = ml or 65536 - len(data)
        at.append((len(data), ml))
        src = len(data) - dist
        blocks[blk].append((len(data) - 3, 3, ml, dist) if blocks[0] else (0, len(data), ml, dist))
        data += data[src:src + ml] if dist >= ml else (bytes(data[src:]) * (ml // dist + 1))[:ml]
    data += rnd.randbytes(20)
    assert len(data) == 65536 + 3 + 65000 + 20
    return (bytes(data), 16) + tuple(_packed(blocks)) + (at,)


@functools.lru_cache(maxsize=None)
def broken_sequence_cases():
    """[(what, data, blk_log, nseq per block, packed sequences, position, chunk end)]: a valid parse of two segments at 8 KiB blocks with ONE sequence made
    wrong, the one that begins at `position` (of the data) in the last quarter of its chunk and has sequences behind it.  The stream the coder owes is
    still valid: from `position` to `chunk end` the chunk is literals."""
    size, blk_log = SEG + 40000, 13
    data, blocks = random_parse(size, blk_log, 4242)
    bsz, per_seg = 1 << blk_log, SEG >> blk_log

    def case(what, b, make, k=None):
        """block b's sequence k -- by default the first in the chunk's last quarter that has two more behind it -- replaced by make(...) of it"""
        s0, c0 = (SEG if b >= per_seg else 0), (b % per_seg) * bsz
        if k is None:
            k = next(i for i, q in enumerate(blocks[b]) if q[0] >= c0 + 3 * bsz // 4 and i + 2 < len(blocks[b]))
        pos, ll, ml, dist = blocks[b][k]
        bad = [list(x) for x in blocks]
        bad[b][k] = (pos,) + make(pos, ll, ml, dist, c0 + bsz)
        return (what, data, blk_log) + tuple(_packed(bad)) + (s0 + pos, s0 + c0 + bsz)
    # (the last two in the SECOND segment: in front of it lies memory, the first segment's, so nothing but the coder's own check stops a distance there)
    return [case("dist == 0", 3, lambda pos, ll, ml, dist, end: (ll, ml, 0)),
            case("dist == pos + ll + 1", 0, lambda pos, ll, ml, dist, end: (ll, ml, pos + ll + 1)),
            case("ml == 1", 5, lambda pos, ll, ml, dist, end: (ll, 1, dist)),
            case("ll one past the chunk's end", 7, lambda pos, ll, ml, dist, end: (end - pos + 1, ml, dist)),
            case("ml one past the chunk's end", per_seg + 2, lambda pos, ll, ml, dist, end: (ll, end - pos - ll + 1, dist)),
            case("the second chunk's first sequence reaches in front of the segment", per_seg + 1, lambda pos, ll, ml, dist, end: (ll, ml, pos + ll + 1), k=0)]


# ---- archives of xz payloads (tests/test_gpu_xz_encode.py, tests/test_gpu_xz_encode_forms.py)
def _entries():
    text = dict(inputs())["text1m12345"]
    rnd = dict(inputs())["random70000"]
    return ["a/text.txt", "a/empty", "b/random.bin", "b/big.txt"], [text[:5000], b"", rnd[:40000], text[:(1 << 20) + 100]]


def _check_archive(pna, pf, codec, ctx, arc, names, ents, password=None):
    """the archive through the existing read-side drivers, through the oracle's container parser, and its payloads through liblzma"""
    got = pna.extract_archive(ctx, arc, password)
    assert [(n, d) for n, _, d in got] == list(zip(names, ents))
    recs, summ = pna.verify_archive(ctx, arc, password)
    assert summ["rc"] == 0 and len(recs) == len(names) and all(r[2] == pna.VERIFY_OK for r in recs)
    _, items = pf.read_archive(arc)
    assert len(items) == len(names)
    for it, n, e in zip(items, names, ents):
        assert (it.name, it.compression, it.raw_file_size) == (n, pna.ALGO_XZ, len(e))     # FHED compression byte 4
        payload = it.data
        if it.encryption:
            phsf = [d for ty, d in it.chunks if ty == b"PHSF"][0].decode()
            if it.cipher_mode == 2:                                                        # GCM STREAM: the key is bound to the entry's header chunk
                payload = codec.decrypt_payload_gcm(codec.derive_key_from_phsf(phsf, password), it.data, it.chunks[0][0], it.chunks[0][1], phsf.encode())
                assert lzma.decompress(payload, format=lzma.FORMAT_XZ) == e, n
                continue
            payload = codec.decrypt_payload(it.encryption, it.cipher_mode, codec.derive_key_from_phsf(phsf, password), it.data)
        assert lzma.decompress(payload, format=lzma.FORMAT_XZ) == e, n
    return items
