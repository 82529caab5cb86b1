"""The inputs that tests/test_xz_enc_core.py (CPU) and tests/test_gpu_xz_encode.py (device) compress to .xz, and the CPU side of the comparison: the
encoder core (csrc/xz_enc_core.h, built with g++ alone by tests/xz_enc_core/Makefile) over the sequences of the oracle's LZ model -- the very
sequences the device's LZ stage hands its coder, so the device's streams must equal these byte for byte."""
import ctypes
import functools
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
    """[(name, bytes)]: the chunk edge, stored and LZMA chunks in one block, matches at the 273 cap, rep0, several blocks"""
    from oracle import codec
    rnd = random.Random(5)
    text = codec.corpus_file(0, 3, (1 << 20) + 12345)
    return [("empty", b""), ("one", b"x"), ("three", text[:3]), ("forty", text[:40]), ("text5k", text[:5000]),
            ("text65536", text[:65536]), ("text65537", text[:65537]), ("random70000", rnd.randbytes(70000)),
            ("random_then_text", rnd.randbytes(200000) + text[:100000]), ("abab", b"ab" * 70000),
            ("zeros2m1", bytes((2 << 20) + 1)), ("text1m12345", text), ("near_stored", near_stored(NEAR_T0, 128))]


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


@functools.lru_cache(maxsize=None)
def model_sequences(name: str, level: int, blk_log: int):
    """(nseq per LZ block, packed sequences) of an input, segment by segment"""
    from oracle import codec
    data = dict(inputs())[name]
    p = lz_params(level, blk_log)
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


@functools.lru_cache(maxsize=None)
def cpu_stream(name: str, level: int = 6, blk_log: int = 16) -> bytes:
    """the encoder core's stream over the model's sequences"""
    data = dict(inputs())[name]
    counts, packed = model_sequences(name, level, blk_log)
    lib = core()
    cap = lib.xze_host_bound(len(data))
    out = ctypes.create_string_buffer(cap)
    ns = (ctypes.c_uint32 * max(len(counts), 1))(*counts)
    sq = (ctypes.c_uint64 * max(len(packed), 1))(*packed)
    n = lib.xze_host_stream(data, len(data), blk_log, sq, ns, out, cap)
    assert n, name
    return out.raw[:n]


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
    data = dict(inputs())[name]
    counts, packed = model_sequences(name, level, blk_log)
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
