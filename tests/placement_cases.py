"""What tests/test_placement_cases.py (CPU) and tests/test_gpu_decode_placement.py (device) share: the plain inputs, the foreign writers' streams of
every codec, and the layouts -- where the streams and the rooms of one decode call lie in their buffers.  The device decoders take raw byte offsets
(include/pna_gpu.h, "Placement" at pna_gpu_decompress_batch_device); the layouts here pack streams and rooms without padding, at every residue mod 16,
between guard bands.  The expected bytes of a stream are always its plain input; the streams of this library's own encoder need a device and are made in
the device test.  Everything is built once per process."""
import functools
import lzma
import random
import struct
import zlib

from xz_cases import golden_xz, lzma2, xz

GUARD = 4096          # guard band in front of and behind every destination buffer, and in front of every source buffer
SRC_SLACK = 15        # readable bytes behind the last stream of a source buffer: what include/pna_gpu.h documents
MIB = 1 << 20
TEXT_LENGTHS = (0, 1, 2, 3, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 4095, 4097, 65537, 131071, 131073)
XZ_MAX = 300001       # one wave decodes ~2 MiB/s of LZMA2: no xz case is larger
RESIDUES = tuple((rd % 4, rd) for rd in range(16))                  # (rs, rd) of a codec's default form
FEW_RESIDUES = ((0, 0), (1, 1), (3, 13), (2, 8), (1, 15))           # ... of the other forms


def _rand(n: int, seed: int) -> bytes:
    return random.Random(seed).randbytes(n)


@functools.lru_cache(maxsize=None)
def plains():
    """[(name, bytes)]: the smallest shapes that reach every store width, every tail, the 128 KiB block / piece edge and the 1 MiB frame edge."""
    from oracle import codec
    out = [("text%d" % n, codec.corpus_file(0, 7100 + n % 97, n)) for n in TEXT_LENGTHS]
    out.append(("zeros70001", bytes(70001)))                                            # matches at distance 1
    out.append(("period7", (_rand(7, 3) * (50003 // 7 + 1))[:50003]))                    # overlapping copies, distance below 8
    out.append(("random33331", _rand(33331, 5)))                                         # raw blocks, stored blocks, uncompressed chunks
    out.append(("text300001", codec.corpus_file(0, 7201, 300001)))                       # three zstd blocks, three inflate pieces, two xz check pieces
    out.append(("text1m4099", codec.corpus_file(0, 7202, MIB + 4099)))                   # two frames of the grid, nine sync-flush pieces
    return out


def plain(name: str) -> bytes:
    return dict(plains())[name]


# ---- zstd: the system libzstd's frames (None when it is absent: the callers skip as the other tests do)
def have_libzstd() -> bool:
    from oracle import codec
    return codec.system_libzstd() is not None


def _libzstd_frame(data: bytes, level: int, checksum: bool) -> bytes:
    from oracle import codec
    return codec.libzstd_compress_checksum(data, level) if checksum else codec.libzstd_compress(data, level)


@functools.lru_cache(maxsize=None)
def zstd_foreign(level: int, checksum: bool):
    """[(name, frame, plain)]: one libzstd frame per plain input."""
    return [("%s_l%d%s" % (n, level, "_chk" if checksum else ""), _libzstd_frame(d, level, checksum), d) for n, d in plains()]


def skippable(k: int) -> bytes:
    body = bytes((7 * i + k) & 0xFF for i in range((0, 1, 7, 300)[k % 4]))
    return struct.pack("<II", 0x184D2A50 + (k % 16), len(body)) + body


@functools.lru_cache(maxsize=None)
def zstd_frame_list():
    """(name, payload, plain): three libzstd frames (levels 1, 3, 19; the middle one with a checksum) with a skippable frame between them -- a payload
    the frame placer cannot take, so its frames are listed one by one (k_zlist)."""
    d = plain("text300001")
    cuts = (0, 70001, 200003, len(d))
    fr = [_libzstd_frame(d[cuts[k]:cuts[k + 1]], (1, 3, 19)[k], k == 1) for k in range(3)]
    return ("frame_list", fr[0] + skippable(3) + fr[1] + skippable(2) + fr[2], d)


def zstd_cpu_decode(stream: bytes, n: int) -> bytes:
    """The independent decoders: oracle/zstd_dec.c, and the system libzstd when present -- they must agree."""
    from oracle import codec
    got = codec.zstd_decompress(stream, n)
    if have_libzstd():
        assert codec.libzstd_decompress_stream(stream, n) == got
    return got


def zstd_cpu_refuses(stream: bytes, n: int) -> bool:
    from oracle import codec
    try:
        if have_libzstd():
            codec.libzstd_decompress_stream(stream, n)
        else:
            codec.zstd_decompress(stream, n)
        return False
    except ValueError:                                                  # what both decoders' wrappers raise for a stream their decoder refuses
        return True


# ---- deflate: the stdlib's zlib
def _z(data: bytes, level: int = 6, strategy: int = zlib.Z_DEFAULT_STRATEGY, wbits: int = 15) -> bytes:
    c = zlib.compressobj(level, zlib.DEFLATED, wbits, 8, strategy)
    return c.compress(data) + c.flush()


DEFLATE_WRITERS = {"z1": dict(level=1), "z6": dict(level=6), "z9": dict(level=9), "fixed": dict(strategy=zlib.Z_FIXED), "huff": dict(strategy=zlib.Z_HUFFMAN_ONLY),
                   "stored": dict(level=0), "w9": dict(wbits=9)}


@functools.lru_cache(maxsize=None)
def deflate_foreign(writer: str):
    """[(name, zlib stream, plain)]: one stream per plain input."""
    return [("%s_%s" % (n, writer), _z(d, **DEFLATE_WRITERS[writer]), d) for n, d in plains()]


@functools.lru_cache(maxsize=None)
def deflate_large():
    """(name, stream, plain): `zlib -6` over 1.5 MiB of text -- well above the 8 x 16 KiB of compressed bytes the chunk decoder asks for."""
    from oracle import codec
    d = codec.corpus_file(0, 7301, MIB) + codec.corpus_file(0, 7302, MIB // 2)
    return ("text1m5_z6", _z(d, 6), d)


def deflate_cpu_refuses(stream: bytes) -> bool:
    try:
        d = zlib.decompressobj()
        d.decompress(stream)
        return not d.eof
    except zlib.error:
        return True


# ---- xz: the stdlib's lzma (liblzma)
@functools.lru_cache(maxsize=None)
def xz_streams():
    """[(name, .xz stream, plain)]"""
    out = []
    for preset in (0, 6):
        out += [("%s_p%d" % (n, preset), xz(d, preset), d) for n, d in plains() if len(d) <= XZ_MAX]
    t = plain("text300001")
    out.append(("text300001_none", xz(t, check=lzma.CHECK_NONE), t))
    out.append(("text300001_crc32", xz(t, check=lzma.CHECK_CRC32), t))                   # CRC32 over more than one 256 KiB check piece
    out.append(("text300001_crc64", xz(t, 1, check=lzma.CHECK_CRC64), t))
    out.append(("text300001_lp4", xz(t, filters=lzma2(0, 4, 0)), t))
    from oracle import codec
    mb = codec.corpus_file(0, 7, 120000)
    out.append(("mb4", golden_xz("mb4.xz"), mb))
    out.append(("mb4_t2", golden_xz("mb4_t2.xz"), mb))
    return out


def xz_cpu_decode(stream: bytes) -> bytes:
    return lzma.decompress(stream, format=lzma.FORMAT_XZ)


def flip_middle(stream: bytes) -> bytes:
    b = bytearray(stream)
    b[len(b) // 2] ^= 0x10
    return bytes(b)


# ---- layouts
class Layout:
    """Where n streams lie in a source buffer and n rooms in a destination buffer.  guards: the byte ranges of the destination buffer outside every room
    (front band, gaps, back band); src_gaps: the ranges of the source buffer outside every stream (front band, gaps, the slack behind the last stream)."""

    def __init__(self, name, src_off, src_len, dst_off, raw_len, src_size, dst_size):
        self.name, self.src_off, self.src_len, self.dst_off, self.raw_len = name, list(src_off), list(src_len), list(dst_off), list(raw_len)
        self.src_size, self.dst_size = src_size, dst_size
        self.guards = _complement(self.dst_off, self.raw_len, dst_size)
        self.src_gaps = _complement(self.src_off, self.src_len, src_size)


def _complement(off, length, size):
    out, pos = [], 0
    for a, n in sorted(zip(off, length)):
        if n == 0:
            continue
        if a > pos:
            out.append((pos, a))
        pos = max(pos, a + n)
    if pos < size:
        out.append((pos, size))
    return out


def _pack(lengths, first, gap, order=None):
    """offsets of ranges of the given lengths laid out from `first` in `order`, gap(k) bytes in front of the k-th range laid (k >= 1)"""
    order = list(range(len(lengths))) if order is None else order
    off, pos = [0] * len(lengths), first
    for k, i in enumerate(order):
        if k:
            pos += gap(k)
        off[i] = pos
        pos += lengths[i]
    return off, pos


def _layout(name, src_len, raw_len, rs, rd, gap, order=None):
    so, s_end = _pack(src_len, GUARD + rs, gap)
    do, d_end = _pack(raw_len, GUARD + rd, gap, order)
    return Layout(name, so, src_len, do, raw_len, s_end + SRC_SLACK, d_end + GUARD)


def tight(src_len, raw_len, rs, rd):
    """streams back to back from residue rs, rooms back to back from residue rd: no padding anywhere (an empty entry shares its offset with its successor)"""
    return _layout("tight(%d,%d)" % (rs, rd), src_len, raw_len, rs, rd, lambda k: 0)


def gapped(src_len, raw_len, rs, rd):
    """gaps of 1 + (7 i) % 15 bytes between streams and between rooms"""
    return _layout("gapped(%d,%d)" % (rs, rd), src_len, raw_len, rs, rd, lambda k: 1 + (7 * k) % 15)


def permutation(n: int, seed: int = 20240607):
    p = list(range(n))
    random.Random(seed).shuffle(p)
    return p


def permuted(src_len, raw_len, rd):
    """tight rooms handed out in a fixed seeded permutation of the entries: dst_off is not monotonic in the entry index"""
    return _layout("permuted(%d)" % rd, src_len, raw_len, rd % 4, rd, lambda k: 0, permutation(len(raw_len)))

