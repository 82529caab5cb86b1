"""The .xz streams that tests/test_xz_core.py (CPU) and tests/test_gpu_xz.py (device) decode: one list, built once per process with the stdlib's
lzma -- liblzma, the decoder the reference itself uses -- plus the two multi-block fixtures under tests/golden/xz/ (the module cannot write those)."""
import functools
import lzma
import os
import random

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN_XZ = os.path.join(HERE, "golden", "xz")


def _rand(n: int, seed: int) -> bytes:
    return random.Random(seed).randbytes(n)


def xz(data: bytes, preset: int = 6, check: int = lzma.CHECK_CRC64, filters=None) -> bytes:
    if filters is not None:
        return lzma.compress(data, format=lzma.FORMAT_XZ, check=check, filters=filters)
    return lzma.compress(data, format=lzma.FORMAT_XZ, check=check, preset=preset)


def lzma2(lc: int, lp: int, pb: int, dict_size: int = 65536):
    return [{"id": lzma.FILTER_LZMA2, "preset": 6, "lc": lc, "lp": lp, "pb": pb, "dict_size": dict_size}]


def golden_xz(name: str) -> bytes:
    with open(os.path.join(GOLDEN_XZ, name), "rb") as f:
        return f.read()


@functools.lru_cache(maxsize=None)
def mixed_plain() -> bytes:
    from oracle import codec
    return codec.corpus_file(0, 3, 100000) + _rand(100000, 11) + codec.corpus_file(0, 4, 100000)


@functools.lru_cache(maxsize=None)
def streams():
    """[(name, .xz stream, decoded bytes)] -- every stream liblzma accepts."""
    from oracle import codec
    text5k = codec.corpus_file(0, 1, 5000)
    text300k = codec.corpus_file(0, 7, 300000)
    out = [("empty", xz(b""), b"")]
    for n in (1, 3, 10, 40):
        d = codec.corpus_file(0, 2, 40)[:n]
        out.append(("bytes%d" % n, xz(d), d))
    for preset in (0, 6, 9):
        out.append(("text5k_p%d" % preset, xz(text5k, preset), text5k))
    out.append(("text300k", xz(text300k), text300k))
    out.append(("mixed", xz(mixed_plain()), mixed_plain()))
    for n in (65536, 65537, 200000):
        d = _rand(n, n)
        out.append(("random%d" % n, xz(d), d))
    out.append(("zeros2m1", xz(bytes(2097153)), bytes(2097153)))
    out.append(("abc", xz(b"abc" * 30000), b"abc" * 30000))
    period = _rand(258, 5) * 300
    out.append(("period258", xz(period), period))
    for lc, lp, pb in ((0, 0, 0), (4, 0, 2), (0, 4, 0), (2, 2, 4), (1, 3, 1)):
        out.append(("lc%d_lp%d_pb%d" % (lc, lp, pb), xz(text300k, filters=lzma2(lc, lp, pb)), text300k))
    out.append(("check_none", xz(text5k, check=lzma.CHECK_NONE), text5k))
    out.append(("check_crc32", xz(text5k, check=lzma.CHECK_CRC32), text5k))
    mb = codec.corpus_file(0, 7, 120000)
    out.append(("mb4", golden_xz("mb4.xz"), mb))
    out.append(("mb4_t2", golden_xz("mb4_t2.xz"), mb))
    return out


@functools.lru_cache(maxsize=None)
def unsupported():
    """[(name, stream)] -- well-formed streams outside the format scope: a SHA-256 check, a Delta + LZMA2 chain."""
    from oracle import codec
    text5k = codec.corpus_file(0, 1, 5000)
    return [("sha256", xz(text5k, check=lzma.CHECK_SHA256)),
            ("delta_lzma2", xz(text5k, filters=[{"id": lzma.FILTER_DELTA, "dist": 1}, {"id": lzma.FILTER_LZMA2, "preset": 6}]))]


def damage_cases(stream: bytes):
    """[(name, damaged stream)]: the ways the `mixed` stream is damaged -- nine bit flips, five truncations."""
    n = len(stream)
    out = []
    for at in (7, 13, 30, n // 4, n // 2, 3 * n // 4, n - 20, n - 6, n - 1):
        b = bytearray(stream)
        b[at] ^= 0x10
        out.append(("flip@%d" % at, bytes(b)))
    for cut in (1, 4, 12, 28, n // 2):
        out.append(("cut%d" % cut, stream[:n - cut]))
    return out


def liblzma_refuses(stream: bytes) -> bool:
    """liblzma's verdict on a stream read to its end, as the reference reads an entry."""
    try:
        d = lzma.LZMADecompressor(format=lzma.FORMAT_XZ)
        d.decompress(stream)
        return not d.eof or bool(d.unused_data)
    except lzma.LZMAError:
        return True
