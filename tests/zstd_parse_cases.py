"""The inputs of tests/test_zstd_parse_core.py (CPU) and tests/test_gpu_zstd_parse_routes.py (device): plain texts, their zstd streams from five writers
-- the system libzstd at levels 1, 3, 19 and at 3 with a checksum, and this repository's encoder model --, and the damage list.

The streams that carry the rare header branches (direct Huffman weights, a single Huffman stream, a block without sequences, RLE mode for each of the
three tables, treeless literals, raw literals with a 3-byte header, an RLE block, every content-size form up to 4 bytes) are committed under
tests/golden/zstd_parse/ -- `python tests/zstd_parse_cases.py --write` made them with libzstd 1.4.8 --, so that what the tests reach does not depend
on the libzstd of the machine; their plain texts are regenerated from the recipe here.  Everything is built once per process."""
import functools
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden", "zstd_parse")
MIB = 1 << 20
WRITERS = ("l1", "l3", "l19", "l3chk", "model")


@functools.lru_cache(maxsize=None)
def common_plains():
    from oracle import codec
    return [("text300k", codec.corpus_file(0, 7106, 300 << 10)), ("kind1_200000", codec.corpus_file(1, 7102, 200000)),
            ("kind2_50000", codec.corpus_file(2, 7103, 50000)), ("text1m5000", codec.corpus_file(0, 7104, MIB + 5000)),
            ("hello", b"hello hello hello"), ("zeros300000", bytes(300000)), ("empty", b""), ("bytes256x40", bytes(range(256)) * 40)]


@functools.lru_cache(maxsize=None)
def rare_plains():
    r = random.Random(5)                                               # (the draws below in this order)
    out = [("skew12x600", bytes(r.choices(range(12), weights=[50, 20, 10, 5, 4, 3, 2, 2, 1, 1, 1, 1], k=600)))]      # direct weights, one Huffman stream
    out.append(("skew6x200", bytes(r.choices(range(6), weights=[50, 20, 10, 5, 4, 3], k=200))))                      # a block without sequences
    out.append(("skew40x5000", bytes(r.choices(range(40), weights=[2 ** (10 - i // 4) for i in range(40)], k=5000))))   # RLE mode for ML
    out.append(("period13x20000", b"".join(bytes([r.randrange(256)]) + b"0123456789AB" for _ in range(20000))))      # RLE mode for LL and OF, treeless
    return out                                                                                                        # literals, raw literals with 3 header bytes


@functools.lru_cache(maxsize=None)
def fixture_plains():
    """a text for the fixtures alone: the start of the 300 KiB text, short enough to commit its streams (a literals section with a 5-byte header)"""
    return [("text64k", dict(common_plains())["text300k"][:64 << 10])]


# the committed streams: every writer's stream of every rare text, of the small common texts (the RLE block, the 0- and 1-byte content sizes) and of the
# first 64 KiB of the 300 KiB text (a literals section with a 5-byte header)
FIXTURE_PLAINS = ("skew12x600", "skew6x200", "skew40x5000", "period13x20000", "hello", "zeros300000", "empty", "bytes256x40", "text64k")


def plain(name: str) -> bytes:
    return dict(common_plains() + rare_plains() + fixture_plains())[name]


def write(data: bytes, writer: str) -> bytes:
    from oracle import codec
    if writer == "model":
        return codec.model_compress(data)
    if writer == "l3chk":
        return codec.libzstd_compress_checksum(data, 3)
    return codec.libzstd_compress(data, int(writer[1:]))


@functools.lru_cache(maxsize=None)
def fixtures():
    """[(name, stream, plain)]: the committed streams, in name order, and three of them in one payload with skippable frames in front and between"""
    import placement_cases as P
    out = []
    for f in sorted(os.listdir(GOLDEN)):
        with open(os.path.join(GOLDEN, f), "rb") as h:
            out.append((f[:-4], h.read(), plain(f[:-4].rsplit("_", 1)[0])))
    by = {n: (s, d) for n, s, d in out}
    parts = [by["skew12x600_l1"], by["hello_l3chk"], by["skew40x5000_model"]]
    out.append(("fixture_frame_list", P.skippable(1) + parts[0][0] + P.skippable(3) + parts[1][0] + P.skippable(0) + parts[2][0], b"".join(d for _, d in parts)))
    return out


@functools.lru_cache(maxsize=None)
def streams():
    """[(name, stream, plain)]: the fixtures, the model's stream of every text, libzstd's where the system has one, and a list of frames with skippable
    frames between them"""
    import placement_cases as P
    have = P.have_libzstd()
    out = list(fixtures())
    for n, d in common_plains():
        if n not in FIXTURE_PLAINS:
            out += [("%s_%s" % (n, w), write(d, w), d) for w in WRITERS if have or w == "model"]
    if have:
        out.append(P.zstd_frame_list())
    return out


def damage_cases(stream: bytes, lengths=tuple(range(40))):
    """[(name, damaged stream)]: the frame header's descriptor bit by bit and with the reserved bit and a dictionary id at once, every byte up to 39 (block
    header, literals header, tree description), cuts at the given lengths below 40 and at 2/3, and bytes behind the end"""
    def x(at, mask):
        return stream[:at] + bytes([stream[at] ^ mask]) + stream[at + 1:]
    out = [("byte4^%02x" % (1 << k), x(4, 1 << k)) for k in range(8)]
    out.append(("byte4^0b", x(4, 0x0B)))
    out += [("byte%d^5a" % at, x(at, 0x5A)) for at in range(5, 40) if at < len(stream)]
    out += [("cut@%d" % n, stream[:n]) for n in lengths if n < len(stream)]
    out.append(("cut@2/3", stream[:len(stream) * 2 // 3]))
    out.append(("trailing", stream + bytes(4)))
    return out


if __name__ == "__main__":
    if sys.argv[1:] != ["--write"]:
        sys.exit("usage: zstd_parse_cases.py --write   (writes tests/golden/zstd_parse/ with this machine's libzstd)")
    os.makedirs(GOLDEN, exist_ok=True)
    for name in FIXTURE_PLAINS:
        for w in WRITERS:
            with open(os.path.join(GOLDEN, "%s_%s.zst" % (name, w)), "wb") as h:
                h.write(write(plain(name), w))
            print(name, w, os.path.getsize(h.name))
