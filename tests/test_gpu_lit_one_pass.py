"""The literal coder's two forms (k_lit / k_write): one pass into four regions of the block's litc slot, spliced by k_write, and the two-pass
form for blocks whose regions do not fit.  Hand-built entries of two blocks: block 0 is text and carries the segment's Huffman tree; block 1 is made of
pieces that block 0 holds, each found as one match, with single bytes between them -- its literals -- or of a run that nothing matches, then matches.
That sets block 1's literal count, and which bytes the literals are; the oracle's LZ model confirms both in every case.  Every case is checked against the
model, byte for byte, and read back by the device decoder, at 128 KiB blocks (the large-batch form) and at 16 KiB blocks (the latency mode), where it also
goes through the CompressionWriter seam.

Which of the two forms a block took cannot be seen from outside (BlkInfo has no accessor beyond debug_block's counts): the cases at the threshold compute the
literal counts on either side of the region rule here and assert the counts and the bytes."""
import heapq
import random

import pytest

from conftest import headline_context

pytestmark = pytest.mark.gpu

BLK_LOGS = (17, 14)


def lit_regions(nlit, maxbits):
    """pna_dev.h lit_regions: the bytes the four (one below 256 literals) regions take."""
    ns = 4 if nlit >= 256 else 1
    segsz = (nlit + 3) // 4 if ns == 4 else nlit
    ms = [segsz, segsz, segsz, nlit - 3 * segsz] if ns == 4 else [nlit]
    return sum(((m * maxbits + 7) // 8 + 9 + 15) & ~15 for m in ms)


def largest_fit(bs, maxbits):
    n = bs
    while lit_regions(n, maxbits) > bs:
        n -= 1
    return n


def blocks_of(frame):
    """(block type, literals type, literal count, [bits of every Huffman stream]) of each block of one frame as the encoder writes it."""
    assert frame[:6] == bytes([0x28, 0xB5, 0x2F, 0xFD, 0x00, 0x50])
    pos, out = 6, []
    while True:
        h = int.from_bytes(frame[pos:pos + 3], "little")
        last, btype, size = h & 1, (h >> 1) & 3, h >> 3
        pos += 3
        if btype != 2:
            out.append((btype, None, None, []))
        else:
            b = frame[pos:pos + size]
            lt, sf = b[0] & 3, (b[0] >> 2) & 3
            if lt < 2:
                nlit = b[0] >> 3 if sf in (0, 2) else (int.from_bytes(b[:2], "little") >> 4 if sf == 1 else int.from_bytes(b[:3], "little") >> 4)
                out.append((2, lt, nlit, []))
            else:
                lh, nb = (3, 10) if sf < 2 else ((4, 14) if sf == 2 else (5, 18))
                v = int.from_bytes(b[:lh], "little")
                nlit, comp = (v >> 4) & ((1 << nb) - 1), (v >> (4 + nb)) & ((1 << nb) - 1)
                p = lh
                if lt == 2:
                    p += 1 + (b[lh] if b[lh] < 128 else (b[lh] - 127 + 1) // 2)
                body = b[p:lh + comp]
                if sf == 0:
                    streams = [body]
                else:
                    sz = [int.from_bytes(body[2 * k:2 * k + 2], "little") for k in range(3)]
                    streams, q = [], 6
                    for s in sz + [len(body) - 6 - sum(sz)]:
                        streams.append(body[q:q + s]); q += s
                out.append((2, lt, nlit, [8 * (len(s) - 1) + s[-1].bit_length() - 1 for s in streams]))
        pos += size if btype != 1 else 1
        if last:
            return out


def huffman_depth(counts):
    """Depth of the unlimited Huffman code of a histogram: from 11 on, the encoder's length-limited code reaches 11 bits."""
    h = [(c, 0) for c in counts if c]
    heapq.heapify(h)
    while len(h) > 1:
        (a, da), (b, db) = heapq.heappop(h), heapq.heappop(h)
        heapq.heappush(h, (a + b, max(da, db) + 1))
    return h[0][1]


class Maker:
    def __init__(self, codec, blk_log):
        self.codec, self.blk_log, self.bs = codec, blk_log, 1 << blk_log
        self.p = codec.params_for_level(3, blk_log=0 if blk_log == 17 else blk_log)
        self.per = 4096 if blk_log == 17 else 2048
        text = bytearray(codec.corpus_file(0, 77, self.bs))
        for i in range(8):
            text[1000 * (i + 1) + 3] = 240 + i                          # eight bytes that occur once: the segment's code reaches the longest length (huffman_depth)
        self.text = bytes(text)
        self.b0 = self.text[:self.bs - self.per] + self.text[:self.per]

    def model_lits(self, data):
        return [l for _, l in self.codec.model_lz_segment(data, self.p)]

    def separated(self, seps):
        """Block 1 = 31-byte pieces of block 0's tail (which repeats no 3-gram: each piece is found whole), one byte of `seps` before each -- its literals --,
        then matches to the end."""
        chunk, n = 32, len(seps)
        g = self.counter_run(n * chunk + 64)
        b1 = b"".join(seps[i:i + 1] + g[2 + chunk * i:2 + chunk * i + chunk - 1] for i in range(n))
        return self.text[:self.bs - len(g)] + g + b1 + (g * (self.bs // len(g) + 1))[:self.bs - len(b1)]

    def letters(self, n, seed):
        rnd = random.Random(seed)
        return bytes(rnd.choice(b"etaoinshrdlu ") for _ in range(n))

    def with_nlit(self, target):
        """Letters of the text as separators; one that continues the piece before it joins that match, so their number is corrected until the model counts `target`."""
        n = target
        for seed in range(16):
            data = self.separated(self.letters(n, target + seed))
            got = len(self.model_lits(data)[1])
            if got == target:
                return data
            n += target - got
        raise AssertionError("no set of separators gives %d literals" % target)

    def counter_run(self, n):
        """n bytes without a repeated 3-gram and with one dominant symbol: Huffman wins on them, and no match shortens the run."""
        g = bytearray()
        for i in range((n + 2) // 3):
            g += bytes([255, i // 220, i % 220])
        return bytes(g[:n])

    def run_then_matches(self, run_of, target):
        """Block 1 = a run of literals, then the period repeated; the run's length is corrected until the model counts `target` literals."""
        n = target
        for _ in range(8):
            data = self.b0 + run_of(n) + (self.text[:self.per] * (self.bs // self.per + 1))[:self.bs - n]
            got = len(self.model_lits(data)[1])
            if got == target:
                return data
            n += target - got
        raise AssertionError("no run gives %d literals" % target)


_cases = {}


def cases(codec, blk_log):
    """name -> (entry, literal count of block 1, literals type of block 1: 0 raw, 1 RLE, 3 Huffman with block 0's tree); built once per block size."""
    if blk_log in _cases:
        return _cases[blk_log]
    m, c = Maker(codec, blk_log), {}
    for n in (63, 64, 255, 256, 257, 259, 261):
        c["n%d" % n] = (m.with_nlit(n), n, 0 if n < 64 else 3)
    # a stream of 64 k bits (the closing bit opens a qword) and one of 64 k - 1 (it fills the last one): search the seeds with the model
    want = {0: None, 63: None}
    for seed in range(1000, 1400):
        d = m.separated(m.letters(256 + seed % 40, seed))
        for bits in blocks_of(codec.model_compress(d, m.p))[1][3]:
            if bits % 64 in want and want[bits % 64] is None:
                want[bits % 64] = (d, len(m.model_lits(d)[1]), 3)
        if all(want.values()):
            break
    c["bits64k"], c["bits64k-1"] = want[0], want[63]
    for name, seps, lit_type in (("rle", b"e" * 300, 1), ("rle_but_one", b"e" * 157 + b"t" + b"e" * 142, 3)):
        d = m.separated(seps)
        lits = m.model_lits(d)[1]
        assert len(lits) >= 256 and sorted(set(lits)) == sorted(set(seps))
        c[name] = (d, len(lits), lit_type)
    # random bytes over 5/8 of the block: their regions fit the slot at any code length (11 bits x 5/8 < 8), they are coded, and Huffman cannot win
    rnd = random.Random(4)
    nu = m.bs * 5 // 8
    assert lit_regions(nu, 11) <= m.bs
    c["uniform"] = (m.run_then_matches(lambda n: bytes(rnd.getrandbits(8) for _ in range(n)), nu), nu, 0)
    fit = largest_fit(m.bs, 11)
    assert lit_regions(fit, 11) <= m.bs < lit_regions(fit + 1, 11) and 256 <= fit < m.bs
    c["fit11"] = (m.run_then_matches(m.counter_run, fit), fit, 3)
    c["fit11+1"] = (m.run_then_matches(m.counter_run, fit + 1), fit + 1, 3)
    c["full11"] = (m.b0 + m.counter_run(m.bs), m.bs, 3)
    _cases[blk_log] = c
    return c


NAMES = ["n63", "n64", "n255", "n256", "n257", "n259", "n261", "bits64k", "bits64k-1", "rle", "rle_but_one", "uniform", "fit11", "fit11+1", "full11"]


@pytest.fixture(scope="module")
def ctxs(pna):
    import torch  # noqa: F401
    big, lat = headline_context(pna), pna.Context(0)
    lat.set_option("blk_log", 14)
    yield {17: big, 14: lat}
    big.close()
    lat.close()


@pytest.mark.parametrize("blk_log", BLK_LOGS)
@pytest.mark.parametrize("name", NAMES)
def test_block_shapes(pna, codec, ctxs, name, blk_log):
    case = cases(codec, blk_log)[name]
    assert case is not None, "the model finds no such stream among the seeds"
    data, nlit, lit_type = case
    m, ctx = Maker(codec, blk_log), ctxs[blk_log]
    lits = m.model_lits(data)
    assert len(lits) == 2 and len(lits[1]) == nlit                      # the premise: block 1 has exactly the literals the case is about
    expect = codec.model_compress(data, m.p)
    blocks = blocks_of(expect)
    assert blocks[1][:3] == (2, lit_type, nlit)                         # raw below 64 literals and where Huffman cannot win, RLE, or Huffman without a tree of its own
    if lit_type == 3:
        assert len(blocks[1][3]) == (4 if nlit >= 256 else 1)
    if name == "bits64k":
        assert any(b % 64 == 0 for b in blocks[1][3])
    if name == "bits64k-1":
        assert any(b % 64 == 63 for b in blocks[1][3])
    if name in ("fit11", "fit11+1", "full11"):
        hist = [0] * 256
        for l in lits:
            for s in l:
                hist[s] += 1
        assert huffman_depth(hist) >= 11                                # the segment's code reaches maxbits = 11: the region rule was evaluated at it
    (out,) = ctx.compress_batch([data])
    assert ctx.timing().blk_log == blk_log
    assert len(ctx.debug_block(1)[1]) == nlit
    assert out == expect
    assert ctx.decompress_batch([out], [len(data)]) == [data]
    if blk_log == 14:
        parts = []

        class Sink:
            def write(self, b): parts.append(bytes(b))
        w = ctx.writer(Sink())
        w.write(data)
        w.try_into_inner()
        sp = codec.params_for_level(3, blk_log=ctx.timing().blk_log)
        assert b"".join(parts) == codec.model_compress(data, sp)


@pytest.mark.parametrize("blk_log", BLK_LOGS)
@pytest.mark.parametrize("kind", [0, 1])
def test_corpus_entry(pna, codec, ctxs, kind, blk_log):
    """An ordinary 1 MiB entry of the synthetic corpus, enwik-style and random text."""
    data = codec.corpus_file(kind, 4242, 1 << 20)
    ctx = ctxs[blk_log]
    (out,) = ctx.compress_batch([data])
    assert ctx.timing().blk_log == blk_log
    assert out == codec.model_compress(data, codec.params_for_level(3, blk_log=0 if blk_log == 17 else blk_log))
    assert ctx.decompress_batch([out], [len(data)]) == [data]
