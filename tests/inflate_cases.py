"""Hand-built deflate streams (RFC 1950 / 1951) for the device inflate decoders: a small deflate WRITER for tests and the case list that
tests/test_inflate_cases.py (CPU: every verdict against the system zlib) and tests/test_gpu_inflate_conformance.py (device) share.  The streams reach what
no encoder in the suite emits: second-level tables full of sub-tables, single-code and empty code sets, repeat symbols across the HLIT | HDIST boundary,
length 258 as symbol 284 + 31, literal runs at the record split, stored headers at every bit phase, re-seats of the reader at ring edges, pieces in this
library's layout that are not this library's, and the streams zlib refuses.  Pure Python, deterministic, built on first use (no fixtures are committed).

A case is (name, stream, plain or None, properties); plain is None when zlib must refuse the stream.  A token is a literal (int) or (length, distance);
("raw", value, nbits) puts bits as they are (refused streams only)."""
import bisect
import functools
import random
import struct
import zlib

LBASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEXT = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
LTOP = [b + (1 << e) - 1 for b, e in zip(LBASE, LEXT)]
LTOP[27] = 257                                                       # (227 + 31 = 258 is the other spelling of length 258)
DBASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577]
DEXT = [0, 0, 0, 0] + [(k >> 1) - 1 for k in range(4, 30)]
DTOP = [b + (1 << e) - 1 for b, e in zip(DBASE, DEXT)]
ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_D = [5] * 32
BLK = 1 << 17                                                        # this library's piece: 128 KiB of output
LL_SPLIT = 1 << 17                                                   # IF_LL_SPLIT of k_inflate.hip


# ---------------------------------------------------------------------------------------------------- the writer
class BitWriter:
    """LSB first, as RFC 1951 packs bits into bytes"""

    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def put(self, v, nbits):
        self.acc |= v << self.n
        self.n += nbits
        if self.n >= 64:
            k = self.n >> 3
            self.out += (self.acc & ((1 << (8 * k)) - 1)).to_bytes(k, "little")
            self.acc >>= 8 * k
            self.n -= 8 * k

    def bitpos(self):
        return len(self.out) * 8 + self.n

    def align(self):
        if self.n & 7:
            self.put(0, 8 - (self.n & 7))
        self.out += self.acc.to_bytes(self.n >> 3, "little")
        self.acc, self.n = 0, 0

    def raw(self, data):
        self.align()
        self.out += data


def canon(lens):
    """canonical codes of a list of code lengths: per symbol (code with its first bit lowest, length) or None.  (Sets zlib refuses get codes too.)"""
    cnt = [0] * 17
    for l in lens:
        cnt[l] += 1
    cnt[0] = 0
    nxt, code = [0] * 17, 0
    for L in range(1, 16):
        code = (code + cnt[L - 1]) << 1
        nxt[L] = code
    out = []
    for l in lens:
        if not l:
            out.append(None)
            continue
        c = nxt[l] & ((1 << l) - 1)
        nxt[l] += 1
        out.append((int(format(c, "0%db" % l)[::-1], 2), l))
    return out


def kraft(lens):
    """sum of 2^-len in units of 2^-15: 32768 for a complete set"""
    return sum(32768 >> l for l in lens if l)


def prefixes(lens, root):
    """the distinct `root`-bit prefixes that carry codes longer than `root` bits (= second-level tables of a decoder with a root table of that size)"""
    cnt = [0] * 17
    for l in lens:
        cnt[l] += 1
    cnt[0] = 0
    nxt, code = [0] * 17, 0
    for L in range(1, 16):
        code = (code + cnt[L - 1]) << 1
        nxt[L] = code
    seen = set()
    for l in lens:
        if l:
            if l > root:
                seen.add(nxt[l] >> (l - root))
            nxt[l] += 1
    return len(seen)


def len_code(l, alt258=False):
    """(symbol, extra bits, extra value) of a match length"""
    if l == 258:
        return (284, 5, 31) if alt258 else (285, 0, 0)
    i = bisect.bisect_right(LBASE, l, 0, 28) - 1
    return 257 + i, LEXT[i], l - LBASE[i]


def dist_code(d):
    i = bisect.bisect_right(DBASE, d) - 1
    return i, DEXT[i], d - DBASE[i]


def put_tokens(w, tokens, lc, dc, alt258=False):
    put = w.put
    for t in tokens:
        if type(t) is int:
            put(*lc[t])
        elif t[0] == "raw":
            put(t[1], t[2])
        else:
            s, eb, ev = len_code(t[0], alt258)
            put(*lc[s])
            if eb:
                put(ev, eb)
            s, eb, ev = dist_code(t[1])
            put(*dc[s])
            if eb:
                put(ev, eb)


def play_into(buf, tokens):
    for t in tokens:
        if type(t) is int:
            buf.append(t)
        elif t[0] != "raw":
            l, d = t
            s = len(buf) - d
            assert s >= 0 and 3 <= l <= 258 and 1 <= d <= 32768, t
            if d >= l:
                buf += buf[s:s + l]
            else:
                buf += (bytes(buf[s:]) * (l // d + 1))[:l]


def play(tokens, prefix=b""):
    """the plain bytes of a token list (behind `prefix`, which matches may reach into)"""
    buf = bytearray(prefix)
    play_into(buf, tokens)
    return bytes(buf[len(prefix):])


def cl_symbols(lens, strategy):
    """the code lengths as code-length symbols [(symbol, extra bits, extra value)]: "none" = one symbol per length; "greedy" = 16 / 17 / 18 over the
    array as it stands (the caller passes literal / length and distance lengths JOINED, so runs cross the boundary between them)"""
    if strategy == "none":
        return [(l, 0, 0) for l in lens]
    out, i, n = [], 0, len(lens)
    while i < n:
        v, j = lens[i], i
        while j < n and lens[j] == v:
            j += 1
        run = j - i
        if v == 0:
            while run >= 11:
                r = min(run, 138)
                out.append((18, 7, r - 11))
                run -= r
            if run >= 3:
                out.append((17, 3, run - 3))
                run = 0
        else:
            out.append((v, 0, 0))
            run -= 1
            while run >= 3:
                r = min(run, 6)
                out.append((16, 2, r - 3))
                run -= r
        out += [(v, 0, 0)] * run
        i = j
    return out


def crosses(syms, hlit):
    """does a repeat symbol of `syms` cover code lengths on both sides of position hlit"""
    n = 0
    for s, _, ev in syms:
        rep = 1 if s < 16 else (3 + ev if s < 18 else 11 + ev)
        if s >= 16 and n < hlit < n + rep:
            return s
        n += rep
    return 0


def flat_code(nsym):
    """the lengths (a multiset, shortest first) of a complete code of nsym >= 2 symbols that uses two adjacent lengths"""
    k = nsym.bit_length() - 1
    short = (2 << k) - nsym
    return [k] * short + [k + 1] * (nsym - short)


def clc_for(syms):
    """a complete code-length code (19 lengths) over the symbols in use, the frequent ones shortest"""
    freq = {}
    for s, _, _ in syms:
        freq[s] = freq.get(s, 0) + 1
    used = sorted(freq, key=lambda s: (-freq[s], s))
    if len(used) == 1:                                              # a single code of one bit is not a complete code-length code: zlib refuses it
        used.append(0 if used[0] != 0 else 1)
    clc = [0] * 19
    for s, l in zip(used, flat_code(len(used))):
        clc[s] = l
    return clc


def raw_header(w, final, hlit_field, hdist_field, clc, syms, hclen=None):
    """a dynamic block's header from its fields as given (any values: refused streams are written with it too)"""
    if hclen is None:
        hclen = max([4] + [i + 1 for i in range(19) if clc[ORDER[i]]])
    w.put(final, 1)
    w.put(2, 2)
    w.put(hlit_field, 5)
    w.put(hdist_field, 5)
    w.put(hclen - 4, 4)
    for i in range(hclen):
        w.put(clc[ORDER[i]], 3)
    cc = canon(clc)
    for s, eb, ev in syms:
        w.put(*cc[s])
        if eb:
            w.put(ev, eb)
    return hclen


class Z:
    """one zlib stream under construction: blocks are appended, `plain` follows"""

    def __init__(self, cmf=0x78):
        self.w, self.plain, self.info = BitWriter(), bytearray(), []
        self.w.put(cmf, 8)
        self.w.put((31 - (cmf << 8) % 31) % 31, 8)

    def stored(self, data, final=0, nlen=None, len_field=None):
        self.info.append(("stored", self.w.bitpos()))
        self.w.put(final, 1)
        self.w.put(0, 2)
        n = len(data) if len_field is None else len_field
        self.w.raw(struct.pack("<HH", n, (n ^ 0xFFFF) if nlen is None else nlen) + bytes(data))
        self.plain += data
        return self

    def fixed(self, tokens, final=0, eob=True, played=True, end_phase=None):
        self.info.append(("fixed", self.w.bitpos()))
        self.w.put(final, 1)
        self.w.put(1, 2)
        lc = canon(FIXED_LL)
        put_tokens(self.w, tokens, lc, canon(FIXED_D))
        tokens = list(tokens)
        while end_phase is not None and (self.w.bitpos() + 7) % 8 != end_phase:      # (a 9-bit literal moves the end on by one bit)
            self.w.put(*lc[200])
            tokens.append(200)
        if eob:
            self.w.put(*lc[256])
        if played:
            play_into(self.plain, tokens)
        return self

    def fixed_raw(self, items, final=0):
        """a fixed block from (code, nbits) pairs: Huffman codes as RFC 1951 prints them (first bit highest); (value, nbits, "extra") = extra bits"""
        self.info.append(("fixed", self.w.bitpos()))
        self.w.put(final, 1)
        self.w.put(1, 2)
        for it in items:
            if len(it) == 3:
                self.w.put(it[0], it[1])
            else:
                self.w.put(int(format(it[0], "0%db" % it[1])[::-1], 2), it[1])
        return self

    def dynamic(self, ll, dl, tokens, final=0, strategy="greedy", clc=None, alt258=False, end_phase=None, eob=True, played=True):
        """a dynamic block with literal / length lengths ll (HLIT = len(ll)) and distance lengths dl (HDIST = len(dl)).  end_phase: literals of an odd code
        length are appended until the block ends at that bit of a byte.  Returns what the header turned out to be."""
        assert 257 <= len(ll) <= 286 and 1 <= len(dl) <= 30
        start = self.w.bitpos()
        self.info.append(("dynamic", start))
        syms = cl_symbols(list(ll) + list(dl), strategy)
        if clc is None:
            clc = clc_for(syms)
        hclen = raw_header(self.w, final, len(ll) - 257, len(dl) - 1, clc, syms)
        hdr_bits = self.w.bitpos() - start
        lc, dc = canon(ll), canon(dl)
        put_tokens(self.w, tokens, lc, dc, alt258)
        tokens = list(tokens)
        if end_phase is not None:
            pad = next(s for s in range(256) if ll[s] & 1)
            while (self.w.bitpos() + ll[256]) % 8 != end_phase:
                self.w.put(*lc[pad])
                tokens.append(pad)
        if eob:
            self.w.put(*lc[256])
        if played:
            play_into(self.plain, tokens)
        return dict(hclen=hclen, cross=crosses(syms, len(ll)), header_bits=hdr_bits, start_bit=start, first=syms[0][0])

    def finish(self, adler=None):
        self.w.raw(struct.pack(">I", zlib.adler32(bytes(self.plain)) if adler is None else adler))
        return bytes(self.w.out)


# ---------------------------------------------------------------------------------------------------- code sets and token lists
@functools.lru_cache(maxsize=None)
def deep_codes():
    """(literal / length lengths, distance lengths) of the DEEP code: HLIT 286, HDIST 30, both complete, both up to 15 bits.
    Literal / length: [1, 2, 3, 4] + [12] * 256 is complete; 23 twelves split into 13 + 13 and one into 13 + 14 + 15 + 15 make 286 leaves under the same
    128 eleven-bit prefixes.  Distance: [1 .. 7] + [11] * 16 is complete; three elevens split into 12 + 12 and one into 12 + 13 + 14 + 15 + 15 make 30
    leaves under the same 8 ten-bit prefixes.  Symbols 283 .. 285 and distance symbols 0 .. 2 all have 12 bits: a run across the HLIT | HDIST boundary."""
    rng = random.Random(1951)
    ll = [0] * 286
    ll[32], ll[101], ll[256], ll[270] = 1, 2, 3, 4
    ll[283] = ll[284] = ll[285] = 12
    rest = [12] * 229 + [13] * 47 + [14] + [15] * 2
    rng.shuffle(rest)
    for s in range(286):
        if not ll[s]:
            ll[s] = rest.pop()
    dl = [12, 12, 12] + [0] * 27
    rest = [1, 2, 3, 4, 5, 6, 7] + [11] * 12 + [12] * 4 + [13, 14, 15, 15]
    rng.shuffle(rest)
    for s in range(3, 30):
        dl[s] = rest.pop()
    assert kraft(ll) == 32768 and kraft(dl) == 32768
    return tuple(ll), tuple(dl)


@functools.lru_cache(maxsize=None)
def deep_tokens():
    """all 256 literals, every length symbol at its base and at its top extra value, every distance symbol at its base and top (32 768 among them); between
    the matches a random literal each, so that no two distances give the same bytes"""
    rng = random.Random(286)
    toks = list(range(256))
    rng.shuffle(toks)
    pos = 256
    for i in range(29):
        for l in sorted({LBASE[i], LTOP[i]}):
            toks += [(l, rng.randint(1, pos)), rng.randrange(256)]
            pos += l + 1
    for j in range(30):
        for d in sorted({DBASE[j], DTOP[j]}):
            while pos < d:
                toks += [(258, rng.randint(1, pos)), rng.randrange(256)]
                pos += 259
            l = 3 + rng.randrange(8)
            toks += [(l, d), rng.randrange(256)]
            pos += l + 1
    return tuple(toks)


def rand_tokens(rng, pos, nbytes, p_match=0.5, lits=None, dists=None, long_matches=False):
    """tokens for exactly nbytes of output behind `pos` bytes already there: literals from `lits` (default: any byte), distances from `dists` (default:
    anything up to the position and 32 768)"""
    toks, made = [], 0
    while made < nbytes:
        left, here = nbytes - made, pos + made
        if left >= 3 and here and rng.random() < p_match:
            l = min(left, 258 if long_matches and rng.random() < 0.9 else rng.choice((3, 4, 5, 8, 11, 19, 35, 67, 130, 131, 227, 257, 258)))
            d = rng.choice([x for x in dists if x <= here] or [0]) if dists else rng.randint(1, min(here, 32768))
            if d:
                toks.append((l, d))
                made += l
                continue
        toks.append(rng.choice(lits) if lits else rng.randrange(256))
        made += 1
    return toks


def flat_ll(symbols, hlit=None):
    """literal / length lengths: a complete two-length code over `symbols` (256 is added), HLIT as small as it can be unless given"""
    symbols = sorted(set(symbols) | {256})
    hlit = max(257, symbols[-1] + 1) if hlit is None else hlit
    ll = [0] * hlit
    for s, l in zip(symbols, flat_code(len(symbols))):
        ll[s] = l
    return ll


ALL_LL = tuple(range(286))


# ---------------------------------------------------------------------------------------------------- the accept cases
def _case(name, z, **props):
    s = z.finish()
    props.setdefault("blocks", list(z.info))
    return (name, s, bytes(z.plain), props)


def _deep_case(name, strategy, alt258=False, cmf=0x78):
    ll, dl = deep_codes()
    z = Z(cmf)
    h = z.dynamic(ll, dl, deep_tokens(), final=1, strategy=strategy, alt258=alt258)
    return _case(name, z, lprefix=prefixes(ll, 11), dprefix=prefixes(dl, 10), lmax=max(ll), dmax=max(dl), llens=sorted(set(ll)), **h)


def _single_code_cases():
    rng = random.Random(11)
    out = []
    # a single one-bit distance code (distance 1 / distance 4 only), two one-bit codes, no distance code at all, nothing but the end of block
    for name, dl, dists in (("one-dist-code", [1], [1]), ("one-dist-code-sym3", [0, 0, 0, 1], [4]), ("two-dist-codes", [1, 1], [1, 2])):
        z = Z()
        toks = [rng.randrange(256) for _ in range(9)] + rand_tokens(rng, 9, 3000, 0.3, dists=dists)
        h = z.dynamic(flat_ll(ALL_LL), dl, toks, final=1)
        out.append(_case(name, z, **h))
    z = Z()
    h = z.dynamic(flat_ll(range(256), hlit=286), [0], rand_tokens(rng, 0, 2000, 0.0), final=1)     # 29 + 1 zero lengths: a run of symbol 18 across the boundary
    out.append(_case("no-dist-code", z, **h))
    z = Z()
    ll = [0] * 259
    ll[256] = 1
    h = z.dynamic(ll, [0], [], final=1)                                                           # 2 + 1 zero lengths: a run of symbol 17 across the boundary
    out.append(_case("eob-only", z, **h))
    return out


def _clc_cases():
    """HCLEN 4 cannot be built: with lengths for 16, 17, 18 and 0 only, every code length of the block is zero, so there is no end-of-block code and zlib
    refuses the block.  HCLEN 5 adds symbol 8: 256 symbols of 8 bits (the literals but 255, and the end of block) and no distance code."""
    rng = random.Random(12)
    out = []
    clc = [0] * 19
    clc[8], clc[0], clc[16], clc[17], clc[18] = 1, 2, 3, 4, 4
    ll = [8] * 255 + [0, 8]
    z = Z()
    h = z.dynamic(ll, [0], [rng.randrange(255) for _ in range(1500)], final=1, clc=clc)
    out.append(_case("hclen-5", z, **h))
    # a code-length code of 1 .. 7 bits: 8 and 9 (the literal / length lengths) short, 4 and 5 (the distance lengths) with the two 7-bit codes
    clc = [0] * 19
    clc[8], clc[9], clc[0], clc[18], clc[17], clc[16], clc[5], clc[4] = 1, 2, 3, 4, 5, 6, 7, 7
    z = Z()
    h = z.dynamic(flat_ll(ALL_LL), [4] * 8 + [5] * 16, rand_tokens(rng, 0, 3000, 0.3, dists=list(range(1, 4097))), final=1, clc=clc)
    out.append(_case("clc-7-bits", z, **h))
    return out


def _ll_split_cases():
    rng = random.Random(13)
    ll = flat_ll(list(range(256)) + [257])
    out = []
    for n in (LL_SPLIT - 1, LL_SPLIT, LL_SPLIT + 1):
        z = Z()
        z.dynamic(ll, [1, 1], list(rng.randbytes(n)) + [(3, 1), 7, 8], final=1)
        out.append(_case("ll-split-%d" % n, z))
    z = Z()
    z.stored(rng.randbytes(65535)).stored(rng.randbytes(65535))
    ll5 = [0] * 258
    ll5[1], ll5[2], ll5[257], ll5[9], ll5[256] = 2, 2, 2, 3, 3
    z.dynamic(ll5, [1], [1, 2, (3, 1), 9], final=1)
    out.append(_case("ll-split-mixed", z))
    z = Z()
    z.dynamic(ll, [1, 1], list(rng.randbytes(BLK)), final=1)
    out.append(_case("piece-131072-literals", z))
    z = Z()
    z.dynamic(ll, [1, 1], list(rng.randbytes(BLK - 3)) + [(3, 1)], final=1)
    out.append(_case("piece-131069+3", z))
    return out


def _stored_cases():
    out = []
    for k in range(8):
        # a fixed block of 8-bit literals ends at bit 2 of a byte (3 + 8 n + 7 bits): every 9-bit literal moves the end on by one
        z = Z()
        z.fixed(list(b"phase") + [144 + 13 * k + i for i in range((k - 2) % 8)])
        phase = z.w.bitpos() % 8
        z.stored(b"").stored(b"end", final=1)
        out.append(_case("stored-phase-%d" % k, z, phase=phase))
    z = Z()
    z.stored(random.Random(14).randbytes(65535), final=1)
    out.append(_case("stored-65535", z))
    return out


# a maximal dynamic header: HLIT 286, HDIST 30, HCLEN 19, one symbol per length, the frequent lengths with the longest code-length codes
BIG_CLC = [0, 3, 3, 3, 3, 3, 3, 3, 0, 0, 0, 6, 7, 7, 5, 4, 0, 0, 0]


def _reseat_cases():
    """stream = zlib header (2 bytes), stored header (5), data, then a DEEP dynamic block: the data ends d bytes in front of stream byte 1 024 (2 048 for
    d = 1 023: 1 in front of a ring half's second word)"""
    rng = random.Random(15)
    ll, dl = deep_codes()
    out = []
    for d in (0, 1, 2, 3, 4, 1023):
        end = (2048 if d == 1023 else 1024) - d
        z = Z()
        z.stored(rng.randbytes(end - 7))
        assert len(z.w.out) == end
        z.dynamic(ll, dl, rand_tokens(rng, end - 7, 2500, 0.4), final=1)
        out.append(_case("reseat-d%d" % d, z, data_end=end))
    for edge in (1024, 2048):
        z = Z()
        z.stored(rng.randbytes(edge - 4 - 7))
        h = z.dynamic(ll, dl, rand_tokens(rng, edge - 11, 2500, 0.4), final=1, strategy="none", clc=BIG_CLC)
        out.append(_case("big-header-at-ring-edge-%d" % edge, z, **h))
    return out


def _piece(z, rng, first_tokens, final, codes, marker=False):
    """one piece of this library's layout: BLK bytes of output in dynamic blocks, closed by an empty non-final stored block (k_deflate.hip: end of block, then
    the header 000, zero padding and 00 00 FF FF) unless it is the stream's last, whose last block is final and is followed by the trailer"""
    ll, dl = codes
    pos = len(z.plain)
    n1 = len(play(first_tokens, bytes(z.plain)))
    if marker:
        half = rand_tokens(rng, pos + n1, 40000, 0.9, long_matches=True)
        z.dynamic(ll, dl, list(first_tokens) + half)
        z.stored(b"\x00\x00\xff\xff")
        n1 += 40004
        first_tokens = []
    z.dynamic(ll, dl, list(first_tokens) + rand_tokens(rng, pos + n1, BLK - n1, 0.9, long_matches=True), final=final)
    if not final:
        z.stored(b"")


def _layout_cases():
    out = []
    for name, marker in (("own-layout-3-pieces", False), ("chance-marker", True)):
        rng = random.Random(16)
        z = Z()
        first = list(rng.randbytes(6000))
        _piece(z, rng, first, 0, (flat_ll(ALL_LL), [5] * 28 + [4] * 2))
        _piece(z, rng, [(100, 5000)], 0, deep_codes(), marker)                    # piece 2 copies from piece 1 ...
        _piece(z, rng, [(258, 32768)], 1, deep_codes())                           # ... and piece 3, at the largest distance, from piece 2
        sizes = [BLK] * 3
        out.append(_case(name, z, pieces=sizes))
    return out


@functools.lru_cache(maxsize=None)
def accept_cases():
    """every accept case but the large stream"""
    out = [_deep_case("deep-greedy", "greedy"), _deep_case("deep-norepeat", "none"), _deep_case("deep-258-as-284+31", "greedy", alt258=True),
           _deep_case("window-256-dist-32768", "greedy", cmf=0x08)]
    out += _single_code_cases() + _clc_cases() + _ll_split_cases() + _stored_cases() + _reseat_cases() + _layout_cases()
    assert len({c[0] for c in out}) == len(out)
    return out


@functools.lru_cache(maxsize=None)
def large_case():
    """large-handbuilt: 48 non-final dynamic blocks in three families -- DEEP code with long matches, a single distance code, DEEP code with literals
    (12 bits and more each: the stream grows) --, a non-final stored block behind every fifth, its header at bit 0, 1, .. 7 of a byte in turn, and a final
    dynamic block"""
    rng = random.Random(17)
    deep = deep_codes()
    one = (flat_ll(ALL_LL), [1])
    z = Z()
    phases, nstored = [], 0
    for i in range(48):
        pos, want = len(z.plain), (nstored % 8 if i % 5 == 4 else None)
        if i % 3 == 0:
            toks = (list(rng.randbytes(2000)) if i == 0 else []) + rand_tokens(rng, pos + (2000 if i == 0 else 0), 56000, 0.95, long_matches=True)
            z.dynamic(*deep, toks, end_phase=want, strategy="greedy" if i % 2 else "none")
        elif i % 3 == 1:
            z.dynamic(*one, rand_tokens(rng, pos, 6000, 0.2, dists=[1]), end_phase=want)
        else:
            z.dynamic(*deep, rand_tokens(rng, pos, 7500, 0.002), end_phase=want)
        if want is not None:
            phases.append(z.w.bitpos() % 8)
            z.stored(rng.randbytes(700 + 37 * nstored))
            nstored += 1
    z.dynamic(*deep, rand_tokens(rng, len(z.plain), 3000, 0.5), final=1)
    return _case("large-handbuilt", z, stored_phases=phases)


@functools.lru_cache(maxsize=None)
def large_family_cases():
    """three more large streams, each with block starts of ONE kind, so that the trial parser (k_ispec) cannot miss a kind unnoticed -- a stream whose
    starts it does not find goes to the serial walk, which the route counter shows: DEEP headers with repeat symbols only; headers with a single
    one-bit distance code only; stored headers only, at bit 0 .. 7 of a byte in turn behind fixed-code blocks (which the parser does not look for; a second
    stored block follows each, because isp_stored_ok takes a stored start only with a stored or dynamic header behind its bytes)"""
    rng = random.Random(18)
    deep, one = deep_codes(), (flat_ll(ALL_LL), [1])
    out = []
    z = Z()
    for i in range(24):
        z.dynamic(*deep, rand_tokens(rng, len(z.plain), 8000, 0.002) if i % 2 == 0 else rand_tokens(rng, len(z.plain), 90000, 0.95, long_matches=True))
    z.dynamic(*deep, rand_tokens(rng, len(z.plain), 1000, 0.5), final=1)
    out.append(_case("large-deep-only", z))
    z = Z()
    for i in range(24):
        z.dynamic(*one, list(rng.randbytes(64)) + rand_tokens(rng, len(z.plain) + 64, 46000, 0.025, dists=[1], long_matches=True))
    z.dynamic(*one, rand_tokens(rng, len(z.plain), 1000, 0.1, dists=[1]), final=1)
    out.append(_case("large-one-dist-code-only", z))
    z = Z()
    z.stored(rng.randbytes(8192))
    phases = []
    for i in range(22):
        z.fixed(rand_tokens(rng, len(z.plain), 44000, 0.95, long_matches=True), end_phase=i % 8)
        phases.append(z.w.bitpos() % 8)
        z.stored(rng.randbytes(6500 + i)).stored(rng.randbytes(40))
    z.fixed(rand_tokens(rng, len(z.plain), 1000, 0.5), final=1)
    out.append(_case("large-stored-starts-only", z, stored_phases=phases))
    return out


# ---------------------------------------------------------------------------------------------------- the streams zlib refuses
def _hdr_only(ll, dl, final=1, **kw):
    """a dynamic block's header with one literal-0 code's worth of zero bits behind it: the code set itself is what is wrong"""
    z = Z()
    z.dynamic(ll, dl, [("raw", 0, 16)], final=final, eob=False, played=False, **kw)
    return z


def _ll(**at):
    ll = [0] * 257
    for k, v in at.items():
        ll[int(k[1:])] = v
    return ll


@functools.lru_cache(maxsize=None)
def reject_cases():
    out = []

    def rej(name, z, raw=1):
        out.append((name, z.finish(), None, dict(raw=raw, blocks=list(z.info))))
    ok_ll = _ll(s0=1, s256=1)
    rej("ll-incomplete", _hdr_only(_ll(s0=2, s256=2), [0]))
    rej("ll-oversubscribed", _hdr_only(_ll(s0=1, s1=1, s256=1), [0]))
    rej("dist-incomplete", _hdr_only(ok_ll, [2, 2, 2]))
    rej("dist-oversubscribed", _hdr_only(ok_ll, [1, 1, 1]))
    one = [0] * 19
    one[8] = 1
    z = Z()
    raw_header(z.w, 1, 0, 0, one, [(8, 0, 0)] * 258)
    rej("clc-incomplete", z)
    over = [0] * 19
    over[0] = over[8] = over[16] = 1
    z = Z()
    raw_header(z.w, 1, 0, 0, over, [])
    z.w.put(0, 300)
    rej("clc-oversubscribed", z)
    two = [0] * 19
    two[0] = two[8] = 1
    for name, hl, hd in (("hlit-30", 30, 0), ("hlit-31", 31, 0), ("hdist-30", 0, 30), ("hdist-31", 0, 31)):
        z = Z()
        raw_header(z.w, 1, hl, hd, two, [(8, 0, 0)] * 255 + [(0, 0, 0), (8, 0, 0)] + [(0, 0, 0)] * 64)
        rej(name, z)
    c16 = [0] * 19
    c16[16] = c16[1] = 1
    z = Z()
    raw_header(z.w, 1, 0, 0, c16, [(16, 2, 0)] + [(1, 0, 0)] * 300)
    rej("repeat-first", z)
    c4 = [0] * 19
    c4[0] = c4[1] = c4[17] = c4[18] = 2
    z = Z()                                                              # lengths 1, 255 x 0, 1, then a run of three zeros where one distance length is left
    raw_header(z.w, 1, 0, 0, c4, [(1, 0, 0), (18, 7, 127), (18, 7, 106), (1, 0, 0), (17, 3, 0)])
    z.w.put(0, 16)
    rej("repeat-overshoots", z)
    rej("no-end-of-block", _hdr_only(_ll(s0=1, s1=1), [0]))
    m_ll = [0] * 258
    m_ll[0], m_ll[256], m_ll[257] = 2, 2, 1
    mc = canon(m_ll)
    z = Z()
    z.dynamic(m_ll, [0], [0, ("raw",) + mc[257], ("raw", 0, 1)], final=1, played=False)
    z.plain += b"\x00"
    rej("match-without-dist-code", z)
    z = Z()
    z.dynamic(m_ll, [1], [0, ("raw",) + mc[257], ("raw", 1, 1)], final=1, played=False)
    z.plain += b"\x00"
    rej("one-dist-code-unused-bit", z)
    z = Z()
    z.fixed_raw([(0x30 + 97, 8), (0xC0 + 6, 8), (0, 7)], final=1)       # 'a', symbol 286, end of block
    z.plain += b"a"
    rej("fixed-symbol-286", z)
    z = Z()
    z.fixed_raw([(0x30 + 97, 8), (1, 7), (30, 5), (0, 7)], final=1)     # 'a', length 3, distance symbol 30, end of block
    z.plain += b"a"
    rej("fixed-dist-symbol-30", z)
    z = Z()
    z.fixed([97, 98, (3, 3)], final=1, played=False)
    z.plain += b"ab"
    rej("fixed-dist-past-start", z, raw=5)
    z = Z()
    z.dynamic(flat_ll([97, 98, 257]), [1, 2, 2], [97, 98, (3, 3)], final=1, played=False)
    z.plain += b"ab"
    rej("dynamic-dist-past-start", z, raw=5)
    rej("stored-bad-nlen", Z().stored(b"abc", final=1, nlen=0x1234), raw=3)
    rej("stored-past-end", Z().stored(b"abcde", final=1, len_field=100), raw=100)
    z = Z()
    z.w.put(1, 1)
    z.w.put(3, 2)
    rej("block-type-3", z)
    rej("no-end-of-block-code-in-stream", Z().fixed(list(b"abc"), final=1, eob=False), raw=3)
    rej("cinfo-8", Z(0x88).stored(b"abc", final=1), raw=3)
    assert len({c[0] for c in out}) == len(out)
    return out


# ---------------------------------------------------------------------------------------------------- seeded random valid streams
def random_code(rng, n, maxlen):
    """the lengths (a multiset) of a complete code of n >= 2 leaves that reaches min(maxlen, n - 1) bits"""
    depth = min(maxlen, n - 1)
    leaves = list(range(1, depth)) + [depth, depth]
    while len(leaves) < n:
        i = rng.randrange(len(leaves))
        if leaves[i] >= maxlen:
            i = next(k for k, l in enumerate(leaves) if l < maxlen)
        l = leaves[i]
        leaves[i] = l + 1
        leaves.append(l + 1)
    return leaves


def _random_block(rng, z, final, budget):
    kind = rng.choice(("stored", "fixed", "dynamic", "dynamic"))
    if kind == "stored":
        z.stored(rng.randbytes(rng.randrange(min(300, budget) + 1)), final=final)
        return
    if kind == "fixed":
        ll, dl = list(FIXED_LL[:286]), list(FIXED_D[:30])
    else:
        maxlen = rng.randint(7, 15)
        n = rng.randint(2, min(286, 1 << maxlen))
        used = rng.sample([s for s in range(286) if s != 256], n - 1) + [256]
        lens = random_code(rng, n, maxlen)
        rng.shuffle(lens)
        hlit = 286 if rng.random() < 0.3 else max(257, max(used) + 1)
        ll = [0] * hlit
        for s, l in zip(used, lens):
            ll[s] = l
        how = rng.choice(("none", "one", "full", "full"))
        if how == "none":
            dl = [0] * rng.randint(1, 4)
        elif how == "one":
            dl = [0] * rng.randint(1, 30)
            dl[rng.randrange(len(dl))] = 1
        else:
            nd = rng.randint(2, 30)
            dused = rng.sample(range(30), nd)
            dlens = random_code(rng, nd, rng.randint(7, 15))
            rng.shuffle(dlens)
            dl = [0] * (30 if rng.random() < 0.3 else max(dused) + 1)
            for s, l in zip(dused, dlens):
                dl[s] = l
    lits = [s for s in range(256) if ll[s]]
    lsyms = [s - 257 for s in range(257, len(ll)) if ll[s]]
    toks, made = [], 0
    for _ in range(rng.randrange(400)):
        pos = len(z.plain) + made
        dsyms = [s for s in range(len(dl)) if dl[s] and DBASE[s] <= pos]
        if made + 258 > budget:
            break
        if lsyms and dsyms and (not lits or rng.random() < 0.4):
            i, j = rng.choice(lsyms), rng.choice(dsyms)
            l = LBASE[i] + rng.randrange(1 << LEXT[i])
            toks.append((l, min(DBASE[j] + rng.randrange(1 << DEXT[j]), pos)))
            made += l
        elif lits:
            toks.append(rng.choice(lits))
            made += 1
    if kind == "fixed":
        z.fixed(toks, final=final)
    else:
        z.dynamic(ll, dl, toks, final=final, strategy=rng.choice(("greedy", "none")), alt258=len(ll) < 286 or not ll[285])


@functools.lru_cache(maxsize=None)
def random_cases(n=200, seed=20261019):
    rng = random.Random(seed)
    out = []
    for k in range(n):
        z = Z()
        nb = rng.randint(1, 4)
        for b in range(nb):
            _random_block(rng, z, int(b == nb - 1), 8192 - len(z.plain))
        assert len(z.plain) <= 8192
        out.append(_case("random-%03d" % k, z))
    return out


def markers(stream):
    """00 00 FF FF at any byte position: what the piece scan counts"""
    return stream.count(b"\x00\x00\xff\xff")
