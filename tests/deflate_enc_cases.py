"""Crafted inputs for the deflate encoder's entropy stage, and an analyser that is independent of oracle/deflate_model.c.

The stage in question: k_dstats<256> / <64> (histograms, the three code builds, the run-length tokens of the table description), k_adler<256> / <64>,
k_dblock (token-parallel packing through LDS), k_dplan (dynamic or stored per block), k_dwrite, k_dfinal, k_dfold (csrc/k_deflate.hip).  The suite's other
inputs -- corpus text and noise, two golden images, structured LZ noise -- were made for the match finder; they clamp a code now and then and never run the
second loop of the Kraft repair.  The cases here are built for the code builder.

THE ANALYSER (pure Python, no torch; it never calls the model's code build or its LZ stage)
  parse_stream / model_blocks   a token-level inflate over a whole zlib stream: per dynamic block HLIT, HDIST, HCLEN, the 19 code-length-code lengths,
                                the tokens (a length 0..15, or 17 / 18 with its run), the lit/len and distance lengths, the count of every symbol it
                                decodes, the match lengths and distances, the header's size in bits, where the end-of-block code ends in its byte, the
                                literal bits per 2 048-byte tile; per stored block the piece sizes.  Blocks are grouped by 128 KiB block and 1 MiB segment.
  build_lens                    the length builder again, with branch counters: stable sort by (count, symbol), two-queue merge in which a leaf wins a tie,
                                clamp, the "up" loop, the "down" loop.
  tokenise                      the greedy zero-run scan (18 from 11, 17 from 3).
  analyse                       per segment: one table description for all its dynamic blocks; build_lens over the decoded counts (one end-of-block per
                                block) must EQUAL the lit/len lengths (limit 15) and the distance lengths (limit 15) of the header, tokenise() of those must
                                equal the header's tokens, build_lens over the token counts (limit 7) its code-length code, and the three sizes and the
                                header's bit count must follow.  So the model's code build is checked by a second implementation, not by itself.

THE CASES (name, plain bytes, levels; build_cases).  What they reach, measured with the model (n = used symbols, dep = depth before the clamp, CL = clamped,
u / d = steps of the up / down loop, t = ties between a queued leaf and an inner node; then the header's bits):
  case                   level   bytes  plan      lit/len                    distance                 code-length code     header
  A.geo_2.0_x28              6  1048576  DDDDDDDD  n32 dep18 CL u3 d0 t4      n22 dep16 CL u1 d0 t0    n16 dep6 -- u0 d0 t9   440
  A.geo_1.7_x40              9  1048576  DDDDDDDD  n35 dep17 CL u2 d0 t1      n22 dep17 CL u2 d1 t2    n16 dep5 -- u0 d0 t4   489
  A.geo_1.1_x256             1  1048576  DDDDDDDD  n129 dep20 CL u26 d2 t24   n12 dep7 -- u0 d0 t3     n16 dep7 -- u0 d0 t3   831
  A.geo_1.8_x30_128k         6   131072  D         n28 dep16 CL u1 d1 t3      n19 dep13 -- u0 d0 t1    n16 dep5 -- u0 d0 t10  423
  B.up1_down2_17k            6    17000  D         n113 dep14 -- u0 d0 t0     n0                       n14 dep8 CL u1 d2 t1   529
  B.up3_down2_30k            6    30000  D         n121 dep16 CL u1 d0 t3     n0                       n13 dep8 CL u3 d2 t2   628
  B.up2_down2_60k            6    60000  D         n114 dep15 -- u0 d0 t2     n0                       n13 dep8 CL u2 d2 t2   543
  B.up1_down0_30k            6    30000  D         n113 dep14 -- u0 d0 t0     n0                       n12 dep8 CL u1 d0 t1   525
  C.permutations_x16_twice   6     8192  D         n259 dep10 -- u0 d0 t20    n1 dep1                  n5 dep3 -- u0 d0 t1    360
  C.equal_pairs_twice        6     1024  D         n259 dep9 -- u0 d0 t256    n1 dep1                  n4 dep3 -- u0 d0 t0    356
  C.all_283                  9   108544  D         n283 dep16 CL u34 d3 t11   n6 dep4 -- u0 d0 t0      n10 dep6 -- u0 d0 t3   508
  C.largest_header           6   169174  DD        n283 dep16 CL u37 d0 t77   n3 dep2 -- u0 d0 t0      n16 dep8 CL u2 d0 t5   846
  D.no_match                 6      550  D         n102 dep8 -- u0 d0 t0      n0                       n5 dep4 -- u0 d0 t1    201
  D.one_distance             6      770  D         n150 dep10 -- u0 d0 t0     n1 dep1                  n7 dep6 -- u0 d0 t2    357
  D.two_distances            6      819  D         n159 dep10 -- u0 d0 t2     n2 dep1                  n8 dep6 -- u0 d0 t2    408
  F.lengths                  9   108544  D         n283 dep16 CL u35 d3 t11   n6 dep4 -- u0 d0 t0      n10 dep6 -- u0 d0 t3   508
  F.near                     6   372749  DDD       n201 dep18 CL u11 d7 t41   n23 dep6 -- u0 d0 t0     n12 dep8 CL u2 d1 t0   773
  G.alternating              6   786432  SDSDSD    n263 dep12 -- u0 d0 t0     n18 dep14 -- u0 d0 t0    n15 dep7 -- u0 d0 t5   588
  G.dense_tile               6  1048576  DDDDDDDD  n222 dep16 CL u5 d5 t0     n23 dep18 CL u2 d0 t2    n14 dep6 -- u0 d0 t6   455
Coverage reached (asserted as measured by test_deflate_enc_cases.py, so that a later change which loses some of it fails):
  deepest code before the clamp   20 (A.geo_1.1_x256)          most "up" steps    37 (C.largest_header)        most "down" steps   7 (F.near)
  largest header                  846 bits (C.largest_header) of at most 14 + 57 + 316 * 7 = 2 283
  densest tile                    30 720 literal bits (G.dense_tile, tile 100): all 2 048 literals of the tile cost 15 bits -- the most k_dblock's staging
                                  area ("2048 x 15 + 342 x 48 bits per tile") can be asked to hold in literals
  match lengths                   every length 6 .. 258, so both ends of every length code 260 .. 284, and 285.  NONE of 3, 4, 5: the match finder takes
                                  matches of min_match = 6 and up, and a match cut from the front is kept only from cut_min = 6 bytes (deflate runs with the zstd
                                  sets' value, codec.params_for_level(.., deflate=True).cut_min).  So the symbols 257 .. 259 never occur, and the most lit/len
                                  symbols a segment can use is 256 + 1 + 26 = 283 with HLIT 29 (C.all_283), not 286.
  distances                       every code 0 .. 29; both ends of every code's range, 1 and 32 768 included (the near ones, 1 .. 4 096, at a tile's first
                                  positions only: a source must lie before the 4 096-byte tile of the position that finds it; F.near)
  zero runs (family E)            of exactly 1, 2, 3, 10, 11, 12, 137, 138, 139, 140, 141, 148, 149 and 255 lengths; runs that end at position 63, 127, 191
                                  and 255, start at 64, 128, 192 and 257, and cross 63|64, 127|128, 191|192 of the concatenated lit/len + distance lengths --
                                  k_dstats looks at them in slots of 64 (a wave's ballot), in rounds of T = 64 or 256 -- a slot without any non-zero length,
                                  and a run that ends the sequence (no match: the single distance length is 0).  Position 256 is the end-of-block symbol and
                                  never zero, so no run crosses 255|256; the distance part lies at 257 .. 315 and the next border would be 320, so a run in it
                                  (D.one_distance: 18 zeros in front of the only code) meets no border.
  end-of-block bit position       all eight values mod 8 (behind it: the 3-bit empty stored header and the alignment)
  block plans                     stored as 65 535 + 65 535 + 2, stored and dynamic alternating under one table, a last block stored / dynamic / of 1 byte,
                                  level 0 (stored only, header 78 01, the empty entry included)
Not reachable from a valid input, and why: the "one code-length symbol, add a dummy" branch (build_tables in the model, n_cl == 1 in k_dstats).  A non-empty
segment always has a literal or a match, and the end-of-block symbol: non-zero lengths.  And it always has a zero run next to them: without a match the
one distance length that is written is 0; with a match HLIT reaches at least symbol 260 and the lengths of 257 .. 259 are zeros (see "match lengths").  So
the tokens name two symbols of the code-length code or more.
"""
from __future__ import annotations

import random
import zlib
from collections import Counter

from oracle import codec

SEG, BLK, TILE = 1 << 20, 1 << 17, 2048

LEN_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LEN_EXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
DIST_BASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577)
DIST_EXTRA = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)


def len_range(code):
    """(smallest, largest) match length of lit/len symbol 257 + code (RFC 1951 3.2.5; 284 ends at 257, 285 is 258 alone)"""
    return LEN_BASE[code], (258 if code == 28 else LEN_BASE[code] + (1 << LEN_EXTRA[code]) - 1)


def dist_range(code):
    return DIST_BASE[code], DIST_BASE[code] + (1 << DIST_EXTRA[code]) - 1


# ----------------------------------------------------------------------------- the length builder, a second time

def build_lens(count, maxlen, leaf_wins_ties=True):
    """Code lengths <= maxlen for the symbols with a count: (lens, facts).  Steps: stable sort by (count, symbol); two-queue merge in which the leaf
    wins a tie; clamp to maxlen; while the code is over-subscribed lengthen the first symbol (in sorted order) of the longest length below maxlen
    ("up"); while it is under-subscribed shorten the most frequent symbol of the shortest length whose step still fits ("down").
    facts: n, maxdepth, clamp, up, down, ties (merge picks at which the leaf at the head of its queue weighed exactly what the inner node at the
    head of the other queue weighed)."""
    nsym = len(count)
    lens = [0] * nsym
    order = sorted((s for s in range(nsym) if count[s]), key=lambda s: (count[s], s))
    n = len(order)
    facts = dict(n=n, maxdepth=0, clamp=False, up=0, down=0, ties=0)
    if n == 0:
        return lens, facts
    if n == 1:
        lens[order[0]] = 1
        facts["maxdepth"] = 1
        return lens, facts
    weight = [count[s] for s in order]
    up_link = [0] * (2 * n - 1)
    leaf, inner = 0, n
    while len(weight) < 2 * n - 1:
        picked = []
        for _ in range(2):
            have_leaf, have_inner = leaf < n, inner < len(weight)
            if have_leaf and have_inner and weight[leaf] == weight[inner]:
                facts["ties"] += 1
                take_leaf = leaf_wins_ties
            else:
                take_leaf = have_leaf and (not have_inner or weight[leaf] < weight[inner])
            if take_leaf:
                picked.append(leaf); leaf += 1
            else:
                picked.append(inner); inner += 1
        for k in picked:
            up_link[k] = len(weight)
        weight.append(weight[picked[0]] + weight[picked[1]])
    depth = [0] * (2 * n - 1)
    for k in range(2 * n - 3, -1, -1):
        depth[k] = depth[up_link[k]] + 1
    facts["maxdepth"] = max(depth[:n])
    cur = [min(d, maxlen) for d in depth[:n]]                    # in sorted order: rarest first
    if facts["maxdepth"] > maxlen:
        facts["clamp"] = True
        debt = sum(1 << (maxlen - l) for l in cur) - (1 << maxlen)
        while debt > 0:
            longest = max(l for l in cur if l < maxlen)
            k = cur.index(longest)
            cur[k] += 1
            debt -= 1 << (maxlen - 1 - longest)
            facts["up"] += 1
        while debt < 0:
            fits = [l for l in cur if l > 1 and (1 << (maxlen - l)) <= -debt]
            if not fits:
                break
            shortest = min(fits)
            k = n - 1 - cur[::-1].index(shortest)
            cur[k] -= 1
            debt += 1 << (maxlen - shortest)
            facts["down"] += 1
    for k, s in enumerate(order):
        lens[s] = cur[k]
    return lens, facts


def tokenise(seq, t18=11, t17=3):
    """The greedy scan over the code lengths: (symbol, run) with 18 for a zero run of 11..138, 17 for 3..10, single zeros below 3; symbol 16 never."""
    out, i, n = [], 0, len(seq)
    while i < n:
        if seq[i] == 0:
            z = 1
            while i + z < n and seq[i + z] == 0 and z < 138:
                z += 1
            if z >= t18:
                out.append((18, z)); i += z; continue
            if z >= t17:
                out.append((17, z)); i += z; continue
        out.append((seq[i], 1)); i += 1
    return out


def zero_runs(seq):
    """maximal zero runs of a sequence: [(first position, length)]"""
    runs, i = [], 0
    while i < len(seq):
        if seq[i] == 0:
            j = i
            while j < len(seq) and seq[j] == 0:
                j += 1
            runs.append((i, j - i)); i = j
        else:
            i += 1
    return runs


# ----------------------------------------------------------------------------- token-level inflate

class StreamError(ValueError):
    pass


def _decode_table(lens):
    """peek table of a canonical code (RFC 1951 3.2.2), indexed by the next bits LSB first: sym << 4 | length, 0 where no code starts"""
    mx = max(lens) if lens else 0
    if mx == 0:
        return [0], 0
    cnt = [0] * (mx + 2)
    for l in lens:
        cnt[l] += 1
    cnt[0] = 0
    nxt, code = [0] * (mx + 2), 0
    for b in range(1, mx + 1):
        code = (code + cnt[b - 1]) << 1
        nxt[b] = code
    tab = [0] * (1 << mx)
    for s, l in enumerate(lens):
        if not l:
            continue
        c = nxt[l]; nxt[l] += 1
        r = int(format(c, "0%db" % l)[::-1], 2)
        for k in range(r, 1 << mx, 1 << l):
            tab[k] = s << 4 | l
    return tab, (1 << mx) - 1


def parse_stream(stream, n_plain):
    """Walk a whole zlib stream token by token.  Returns (flevel byte, deflate blocks, trailer): a block is a dict with kind 'D' (dynamic), 'S' (stored,
    with `size`), 'F' (the fixed block of the empty entry); a dynamic one carries hlit, hdist, hclen, cl_lens[19], tokens [(symbol, run)], ll_lens[286],
    d_lens[30], llc[286], dc[30], mlens / dists (Counter), hdr_bits, eob_bit (bit position mod 8 behind its end-of-block code), start / size (plain bytes),
    and lit_bits: {tile index: bits of the literal codes of that 2 048-byte stretch of the plain data}."""
    d = bytes(stream)
    if len(d) < 6 or d[0] != 0x78 or (d[0] << 8 | d[1]) % 31:
        raise StreamError("zlib header")
    p, acc, nb = 2, 0, 0
    pos, blocks = 0, []

    def refill():
        nonlocal p, acc, nb
        c = d[p:p + 8]
        if not c:
            raise StreamError("stream ends inside a block")
        acc |= int.from_bytes(c, "little") << nb
        nb += 8 * len(c); p += len(c)

    def get(k):
        nonlocal acc, nb
        while nb < k:
            refill()
        v = acc & ((1 << k) - 1)
        acc >>= k; nb -= k
        return v

    while True:
        final, kind = get(1), get(2)
        if kind == 0:
            acc >>= nb & 7; nb -= nb & 7
            ln, nln = get(16), get(16)
            if ln ^ nln != 0xFFFF:
                raise StreamError("stored length check")
            p -= nb >> 3; acc = nb = 0
            if p + ln > len(d):
                raise StreamError("stored data")
            blocks.append(dict(kind="S", start=pos, size=ln, final=final))
            p += ln; pos += ln
        elif kind == 1:
            if get(7) != 0:
                raise StreamError("fixed block other than the empty one")
            blocks.append(dict(kind="F", start=pos, size=0, final=final))
        elif kind == 2:
            h0 = p * 8 - nb
            hlit, hdist, hclen = get(5), get(5), get(4)
            cl_lens = [0] * 19
            for k in range(hclen + 4):
                cl_lens[CL_ORDER[k]] = get(3)
            ctab, cmask = _decode_table(cl_lens)
            nll, nd = hlit + 257, hdist + 1
            seq, tokens = [], []
            while len(seq) < nll + nd:
                while nb < 16:
                    refill()
                e = ctab[acc & cmask]
                if not e:
                    raise StreamError("code-length code")
                acc >>= e & 15; nb -= e & 15
                s = e >> 4
                if s < 16:
                    seq.append(s); tokens.append((s, 1))
                elif s == 16:
                    raise StreamError("symbol 16: the encoder never emits it")
                else:
                    r = get(3) + 3 if s == 17 else get(7) + 11
                    seq += [0] * r; tokens.append((s, r))
            if len(seq) != nll + nd:
                raise StreamError("code lengths overrun")
            hdr_bits = p * 8 - nb - h0
            ll_lens, d_lens = seq[:nll] + [0] * (286 - nll), seq[nll:] + [0] * (30 - nd)
            lt, lmask = _decode_table(ll_lens)
            dt, dmask = _decode_table(d_lens)
            llc, dc, mlens, dists, lit_bits = [0] * 286, [0] * 30, Counter(), Counter(), Counter()
            start = pos
            while True:
                if nb < 48:
                    refill() if p < len(d) else None
                e = lt[acc & lmask]
                l = e & 15
                if not l or l > nb:
                    raise StreamError("lit/len code")
                acc >>= l; nb -= l
                s = e >> 4
                llc[s] += 1
                if s < 256:
                    lit_bits[pos >> 11] += l
                    pos += 1
                elif s == 256:
                    break
                else:
                    c = s - 257
                    x = LEN_EXTRA[c]
                    ml = LEN_BASE[c] + (acc & ((1 << x) - 1))
                    acc >>= x; nb -= x
                    e = dt[acc & dmask]
                    l = e & 15
                    if not l:
                        raise StreamError("distance code")
                    acc >>= l; nb -= l
                    c = e >> 4
                    x = DIST_EXTRA[c]
                    if nb < x:
                        refill()
                    off = DIST_BASE[c] + (acc & ((1 << x) - 1))
                    acc >>= x; nb -= x
                    if off > pos:
                        raise StreamError("distance beyond the start")
                    dc[c] += 1; mlens[ml] += 1; dists[off] += 1
                    pos += ml
            blocks.append(dict(kind="D", start=start, size=pos - start, final=final, hlit=hlit, hdist=hdist, hclen=hclen, cl_lens=cl_lens, tokens=tokens,
                               ll_lens=ll_lens, d_lens=d_lens, llc=llc, dc=dc, mlens=mlens, dists=dists, hdr_bits=hdr_bits, eob_bit=(p * 8 - nb) & 7,
                               lit_bits=lit_bits))
        else:
            raise StreamError("block type 3")
        if final:
            break
    p -= nb >> 3
    if pos != n_plain or p + 4 != len(d):
        raise StreamError("length: %d plain bytes of %d, %d stream bytes of %d" % (pos, n_plain, p + 4, len(d)))
    return d[1], blocks, int.from_bytes(d[p:p + 4], "big")


def model_blocks(stream, plain):
    """The deflate blocks grouped as the encoder laid them out: one record per 128 KiB block of a 1 MiB segment -- its dynamic block or its stored pieces
    -- each but the entry's last followed by the empty stored block of the sync flush.  Returns (flevel, [(segment, [block record ...])], adler)."""
    n = len(plain)
    flevel, blocks, adler = parse_stream(stream, n)
    if n == 0:
        return flevel, [], adler
    it = iter(blocks)
    segs = []
    for s0 in range(0, n, SEG):
        sl, recs = min(SEG, n - s0), []
        for b0 in range(s0, s0 + sl, BLK):
            bl = min(BLK, s0 + sl - b0)
            last = b0 + bl >= n
            first = next(it)
            if first["start"] != b0:
                raise StreamError("block does not start at %d" % b0)
            if first["kind"] == "D":
                if first["size"] != bl:
                    raise StreamError("dynamic block of %d bytes for a block of %d" % (first["size"], bl))
                rec = dict(first, pieces=None)
            else:
                pieces, got = [first["size"]], first["size"]
                lastpiece = first
                while got < bl:
                    lastpiece = next(it)
                    if lastpiece["kind"] != "S":
                        raise StreamError("stored pieces interrupted")
                    pieces.append(lastpiece["size"]); got += lastpiece["size"]
                if got != bl or 0 in pieces:
                    raise StreamError("stored pieces %r for a block of %d" % (pieces, bl))
                rec = dict(kind="S", start=b0, size=bl, pieces=pieces, final=lastpiece["final"])
            if bool(rec["final"]) != last:
                raise StreamError("BFINAL misplaced")
            if not last:
                sync = next(it)
                if sync["kind"] != "S" or sync["size"] != 0 or sync["final"]:
                    raise StreamError("sync flush missing behind a block")
            recs.append(rec)
        segs.append((s0, recs))
    if next(it, None) is not None:
        raise StreamError("blocks behind the last one")
    return flevel, segs, adler


def analyse(stream, plain):
    """Per-segment records of a model (or device) stream, after checking it against the replicas: for every segment with a dynamic block, all its
    dynamic blocks repeat ONE table description; the lit/len and distance lengths in it equal build_lens(counts, 15) of the counts decoded from the
    segment's blocks (+ the stored blocks' bytes as literals, see below, + one end-of-block per block); its tokens equal tokenise(lengths); its
    code-length-code lengths equal build_lens(token counts, 7); HLIT / HDIST / HCLEN are the trimmed sizes.  Raises AssertionError otherwise.

    A block the planner stored still counted in the segment's statistics, with whatever matches the LZ stage found in it, and those cannot be read
    from the stream: the analyser counts its bytes as literals.  The cases that mix stored and dynamic blocks store blocks of noise, where that is
    what the LZ stage emits; if it were not, the rebuilt lengths would differ from the header's and analyse() would fail, not pass by mistake."""
    flevel, segs, adler = model_blocks(stream, plain)
    out = []
    for s0, recs in segs:
        dyn = [r for r in recs if r["kind"] == "D"]
        rec = dict(start=s0, size=sum(r["size"] for r in recs), plan="".join(r["kind"] for r in recs), pieces=[r["pieces"] for r in recs if r["kind"] == "S"],
                   eob_bits=sorted({r["eob_bit"] for r in dyn}), flevel=flevel, adler=adler, ll=None, d=None, cl=None)
        if dyn:
            h = dyn[0]
            for r in dyn[1:]:
                assert (r["hlit"], r["hdist"], r["hclen"], r["cl_lens"], r["tokens"]) == (h["hlit"], h["hdist"], h["hclen"], h["cl_lens"], h["tokens"]), "one table per segment"
            llc, dc, mlens, dists, lit_bits = [0] * 286, [0] * 30, Counter(), Counter(), Counter()
            for r in recs:
                if r["kind"] == "D":
                    llc = [a + b for a, b in zip(llc, r["llc"])]
                    dc = [a + b for a, b in zip(dc, r["dc"])]
                    mlens += r["mlens"]; dists += r["dists"]; lit_bits += r["lit_bits"]
                else:
                    for v, c in Counter(plain[r["start"]:r["start"] + r["size"]]).items():
                        llc[v] += c
                    llc[256] += 1
            ll_lens, ll = build_lens(llc, 15)
            d_lens, dd = build_lens(dc, 15)
            assert ll_lens == h["ll_lens"], ("lit/len lengths", s0)
            assert d_lens == h["d_lens"], ("distance lengths", s0)
            nll = max([257] + [s + 1 for s in range(257, 286) if ll_lens[s]])
            nd = max([1] + [s + 1 for s in range(30) if d_lens[s]])
            assert (h["hlit"], h["hdist"]) == (nll - 257, nd - 1), ("HLIT / HDIST", s0)
            seq = ll_lens[:nll] + d_lens[:nd]
            tokens = tokenise(seq)
            assert tokens == h["tokens"], ("tokens", s0)
            clc = [0] * 19
            for s, _ in tokens:
                clc[s] += 1
            cl_lens, cl = build_lens(clc, 7)
            if cl["n"] == 1:                                  # (unreachable from a valid input, see the module docstring; kept so that the replica is the whole procedure)
                cl_lens[cl_lens.index(0)] = 1
            assert cl_lens == h["cl_lens"], ("code-length code", s0)
            ncl = max([4] + [k + 1 for k in range(19) if cl_lens[CL_ORDER[k]]])
            assert h["hclen"] == ncl - 4, ("HCLEN", s0)
            bits = 14 + 3 * ncl + sum(cl_lens[s] + (3 if s == 17 else 7 if s == 18 else 0) for s, _ in tokens)
            assert bits == h["hdr_bits"], ("header bits", s0)
            rec.update(ll=ll, d=dd, cl=cl, hlit=h["hlit"], hdist=h["hdist"], hclen=h["hclen"], hdr_bits=bits, tokens=tokens, seq=seq, nll=nll, runs=zero_runs(seq),
                       llc=llc, dc=dc, mlens=mlens, dists=dists, lit_bits=lit_bits, ll_lens=ll_lens, d_lens=d_lens, cl_lens=cl_lens)
        out.append(rec)
    return out


def model_bound(n):
    L = codec.lib()
    L.pna_deflate_bound.restype = codec.ctypes.c_size_t
    L.pna_deflate_bound.argtypes = [codec.ctypes.c_size_t]
    return L.pna_deflate_bound(n)


def model_stream(plain, level):
    return codec.deflate_model_compress(plain, codec.params_for_level(level, deflate=True))


# ----------------------------------------------------------------------------- the cases

def _geometric(seed, n, nsym, ratio):
    """i.i.d. bytes, geometric over a shuffled alphabet"""
    rnd = random.Random(seed)
    al = list(range(256)); rnd.shuffle(al)
    return bytes(rnd.choices(al[:nsym], [ratio ** -i for i in range(nsym)], k=n))


def _mixture(seed, n, head, tail, ratio, frac):
    """i.i.d. bytes: a near-uniform head of `head` symbols with `frac` of the mass, a geometric tail of `tail` symbols"""
    rnd = random.Random(seed)
    al = list(range(256)); rnd.shuffle(al)
    w = [frac / head * (1 + 0.1 * rnd.random()) for _ in range(head)] + [(1 - frac) * ratio ** -(i + 1) for i in range(tail)]
    return bytes(rnd.choices(al[:head + tail], w, k=n))


def _shuffled(seed, counts):
    """every byte value v counts[v] times, in a seeded random order"""
    buf = [v for v, c in sorted(counts.items()) for _ in range(c)]
    random.Random(seed).shuffle(buf)
    return bytes(buf)


def _noise(seed, n):
    return random.Random(seed).randbytes(n)


# B: (seed, bytes, head, tail, ratio, head mass) -- the winners of a search over 3 000 seeds for a code-length code deeper than 7
B_PARAMS = {"B.up1_down2_17k": (49, 17000, 100, 24, 2.0, 0.7), "B.up3_down2_30k": (75, 30000, 100, 31, 1.7, 0.7),
            "B.up2_down2_60k": (21, 60000, 100, 13, 2.0, 0.9), "B.up1_down0_30k": (20, 30000, 100, 37, 2.0, 0.9)}


def _gaps_to_used(first, gaps, fill_from=None):
    """byte values: `first`, then one more behind each gap of unused values; from fill_from on every value up to 255 is used"""
    used, v = [first], first
    for g in gaps:
        v += g + 1
        used.append(v)
    assert v <= 255
    if fill_from is not None:
        assert fill_from > v
        used += range(fill_from, 256)
    return used


def _e_entry(seed, used):
    """every value of `used` equally often, shuffled, at least 96 bytes (below that the block is stored and shows no table): the lit/len lengths of the
    literals are zero exactly off `used`; many values give no match (six bytes do not repeat), a few values do give some"""
    return _shuffled(seed, {v: max(2, -(-96 // len(used))) for v in used})


# E: name -> byte values used.  The gaps between them are the zero runs of the lit/len lengths.
E_USED = {
    "E.gaps_1_2_3_10_11_12_137": _gaps_to_used(0, [1, 2, 3, 10, 11, 12, 137], 250),
    "E.gap_138": _gaps_to_used(5, [138], 200),
    "E.gap_139": _gaps_to_used(5, [139, 2], 200),
    "E.gap_140": _gaps_to_used(3, [140, 10], 210),
    "E.gap_141": _gaps_to_used(2, [141, 11]),
    "E.gap_148": _gaps_to_used(1, [148, 3], 220),
    "E.gap_149": _gaps_to_used(0, [149, 12, 1], 230),
    "E.gap_255_front": [255],
    "E.gap_255_back": [0],
    # a run that ends at 63 / starts at 64 / crosses 63|64: the same at 127|128, 191|192, and a run that ends at 255 (256 is the end-of-block symbol: never zero)
    "E.end_63": [0, 50, 64, 65, 130] + list(range(250, 256)),
    "E.start_64": [1, 63, 80, 127, 129] + list(range(240, 256)),
    "E.cross_64": [2, 40, 100, 255],
    "E.end_127": [3, 120, 128, 254],
    "E.start_128": [127, 131, 255],
    "E.cross_128": [60, 126, 130, 140, 255],
    "E.end_191": [100, 180, 192, 200, 255],
    "E.start_192": [191, 203, 255],
    "E.cross_192": [0, 64, 128, 189, 194, 255],
    "E.end_255": [0, 252],
    "E.whole_waves_empty": [63, 192],
}


def _plant(buf, length, dist):
    """append a copy of `length` bytes from `dist` back (overlapping copies repeat their period)"""
    st = len(buf) - dist
    assert st >= 0
    for k in range(length):
        buf.append(buf[st + k])


def _f_filler(rnd, n):
    return bytes(rnd.choices(_F_ALPHA, k=n))


_F_ALPHA = list(range(32, 96))                                 # 64 values: six bits a byte, so the blocks stay dynamic; six bytes hardly ever repeat
F_FAR = (4097, 6144, 6145, 8192, 8193, 12288, 12289, 16384, 16385, 24576, 24577, 32768)
F_NEAR = tuple(sorted({d for c in range(24) for d in dist_range(c)}))


def _f_lengths(seed):
    """every match length 6 .. 258 planted once as a copy from 4 097 .. 32 768 bytes back (the sources lie before the current 4 096-byte tile at every such distance;
    they start on even positions: the sets that insert even positions only find the whole copy), all 256 byte values as literals, every far distance code's two ends"""
    rnd = random.Random(seed)
    buf = bytearray(range(256)) + bytearray(_f_filler(rnd, 4400 - 256))
    # (the table has 24 512 slots and keeps the latest position of a slot: the farther back a source, the likelier it is overwritten and the copy found a
    # byte or two late -- so every length comes from just over a tile back, and every far distance several times)
    plan = [(length, dist + 2 * (length % 3)) for dist in (4097, 4301) for length in list(range(6, 259)) + [258, 257, 6]]
    plan += [(0, 0)] + [(9 + 5 * k, dist) for k in range(4) for dist in F_FAR]
    for length, dist in plan:
        if not length:                  # fresh bytes for the far copies to come from: what lies before is copies of copies, whose bytes recur every 4 100 or so
            buf += _f_filler(rnd, 33000)
            continue
        if (len(buf) - dist) & 1:
            buf.append(rnd.choice(_F_ALPHA))
        st = len(buf) - dist
        while buf[st - 1] == buf[-1]:                               # the byte in front must differ, or the match starts earlier
            buf[-1] = rnd.choice(_F_ALPHA)
        _plant(buf, length, dist)
        sep = rnd.choice(_F_ALPHA)
        while sep == buf[st + length]:                              # ... and the byte behind, or it runs on
            sep = rnd.choice(_F_ALPHA)
        buf.append(sep)
        buf += _f_filler(rnd, 3)
    return bytes(buf)


def _f_near(seed):
    """short distances: a source must lie before the tile of the position that finds it, so the copies start at a tile's first position (and at its second, for
    the sets whose table holds even positions only: an odd distance needs an odd position)"""
    rnd = random.Random(seed)
    buf = bytearray(_f_filler(rnd, 4096))
    for dist in F_NEAR:
        for shift in (0, 1):
            t = (len(buf) + dist + 4096) // 4096 * 4096
            buf += _f_filler(rnd, t + shift - len(buf))
            if dist >= 6:                                            # a unit of its own in front of the tile, so that the nearest source is `dist` back
                buf[len(buf) - dist:] = bytes(rnd.randrange(96, 160) for _ in range(dist))
            else:
                buf[len(buf) - dist:] = bytes(rnd.sample(range(160, 200), dist))
            _plant(buf, min(258, 7 + dist % 11), dist)
            buf.append(rnd.randrange(200, 256))
    return bytes(buf)


def _dense_tile(seed):
    """1 MiB of eight frequent symbols (weights 100 .. 2: their chain of merges pushes everything rarer below depth 15); one aligned 2 048-byte stretch at
    100 * 2048 of 210 rare symbols, about ten of each: every one of its literals costs 15 bits"""
    rnd = random.Random(seed)
    buf = bytearray(rnd.choices(range(8), [100, 50, 30, 20, 10, 5, 3, 2], k=SEG))
    rare = [v for v in range(8, 218) for _ in range(10)][:TILE]
    rare += rnd.choices(range(8, 218), k=TILE - len(rare))
    rnd.shuffle(rare)
    buf[100 * TILE:101 * TILE] = bytes(rare)
    return bytes(buf)


def _alternating(seed, blocks, tail=0):
    """blocks of noise (stored) and of skewed bytes without matches to speak of (dynamic), alternating, under one table"""
    out = bytearray()
    for b in range(blocks):
        out += _noise(seed + b, BLK) if b & 1 == 0 else _geometric(seed + b, BLK, 12, 1.4)
    return bytes(out) + _geometric(seed + 99, tail, 12, 1.4)


def _eob_sweep(seed, k):
    return _geometric(seed, 3000 + k, 20, 1.3)


def build_cases():
    """[(name, plain bytes, levels)]"""
    c = []
    add = lambda name, plain, levels=(6,): c.append((name, bytes(plain), tuple(levels)))
    # A: deep codes
    add("A.geo_2.0_x28", _geometric(1, SEG, 28, 2.0), (6,))
    add("A.geo_1.7_x40", _geometric(1, SEG, 40, 1.7), (9,))
    add("A.geo_1.1_x256", _geometric(1, SEG, 256, 1.1), (1,))
    add("A.geo_1.8_x30_128k", _geometric(3, BLK, 30, 1.8), (6,))
    # B: the code-length code at its limit of 7
    for name, prm in B_PARAMS.items():
        add(name, _mixture(*prm), (6,))
    # C: ties
    rnd = random.Random(11)
    perms = b"".join(bytes(rnd.sample(range(256), 256)) for _ in range(16))
    add("C.permutations_x16_twice", perms + perms, (1, 6, 9))          # (the second half is all matches: without it the block would be stored and show no table)
    add("C.powers_of_two", _shuffled(12, {10 * i + 1: 1 << i for i in range(12)}), (1, 6))
    add("C.equal_but_one", _shuffled(13, {**{v: 8 for v in range(0, 200, 2)}, 201: 300}), (6,))
    pairs = _shuffled(14, {v: 2 for v in range(256)})
    add("C.equal_pairs_twice", pairs + pairs, (6,))
    add("C.two_symbols", _shuffled(15, {7: 700, 250: 300}), (1, 6))
    add("C.three_symbols", _shuffled(16, {0: 500, 128: 300, 255: 200}), (6,))
    add("C.four_symbols", _shuffled(17, {1: 400, 2: 400, 3: 400, 4: 400}), (6, 9))
    add("C.all_283", _f_lengths(21), (1, 9))
    add("C.largest_header", _shuffled(18, {v: 1 + (v * 7919 % 13) * (v % 3) + (1 << (v % 14)) for v in range(0, 256, 2)}) + _f_lengths(22)[:70000], (6,))
    # D: degenerate distance codes
    add("D.no_match", _shuffled(31, {**{v: 4 for v in range(100)}, 200: 150}), (1, 6))
    d1 = _shuffled(32, {**{v: 5 for v in range(3, 120)}, 222: 115})
    add("D.one_distance", d1 + d1[100:140] + bytes(range(130, 160)), (6,))
    add("D.two_distances", d1 + d1[100:140] + bytes(range(130, 160)) + d1[660:700] + bytes(range(160, 169)), (6,))
    add("D.distance_32768", _f_lengths(23), (6,))
    for n in (0, 1, 2, 5):
        add("D.entry_of_%d" % n, b"\xa7\x00\xff\x00\xa7"[:n], (0, 1, 6, 9))
    # E: zero-run edges
    for k, (name, used) in enumerate(E_USED.items()):
        add(name, _e_entry(50 + k, used), (6,))
    # F: symbols and extra bits
    add("F.lengths", _f_lengths(24), (1, 6, 9))
    add("F.near", _f_near(25), (1, 6, 9))
    # G: block plan and writer
    add("G.stored_3_pieces", _noise(61, BLK), (6,))
    add("G.alternating", _alternating(62, 6), (6,))
    add("G.final_stored", _geometric(63, BLK, 12, 1.4) + _noise(64, 5000), (6,))
    add("G.final_dynamic", _noise(65, BLK) + _geometric(66, 5000, 12, 1.4), (6,))
    add("G.last_block_1_byte", _geometric(67, BLK, 30, 1.2) + b"q", (1, 6))
    add("G.dense_tile", _dense_tile(68), (6,))
    for k in range(10):
        add("G.eob_sweep_%d" % k, _eob_sweep(70 + k, k), (6,))
    for n in (0, 1, 65535, 65536, BLK, BLK + 1, 3 * BLK + 7):
        add("G.level0_%d" % n, _noise(80, n), (0,))
    # H: Adler-32
    for n in (1, 5552, 5553, 65521, BLK, SEG + 1, 3 * SEG + 17):
        add("H.ff_%d" % n, b"\xff" * n, (6,) if n > BLK else (0, 6))
    for n in (5553, 65521, SEG + 1):
        add("H.f1_%d" % n, b"\xf1" * n, (1,))
    add("H.ff_00_blocks_2mib", b"".join((b"\xff" if b & 1 == 0 else b"\x00") * BLK for b in range(16)), (6,))
    return c


_CASES = None


def cases():
    global _CASES
    if _CASES is None:
        _CASES = build_cases()
    return _CASES


# ----------------------------------------------------------------------------- what a stream reaches

RUN_LENGTHS = (1, 2, 3, 10, 11, 12, 137, 138, 139, 140, 141, 148, 149, 255)
# positions in the concatenated lit/len + distance lengths; k_dstats looks at them in slots of 64 (a wave), rounds of T = 64 or 256
BORDERS = ("end_63", "start_64", "cross_64", "end_127", "start_128", "cross_128", "end_191", "start_192", "cross_192", "end_255", "start_257",
           "run_in_distances", "run_ends_sequence")
BRANCHES = (["ll_clamp", "ll_up", "ll_down", "d_clamp", "d_up", "d_down", "cl_clamp", "cl_up", "cl_down", "n0", "n1", "n2", "n283", "tie"]
            + ["run_%d" % r for r in RUN_LENGTHS] + list(BORDERS)
            + ["stored_3_pieces", "mixed_plan", "final_stored", "final_dynamic"] + ["eob_bit_%d" % k for k in range(8)])


def branches(records):
    """names of BRANCHES that the segments of one analysed stream reach"""
    out = set()
    for r in records:
        if [65535, 65535, 2] in r["pieces"]:
            out.add("stored_3_pieces")
        if "S" in r["plan"] and "D" in r["plan"]:
            out.add("mixed_plan")
        out.update("eob_bit_%d" % k for k in r["eob_bits"])
        if r["ll"] is None:
            continue
        for key in ("ll", "d", "cl"):
            f = r[key]
            out.update(name for name, hit in (("%s_clamp" % key, f["clamp"]), ("%s_up" % key, f["up"]), ("%s_down" % key, f["down"])) if hit)
        if r["ll"]["ties"] or r["d"]["ties"] or r["cl"]["ties"]:
            out.add("tie")
        if r["d"]["n"] <= 2:
            out.add("n%d" % r["d"]["n"])
        if r["ll"]["n"] == 283 and r["hlit"] == 29:
            out.add("n283")
        for a, ln in r["runs"]:
            e = a + ln - 1
            if ln in RUN_LENGTHS:
                out.add("run_%d" % ln)
            for b in (64, 128, 192):
                if e == b - 1: out.add("end_%d" % (b - 1))
                if a == b: out.add("start_%d" % b)
                if a < b <= e: out.add("cross_%d" % b)
            if e == 255: out.add("end_255")
            if a == 257: out.add("start_257")
            if a >= r["nll"]: out.add("run_in_distances")
            if e == len(r["seq"]) - 1: out.add("run_ends_sequence")
    last = records[-1] if records else None
    if last and len(last["plan"]) + (len(records) - 1) * 8 > 1:
        out.add("final_stored" if last["plan"][-1] == "S" else "final_dynamic")
    return out


_FACTS = {}


def facts(name, level):
    """(model stream, analysed records) of one case at one level, computed once per process"""
    if (name, level) not in _FACTS:
        plain = next(p for n, p, _ in cases() if n == name)
        stream = model_stream(plain, level)
        _FACTS[name, level] = (stream, analyse(stream, plain))
    return _FACTS[name, level]
