// xz_enc_core.h -- the .xz / LZMA2 encoder's algorithm, once: a chunk's sequences -> LZMA coding decisions -> the range encoder; the chunk and block
// headers, the Index and the stream footer.  __host__ __device__ inline code in the style of xz_core.h (whose model layout XZP_* and CRC arithmetic it
// shares): k_xzenc.hip runs it on the device (one wave per chunk: every lane walks the same instruction stream over wave-uniform values, lane 0 stores
// the model and the output bytes), tests/xz_enc_core builds it with g++ alone (one "lane") and hands the streams to liblzma and to xz_core.h's decoder.
//
// What is written (include/pna_gpu.h has the rules): per entry one .xz stream, check CRC64; one block per 1 MiB segment, filter LZMA2 with a 1 MiB
// dictionary; one LZMA2 chunk per LZ block of at most 64 KiB.  Every LZMA chunk resets the state and carries the properties (lc 3, lp 0, pb 2), none resets
// the dictionary but a block's first: the chunks of a segment are independent range-coding jobs whose matches reach back over the whole segment.
// Safety: the coder reads seg[0, seg_len) only and writes o[0, cap) only; at a sequence that does not fit its chunk or reaches in front of the segment it
// codes the rest of the chunk as literals.
#pragma once
#include "xz_core.h"

enum { XZE_PROPS = 93 /* (pb * 5 + lp) * 9 + lc */, XZE_DICT_BYTE = 16 /* 1 MiB */, XZE_MAX_LEN = 273, XZE_MIN_LEN = 2, XZE_CHUNK_MAX = 65536,
       XZE_PROBS = XZP_LIT + (0x300 << 3) /* 7 992 */, XZE_BLOCK_HEADER = 12, XZE_STREAM_HEADER = 12, XZE_STREAM_FOOTER = 12 };
// a sequence as the LZ stage packs it (pna_dev.h seq_pack): literal run, match length, match distance
XZ_HD uint32_t xze_seq_off(uint64_t s) { return (uint32_t)(s & 0xFFFFF); }
XZ_HD uint32_t xze_seq_ml(uint64_t s) { return (uint32_t)((s >> 20) & 0x3FFFF); }
XZ_HD uint32_t xze_seq_ll(uint64_t s) { return (uint32_t)((s >> 38) & 0x3FFFF); }

// ---- sizes
// the worst case of an entry of n bytes: every chunk stored (3 bytes per LZ block of the smallest size, 8 KiB -- xze_chunk stores every chunk whose LZMA form,
// header included, would not be smaller than that), 24 bytes per block (header, end marker, padding, check), per entry the stream header and footer, the
// Index's framing (32 bytes) + its record count + at most 8 bytes per record
XZ_HD uint64_t xze_bound(uint64_t n) {
    const uint64_t nblk = (n + (1u << 20) - 1) >> 20, nchunk = (n + 8191) >> 13;
    return n + 3 * nchunk + nblk * (24 + 8) + 32 + 9;
}
XZ_HD uint32_t xze_chunk_bytes(uint32_t lzma_size, uint32_t clen) { return lzma_size ? 6u + lzma_size : 3u + clen; }   // lzma_size 0: stored
XZ_HD uint64_t xze_block_unpadded(uint64_t chunk_bytes) { return XZE_BLOCK_HEADER + chunk_bytes + 1 + 8; }              // what the Index records
XZ_HD uint64_t xze_block_padded(uint64_t chunk_bytes) { return (xze_block_unpadded(chunk_bytes) + 3) & ~3ull; }

// ---- the container's fixed parts
XZ_HD void xze_le32(uint8_t *o, uint32_t v) { o[0] = (uint8_t)v; o[1] = (uint8_t)(v >> 8); o[2] = (uint8_t)(v >> 16); o[3] = (uint8_t)(v >> 24); }
XZ_HD void xze_stream_header(uint8_t *o) {
    o[0] = 0xFD; o[1] = '7'; o[2] = 'z'; o[3] = 'X'; o[4] = 'Z'; o[5] = 0; o[6] = 0; o[7] = XZ_CHECK_CRC64;
    xze_le32(o + 8, xz_crc32(o + 6, 2));
}
XZ_HD void xze_stream_footer(uint8_t *o, uint64_t index_size) {
    xze_le32(o + 4, (uint32_t)(index_size / 4 - 1));
    o[8] = 0; o[9] = XZ_CHECK_CRC64;
    xze_le32(o, xz_crc32(o + 4, 6));
    o[10] = 'Y'; o[11] = 'Z';
}
// no size fields, one filter: LZMA2 (id 0x21, one property byte: the dictionary size)
XZ_HD void xze_block_header(uint8_t *o) {
    o[0] = XZE_BLOCK_HEADER / 4 - 1; o[1] = 0; o[2] = 0x21; o[3] = 1; o[4] = XZE_DICT_BYTE; o[5] = 0; o[6] = 0; o[7] = 0;
    xze_le32(o + 8, xz_crc32(o, 8));
}
// the header of the chunk of clen input bytes (lzma_size 0: stored); first: the block's first chunk (it resets the dictionary).  Returns its length.
XZ_HD uint32_t xze_chunk_header(uint8_t *o, bool first, uint32_t lzma_size, uint32_t clen) {
    const uint32_t u = clen - 1;
    if (!lzma_size) { o[0] = first ? 1 : 2; o[1] = (uint8_t)(u >> 8); o[2] = (uint8_t)u; return 3; }
    const uint32_t cs = lzma_size - 1;
    o[0] = (uint8_t)((first ? 0xE0u : 0xC0u) | (u >> 16)); o[1] = (uint8_t)(u >> 8); o[2] = (uint8_t)u; o[3] = (uint8_t)(cs >> 8); o[4] = (uint8_t)cs; o[5] = XZE_PROPS;
    return 6;
}
// the Index, record by record; o == null: only counted.  begin, one record per block, end (padding + CRC32): end returns the Index's size.
struct XzeIndex { uint8_t *o; uint64_t n; uint32_t crc; };
XZ_HD void xze_idx_byte(XzeIndex &w, uint32_t b) {
    if (w.o) w.o[w.n] = (uint8_t)b;
    w.n++;
    w.crc ^= b;
    for (int k = 0; k < 8; k++) w.crc = (w.crc >> 1) ^ (XZ_POLY32 & (0u - (w.crc & 1u)));
}
XZ_HD void xze_idx_vli(XzeIndex &w, uint64_t v) { while (v >= 0x80) { xze_idx_byte(w, (uint32_t)(v & 0x7F) | 0x80u); v >>= 7; } xze_idx_byte(w, (uint32_t)v); }
XZ_HD void xze_idx_begin(XzeIndex &w, uint8_t *o, uint64_t nrec) { w.o = o; w.n = 0; w.crc = 0xFFFFFFFFu; xze_idx_byte(w, 0); xze_idx_vli(w, nrec); }
XZ_HD void xze_idx_record(XzeIndex &w, uint64_t unpadded, uint64_t usize) { xze_idx_vli(w, unpadded); xze_idx_vli(w, usize); }
XZ_HD uint64_t xze_idx_end(XzeIndex &w) {
    while (w.n & 3) xze_idx_byte(w, 0);
    if (w.o) xze_le32(w.o + w.n, ~w.crc);
    return w.n + 4;
}

// ---- the segment's bytes as the coder reads them: in order, with jumps over the matches
struct XzeSrc {
    const uint8_t *p; uint32_t len;
#if XZ_DEV
    uint32_t base, w;                   // a window of 256 bytes from `base` on, four per lane
#endif
};
XZ_HD uint32_t xze_src_byte(XzeSrc &s, uint32_t pos, uint32_t lane) {
#if XZ_DEV
    uint32_t d = pos - s.base;
    if (d >= 256) {
        s.base = pos & ~255u; d = pos - s.base;
        const uint32_t a = s.base + lane * 4;
        uint32_t w = 0;
        for (uint32_t k = 0; k < 4; k++) if (a + k < s.len) w |= (uint32_t)s.p[a + k] << (8 * k);
        s.w = w;
    }
    return (XZ_LANE_OF(s.w, d >> 2) >> ((d & 3) * 8)) & 255u;
#else
    (void)lane;
    return s.p[pos];
#endif
}

// ---- the range encoder: low / range / cache with carry.  Bytes go to o[0, cap); `over`: one did not fit.
struct XzeRc { uint64_t low; uint32_t range, cache, pending, out, cap, over; uint8_t *o; };
XZ_HD void xze_rc_init(XzeRc &rc, uint8_t *o, uint32_t cap) { rc.low = 0; rc.range = 0xFFFFFFFFu; rc.cache = 0; rc.pending = 1; rc.out = 0; rc.cap = cap; rc.over = 0; rc.o = o; }
XZ_HD void xze_put(XzeRc &rc, uint32_t b, uint32_t lane) {
    if (rc.out < rc.cap) { if (lane == 0) rc.o[rc.out] = (uint8_t)b; }
    else rc.over = 1;
    rc.out++;
}
XZ_HD void xze_shift_low(XzeRc &rc, uint32_t lane) {
    if ((uint32_t)rc.low < 0xFF000000u || (uint32_t)(rc.low >> 32) != 0) {
        const uint32_t carry = (uint32_t)(rc.low >> 32);
        do { xze_put(rc, rc.cache + carry, lane); rc.cache = 0xFF; } while (--rc.pending != 0);
        rc.cache = (uint32_t)(rc.low >> 24) & 0xFFu;
    }
    rc.pending++;
    rc.low = (rc.low & 0x00FFFFFFull) << 8;
}
XZ_HD void xze_bit(XzeRc &rc, uint16_t *pr, uint32_t bit, uint32_t lane) {
    const uint32_t p = XZ_U(*pr);
    const uint32_t bound = (rc.range >> 11) * p;
    if (!bit) { rc.range = bound; xz_put_prob(pr, p + ((2048u - p) >> 5), lane); }
    else { rc.low += bound; rc.range -= bound; xz_put_prob(pr, p - (p >> 5), lane); }
    while (rc.range < (1u << 24)) { rc.range <<= 8; xze_shift_low(rc, lane); }
}
XZ_HD void xze_tree(XzeRc &rc, uint16_t *pr, uint32_t nbits, uint32_t v, uint32_t lane) {
    uint32_t m = 1;
    for (uint32_t i = nbits; i-- > 0;) { const uint32_t b = (v >> i) & 1u; xze_bit(rc, pr + m, b, lane); m = (m << 1) | b; }
}
XZ_HD void xze_tree_rev(XzeRc &rc, uint16_t *pr, uint32_t nbits, uint32_t v, uint32_t lane) {
    uint32_t m = 1;
    for (uint32_t i = 0; i < nbits; i++) { const uint32_t b = (v >> i) & 1u; xze_bit(rc, pr + m, b, lane); m = (m << 1) | b; }
}
XZ_HD void xze_direct(XzeRc &rc, uint32_t nbits, uint32_t v, uint32_t lane) {
    for (uint32_t i = nbits; i-- > 0;) {
        rc.range >>= 1;
        rc.low += rc.range & (0u - ((v >> i) & 1u));
        while (rc.range < (1u << 24)) { rc.range <<= 8; xze_shift_low(rc, lane); }
    }
}
XZ_HD void xze_len(XzeRc &rc, uint16_t *L, uint32_t pos_state, uint32_t len, uint32_t lane) {
    const uint32_t l = len - 2;
    if (l < 8) { xze_bit(rc, L, 0, lane); xze_tree(rc, L + XZP_LEN_LOW + pos_state * 8, 3, l, lane); return; }
    xze_bit(rc, L, 1, lane);
    if (l < 16) { xze_bit(rc, L + 1, 0, lane); xze_tree(rc, L + XZP_LEN_MID + pos_state * 8, 3, l - 8, lane); return; }
    xze_bit(rc, L + 1, 1, lane);
    xze_tree(rc, L + XZP_LEN_HIGH, 8, l - 16, lane);
}
XZ_HD uint32_t xze_log2(uint32_t v) { uint32_t n = 0; while (v >>= 1) n++; return n; }

// the coder's state between the decisions of one chunk
struct XzeState { uint32_t state, rep0, rep1, rep2, rep3; };
XZ_HD void xze_literal(XzeRc &rc, uint16_t *probs, XzeState &st, XzeSrc &src, uint32_t pos, uint32_t lane) {
    xze_bit(rc, probs + XZP_IS_MATCH + st.state * 16 + (pos & 3u), 0, lane);
    const uint32_t prev = pos ? xze_src_byte(src, pos - 1, lane) : 0u;
    const uint32_t byte = xze_src_byte(src, pos, lane);
    uint16_t *lit = probs + XZP_LIT + 0x300u * (prev >> 5);
    uint32_t sym = 1, k = 8;
    if (st.state >= 7) {                                                  // behind a match: the byte the match would have gone on with steers the model
        const uint32_t mb = XZ_U(src.p[pos - st.rep0 - 1]);
        while (k > 0) {
            k--;
            const uint32_t mbit = (mb >> k) & 1u, b = (byte >> k) & 1u;
            xze_bit(rc, lit + ((1u + mbit) << 8) + sym, b, lane);
            sym = (sym << 1) | b;
            if (mbit != b) break;
        }
    }
    while (k > 0) { k--; const uint32_t b = (byte >> k) & 1u; xze_bit(rc, lit + sym, b, lane); sym = (sym << 1) | b; }
    st.state = st.state < 4 ? 0 : (st.state < 10 ? st.state - 3 : st.state - 6);
}
// a match of len (2 .. 273) bytes at distance dist; a distance among the four latest is a repeat
XZ_HD void xze_match(XzeRc &rc, uint16_t *probs, XzeState &st, uint32_t pos, uint32_t len, uint32_t dist, uint32_t lane) {
    const uint32_t ps = pos & 3u, r = dist - 1, s0 = st.state;
    xze_bit(rc, probs + XZP_IS_MATCH + s0 * 16 + ps, 1, lane);
    if (r == st.rep0 || r == st.rep1 || r == st.rep2 || r == st.rep3) {
        xze_bit(rc, probs + XZP_IS_REP + s0, 1, lane);
        if (r == st.rep0) { xze_bit(rc, probs + XZP_IS_REP0 + s0, 0, lane); xze_bit(rc, probs + XZP_IS_REP0_LONG + s0 * 16 + ps, 1, lane); }
        else {
            xze_bit(rc, probs + XZP_IS_REP0 + s0, 1, lane);
            if (r == st.rep1) xze_bit(rc, probs + XZP_IS_REP1 + s0, 0, lane);
            else {
                xze_bit(rc, probs + XZP_IS_REP1 + s0, 1, lane);
                if (r == st.rep2) xze_bit(rc, probs + XZP_IS_REP2 + s0, 0, lane);
                else { xze_bit(rc, probs + XZP_IS_REP2 + s0, 1, lane); st.rep3 = st.rep2; }
                st.rep2 = st.rep1;
            }
            st.rep1 = st.rep0; st.rep0 = r;
        }
        xze_len(rc, probs + XZP_REP_LEN, ps, len, lane);
        st.state = s0 < 7 ? 8 : 11;
        return;
    }
    xze_bit(rc, probs + XZP_IS_REP + s0, 0, lane);
    st.rep3 = st.rep2; st.rep2 = st.rep1; st.rep1 = st.rep0; st.rep0 = r;
    xze_len(rc, probs + XZP_MATCH_LEN, ps, len, lane);
    st.state = s0 < 7 ? 7 : 10;
    uint32_t slot = r;
    if (r >= 4) { const uint32_t nb = xze_log2(r); slot = nb * 2 + ((r >> (nb - 1)) & 1u); }
    xze_tree(rc, probs + XZP_POS_SLOT + (len < 6 ? len - 2 : 3) * 64, 6, slot, lane);
    if (slot >= 4) {
        const uint32_t fb = (slot >> 1) - 1, base = (2u | (slot & 1u)) << fb, red = r - base;
        if (slot < 14) xze_tree_rev(rc, probs + XZP_POS_SPECIAL + base - slot, fb, red, lane);
        else { xze_direct(rc, fb - 4, red >> 4, lane); xze_tree_rev(rc, probs + XZP_POS_ALIGN, 4, red & 15u, lane); }
    }
}

// One chunk: bytes [c0, c0 + clen) of the segment seg[0, seg_len), parsed into nseq sequences (the rest: literals) -> its LZMA form in o[0, cap).
// probs: room for XZE_PROBS entries (LDS on the device).  Returns the LZMA form's size, or 0: the chunk is to be STORED.  An LZMA chunk costs 6 bytes of
// header, a stored one 3, so the chunk is stored unless its LZMA form is at least 4 bytes shorter than its input (size + 3 < clen): no chunk ever costs
// more than 3 + clen bytes, which is what xze_bound counts.  The coder stops as soon as the bytes written and pending reach clen - 3, so with cap >= clen
// no byte is refused.  Every lane gets the same.
XZ_HD uint32_t xze_chunk(const uint8_t *seg, uint32_t seg_len, uint32_t c0, uint32_t clen, const uint64_t *seqs, uint32_t nseq, uint16_t *probs,
                         uint8_t *o, uint32_t cap, uint32_t lane) {
    XZ_SYNC();
    for (uint32_t i = lane; i < (uint32_t)XZE_PROBS; i += XZ_LANES) probs[i] = 1024;
    XZ_SYNC();
    XzeRc rc; xze_rc_init(rc, o, cap);
    XzeState st; st.state = 0; st.rep0 = st.rep1 = st.rep2 = st.rep3 = 0;
    XzeSrc src; src.p = seg; src.len = seg_len;
#if XZ_DEV
    src.base = 0xFFFFF000u; src.w = 0;                                    // (no window yet: the first read fills it)
    uint32_t wlo = 0, whi = 0;                                            // 64 sequences at a time, one per lane
#endif
    const uint32_t end = c0 + clen;
    uint32_t pos = c0;
    for (uint32_t i = 0; i <= nseq; i++) {                                // (the turn behind the last sequence: the literals up to the chunk's end)
        uint32_t ll = end - pos, ml = 0, dist = 0;
        if (i < nseq) {
#if XZ_DEV
            if ((i & 63u) == 0) { const uint64_t s = i + lane < nseq ? seqs[i + lane] : 0ull; wlo = (uint32_t)s; whi = (uint32_t)(s >> 32); }
            const uint64_t s = ((uint64_t)XZ_LANE_OF(whi, i & 63u) << 32) | XZ_LANE_OF(wlo, i & 63u);
#else
            const uint64_t s = seqs[i];
#endif
            ll = xze_seq_ll(s); ml = xze_seq_ml(s); dist = xze_seq_off(s);
            // (a sequence that does not fit the chunk or reaches in front of the segment -- the LZ stage writes none --: the rest of the chunk as literals)
            if (ll > end - pos || ml > end - pos - ll || (ml && (ml < (uint32_t)XZE_MIN_LEN || dist == 0 || dist > pos + ll))) { i = nseq; ll = end - pos; ml = 0; }
        }
        for (uint32_t k = 0; k < ll; k++) {
            if (rc.out + rc.pending + 3 >= clen) return 0;
            xze_literal(rc, probs, st, src, pos, lane);
            pos++;
        }
        while (ml) {                                                      // pieces of at most 273 bytes, none shorter than 2
            if (rc.out + rc.pending + 3 >= clen) return 0;
            const uint32_t piece = ml <= (uint32_t)XZE_MAX_LEN ? ml : (ml - XZE_MAX_LEN < (uint32_t)XZE_MIN_LEN ? XZE_MAX_LEN - 1 : XZE_MAX_LEN);
            xze_match(rc, probs, st, pos, piece, dist, lane);
            pos += piece; ml -= piece;
        }
    }
    for (int k = 0; k < 5; k++) xze_shift_low(rc, lane);
    return (rc.over || rc.out + 3 >= clen) ? 0u : rc.out;
}
