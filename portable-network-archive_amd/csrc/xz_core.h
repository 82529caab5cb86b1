// xz_core.h -- the .xz / LZMA2 decoder's algorithm, once: container walk, chunk walk, range decoder, probability model, the CRCs' arithmetic.
// __host__ __device__ inline code: k_xz.hip runs it on the device (one wave per block: every lane walks the same instruction stream over wave-uniform
// values -- what comes out of memory goes through readfirstlane --, lane 0 stores the model and the literals, all 64 lanes copy matches and uncompressed
// chunks); tests/xz_core builds it with g++ alone (one "lane") and compares it with liblzma.
//
// What is read (include/pna_gpu.h has the rules): one .xz stream, blocks located from its Index, one filter (LZMA2), checks None / CRC32 / CRC64.
// Safety: every read is bounds-checked against the stream / the block's compressed bytes, every write against the block's decoded range; every loop
// iteration consumes input or produces output, and running out of either ends the block with a status.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define XZ_HD __host__ __device__ inline
#else
#define XZ_HD inline
#endif
#if defined(__HIP_DEVICE_COMPILE__)
#define XZ_DEV 1
#define XZ_LANES 64u
#define XZ_U(x) ((uint32_t)__builtin_amdgcn_readfirstlane((int)(x)))                                       // a value every lane holds: onto the scalar unit
#define XZ_LANE_OF(v, l) ((uint32_t)__builtin_amdgcn_readlane((int)(v), (int)XZ_U(l)))
// lanes exchange bytes through memory (the model in LDS, the dictionary in the output buffer): a wave's memory instructions are issued in order, the
// fence keeps the compiler from moving them across
#define XZ_SYNC() do { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront"); } while (0)
#else
#define XZ_DEV 0
#define XZ_LANES 1u
#define XZ_U(x) ((uint32_t)(x))
#define XZ_LANE_OF(v, l) ((uint32_t)(v))
#define XZ_SYNC() do { } while (0)
#endif

enum { XZ_OK = 0, XZ_CORRUPT = 1, XZ_UNSUPPORTED = 2, XZ_SIZE = 3 };      // = ZFrame::status of the other decoders
enum { XZ_CHECK_NONE = 0, XZ_CHECK_CRC32 = 1, XZ_CHECK_CRC64 = 4, XZ_CHECK_SHA256 = 10 };
enum { XZ_UNSUP_CHECK = 1, XZ_UNSUP_SHA256 = 2, XZ_UNSUP_FILTER = 3, XZ_UNSUP_BIG_BLOCK = 4, XZ_UNSUP_HEADER = 5 };   // XzScan::why

// ---- the probability model: 16-bit entries, offsets into one array
enum {
    XZP_IS_MATCH = 0, XZP_IS_REP = 192, XZP_IS_REP0 = 204, XZP_IS_REP1 = 216, XZP_IS_REP2 = 228, XZP_IS_REP0_LONG = 240, XZP_POS_SLOT = 432,
    XZP_POS_SPECIAL = 688, XZP_POS_ALIGN = 804, XZP_MATCH_LEN = 820, XZP_REP_LEN = 1334, XZP_LIT = 1848,
    XZP_LEN_LOW = 2, XZP_LEN_MID = 130, XZP_LEN_HIGH = 258
};
XZ_HD uint32_t xz_prob_count(uint32_t lclp) { return (uint32_t)XZP_LIT + (0x300u << lclp); }

struct XzScan { uint32_t status, nblk, check, lclp; uint64_t total; uint32_t why, pad; };    // one stream: what the container walk found
struct XzBlock { uint64_t src, src_len, dst, check_off; uint32_t dst_len, dict, check, stream, status, pad; };   // one block: offsets from the buffers' starts

// ---- CRC arithmetic (reflected bit order: the top bit of the register is x^0)
constexpr uint32_t XZ_POLY32 = 0xEDB88320u;
constexpr uint64_t XZ_POLY64 = 0xC96C5795D7870F42ull;
XZ_HD uint32_t xz_crc32(const uint8_t *p, uint64_t n) {              // headers, Index, footer: short runs, bit by bit
    uint32_t c = 0xFFFFFFFFu;
    for (uint64_t i = 0; i < n; i++) { c ^= p[i]; for (int k = 0; k < 8; k++) c = (c >> 1) ^ (XZ_POLY32 & (0u - (c & 1u))); }
    return ~c;
}
// a * b mod P; both CRCs in a 64-bit register: the CRC-32's values live in its top half (polynomial shifted up, the carry out of bit 32), so one routine serves both
XZ_HD uint64_t xz_poly_of(uint32_t check) { return check == XZ_CHECK_CRC32 ? (uint64_t)XZ_POLY32 << 32 : XZ_POLY64; }
XZ_HD uint64_t xz_gf_mul(uint64_t a, uint64_t b, uint32_t check) {
    const uint64_t poly = xz_poly_of(check), carry = check == XZ_CHECK_CRC32 ? 1ull << 32 : 1ull, keep = 0ull - carry;   // keep: the register's bits
    uint64_t r = 0;
    for (int i = 0; i < 64 && a; i++) {
        if (a >> 63) r ^= b;
        a <<= 1;
        b = ((b >> 1) & keep) ^ (poly & (0ull - (uint64_t)((b & carry) != 0)));
    }
    return r;
}
// x^(8 n) mod P
XZ_HD uint64_t xz_gf_xpow8(uint64_t n, uint32_t check) {
    uint64_t r = 1ull << 63, sq = 1ull << 55;                        // x^0, x^8
    while (n) { if (n & 1) r = xz_gf_mul(r, sq, check); sq = xz_gf_mul(sq, sq, check); n >>= 1; }
    return r;
}
// the raw register (initial value 0, no final xor) over n bytes, table-free; tab: 256 entries of xz_crc_tab_entry, or null
XZ_HD uint64_t xz_crc_tab_entry(uint32_t b, uint64_t poly) {
    uint64_t c = b;
    for (int k = 0; k < 8; k++) c = (c >> 1) ^ (poly & (0ull - (c & 1ull)));
    return c;
}
// (the table is built for the register's LOW-aligned form: CRC-64 as it is, CRC-32 in the low half with its own polynomial)
XZ_HD uint64_t xz_crc_raw(const uint8_t *p, uint64_t n, const uint64_t *tab, uint64_t poly_low) {
    uint64_t c = 0;
    if (tab) for (uint64_t i = 0; i < n; i++) c = tab[(c ^ p[i]) & 255] ^ (c >> 8);
    else for (uint64_t i = 0; i < n; i++) c = xz_crc_tab_entry((uint32_t)((c ^ p[i]) & 255), poly_low) ^ (c >> 8);
    return c;
}
XZ_HD uint64_t xz_poly_low(uint32_t check) { return check == XZ_CHECK_CRC32 ? (uint64_t)XZ_POLY32 : XZ_POLY64; }
// raw register of a piece -> its share of the block's value: times x^(8 * bytes behind the piece).  Registers travel in the TOP-aligned form here.
XZ_HD uint64_t xz_crc_top(uint64_t low, uint32_t check) { return check == XZ_CHECK_CRC32 ? low << 32 : low; }
XZ_HD uint64_t xz_crc_share(uint64_t raw_top, uint64_t bytes_behind, uint32_t check) {
    return xz_gf_mul(raw_top, xz_gf_xpow8(bytes_behind, check), check);
}
// the xor of all shares -> the check value as stored: the initial all-ones run through the block's length, the final xor
XZ_HD uint64_t xz_crc_finish(uint64_t acc_top, uint64_t len, uint32_t check) {
    const uint64_t ones = check == XZ_CHECK_CRC32 ? 0xFFFFFFFF00000000ull : ~0ull;
    const uint64_t v = acc_top ^ xz_gf_mul(ones, xz_gf_xpow8(len, check), check) ^ ones;
    return check == XZ_CHECK_CRC32 ? v >> 32 : v;
}
XZ_HD uint32_t xz_check_size(uint32_t check) { return check == 0 ? 0u : (check <= 3 ? 4u : (check <= 6 ? 8u : (check <= 9 ? 16u : (check <= 12 ? 32u : 64u)))); }

// ---- the container
XZ_HD uint32_t xz_le32(const uint8_t *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }
XZ_HD bool xz_vli(const uint8_t *p, uint64_t &pos, uint64_t end, uint64_t &v) {
    v = 0;
    for (int i = 0; i < 9; i++) {
        if (pos >= end) return false;
        const uint8_t b = p[pos++];
        v |= (uint64_t)(b & 0x7F) << (7 * i);
        if (!(b & 0x80)) return !(b == 0 && i > 0);                  // (a zero byte that is not the first: not the shortest form)
    }
    return false;
}
XZ_HD uint32_t xz_dict_size(uint32_t b) { return b == 40 ? 0xFFFFFFFFu : (2u | (b & 1u)) << (b / 2 + 11); }

// The chunk headers of one block's LZMA2 data (n bytes that decode to dec_len): control bytes, sizes that add up, the end marker as the last byte;
// *lclp = the largest lc + lp of its property bytes (the decode launch's model size).  Each step moves forward by at least one byte.
XZ_HD uint32_t xz_chunk_walk(const uint8_t *p, uint64_t n, uint64_t dec_len, uint32_t *lclp) {
    uint64_t pos = 0, out = 0;
    for (;;) {
        if (pos >= n) return XZ_CORRUPT;
        const uint32_t ctl = p[pos];
        if (ctl == 0) { pos++; break; }
        if (ctl < 0x80) {
            if (ctl > 2 || n - pos < 3) return XZ_CORRUPT;
            const uint64_t sz = (((uint32_t)p[pos + 1] << 8) | p[pos + 2]) + 1u;
            if (n - pos - 3 < sz) return XZ_CORRUPT;
            pos += 3 + sz; out += sz;
        } else {
            const uint32_t hdr = ctl >= 0xC0 ? 6u : 5u;
            if (n - pos < hdr) return XZ_CORRUPT;
            const uint64_t u = ((uint64_t)(ctl & 31) << 16) + (((uint32_t)p[pos + 1] << 8) | p[pos + 2]) + 1u;
            const uint64_t cs = (((uint32_t)p[pos + 3] << 8) | p[pos + 4]) + 1u;
            if (ctl >= 0xC0) {
                uint32_t pr = p[pos + 5];
                if (pr > 224) return XZ_CORRUPT;
                const uint32_t lc = pr % 9; pr /= 9;
                const uint32_t lp = pr % 5;
                if (lc + lp > 4) return XZ_CORRUPT;
                if (lc + lp > *lclp) *lclp = lc + lp;
            }
            if (n - pos - hdr < cs) return XZ_CORRUPT;
            pos += hdr + cs; out += u;
        }
        if (out > dec_len) return XZ_CORRUPT;
    }
    return pos == n && out == dec_len ? XZ_OK : XZ_CORRUPT;
}

// One .xz stream of n bytes at p: header, footer, Index, every block header, the chunk headers.  blocks == null: count (o->nblk, o->total, o->lclp);
// otherwise the block descriptors as well, o->nblk of them and never more than blk_cap (the caller has made room by a first call): offsets src_abs + ...,
// dst_abs + ....
XZ_HD void xz_scan(const uint8_t *p, uint64_t n, uint64_t src_abs, uint64_t dst_abs, uint32_t stream, XzScan *o, XzBlock *blocks, uint32_t blk_cap) {
    o->status = XZ_CORRUPT; o->nblk = 0; o->check = 0; o->lclp = 0; o->total = 0; o->why = 0; o->pad = 0;
    if (n < 32 || (n & 3)) return;
    // stream header: magic, flags, CRC32 of the flags
    if (p[0] != 0xFD || p[1] != '7' || p[2] != 'z' || p[3] != 'X' || p[4] != 'Z' || p[5] != 0) return;
    if (xz_crc32(p + 6, 2) != xz_le32(p + 8)) return;
    // stream footer: CRC32 of backward size + flags, flags as in the header, magic
    const uint8_t *f = p + n - 12;
    if (f[10] != 'Y' || f[11] != 'Z') return;
    if (xz_crc32(f + 4, 6) != xz_le32(f)) return;
    if (f[8] != p[6] || f[9] != p[7]) return;
    if (p[6] != 0 || (p[7] & 0xF0)) { o->status = XZ_UNSUPPORTED; o->why = XZ_UNSUP_HEADER; return; }
    const uint32_t check = p[7];
    o->check = check;
    const uint64_t isize = ((uint64_t)xz_le32(f + 4) + 1) * 4;
    if (isize > n - 24) return;
    const uint64_t ioff = n - 12 - isize, iend = n - 12;
    // the Index: indicator, record count, records, padding, CRC32 -- exactly `backward size` bytes
    if (p[ioff] != 0) return;
    if (xz_crc32(p + ioff, isize - 4) != xz_le32(p + iend - 4)) return;
    uint64_t ip = ioff + 1, nrec = 0;
    if (!xz_vli(p, ip, iend - 4, nrec)) return;
    if (nrec > isize / 2 || nrec > 0x7FFFFFFFull) return;                // (a record takes two bytes at least)
    if (check != XZ_CHECK_NONE && check != XZ_CHECK_CRC32 && check != XZ_CHECK_CRC64) {
        o->status = XZ_UNSUPPORTED; o->why = check == XZ_CHECK_SHA256 ? XZ_UNSUP_SHA256 : XZ_UNSUP_CHECK; return;
    }
    const uint32_t csz = xz_check_size(check);
    uint64_t cur = 12, total = 0;
    uint32_t lclp = 0, unsup = 0;
    for (uint64_t r = 0; r < nrec; r++) {
        uint64_t unpadded = 0, usize = 0;
        if (!xz_vli(p, ip, iend - 4, unpadded) || !xz_vli(p, ip, iend - 4, usize)) return;
        if (unpadded < 5 || unpadded > (1ull << 62) || usize > (1ull << 62)) return;
        const uint64_t padded = (unpadded + 3) & ~3ull;
        if (padded > ioff - cur) return;
        // the block header: size, flags, optional sizes, the filter, padding, CRC32
        const uint8_t *b = p + cur;
        if (b[0] == 0) return;
        const uint64_t hs = ((uint64_t)b[0] + 1) * 4;
        if (hs + csz + 1 > unpadded) return;
        if (xz_crc32(b, hs - 4) != xz_le32(b + hs - 4)) return;
        const uint64_t comp = unpadded - hs - csz;
        for (uint64_t q = cur + hs + comp; q < cur + padded - csz; q++) if (p[q] != 0) return;     // block padding
        if (b[1] & 0x3C) { unsup = XZ_UNSUP_HEADER; }
        else if ((b[1] & 3) != 0) { unsup = XZ_UNSUP_FILTER; }           // a chain of more than one filter (Delta, BCJ in front of LZMA2)
        uint32_t dict = 0;
        if (!unsup) {
            uint64_t hp = 2, v = 0;
            if (b[1] & 0x40) { if (!xz_vli(b, hp, hs - 4, v) || v != comp) return; }
            if (b[1] & 0x80) { if (!xz_vli(b, hp, hs - 4, v) || v != usize) return; }
            uint64_t id = 0, psz = 0;
            if (!xz_vli(b, hp, hs - 4, id) || !xz_vli(b, hp, hs - 4, psz)) return;
            if (id != 0x21) unsup = XZ_UNSUP_FILTER;
            else {
                if (psz != 1 || hp >= hs - 4) return;
                if (b[hp] > 40) unsup = XZ_UNSUP_HEADER;
                else dict = xz_dict_size(b[hp]);
                hp++;
                for (; hp < hs - 4; hp++) if (b[hp] != 0) unsup = XZ_UNSUP_HEADER;
            }
        }
        if (!unsup && usize > 0xFFFFFFFFull) unsup = XZ_UNSUP_BIG_BLOCK;
        if (!unsup) {
            if (xz_chunk_walk(b + hs, comp, usize, &lclp) != XZ_OK) return;
            if (blocks && r < blk_cap) {
                XzBlock &d = blocks[r];
                d.src = src_abs + cur + hs; d.src_len = comp; d.dst = dst_abs + total; d.check_off = src_abs + cur + padded - csz;
                d.dst_len = (uint32_t)usize; d.dict = dict; d.check = check; d.stream = stream; d.status = XZ_OK; d.pad = 0;
            }
        }
        total += usize; cur += padded;
        if (total > (1ull << 62)) return;
    }
    if (cur != ioff) return;                                              // blocks the Index does not list, or bytes between them and the Index
    while ((ip - ioff) & 3) { if (p[ip] != 0) return; ip++; }
    if (ip != iend - 4) return;
    if (unsup) { o->status = XZ_UNSUPPORTED; o->why = unsup; return; }
    o->status = XZ_OK; o->nblk = (uint32_t)nrec; o->lclp = lclp; o->total = total;
}

// ---- the block decoder
struct XzIn {                           // the block's compressed bytes [0, end); lim: the end of the chunk being read; bad: a read went past it
    const uint8_t *p; uint64_t pos, end, lim; uint32_t bad;
#if XZ_DEV
    uint64_t base; uint32_t w;          // a window of 256 bytes from `base` on, four per lane
#endif
};
XZ_HD uint32_t xz_in_byte(XzIn &in, uint32_t lane) {
    if (in.pos >= in.lim) { in.bad = 1; return 0; }
#if XZ_DEV
    uint64_t d = in.pos - in.base;
    if (d >= 256) {
        in.base = in.pos; d = 0;
        const uint64_t a = in.base + lane * 4;
        uint32_t w = 0;
        for (uint32_t k = 0; k < 4; k++) if (a + k < in.end) w |= (uint32_t)in.p[a + k] << (8 * k);
        in.w = w;
    }
    in.pos++;
    return (XZ_LANE_OF(in.w, (uint32_t)d >> 2) >> (((uint32_t)d & 3) * 8)) & 255u;
#else
    (void)lane;
    return in.p[in.pos++];
#endif
}
struct XzRc { uint32_t range, code; };
XZ_HD void xz_put_prob(uint16_t *pr, uint32_t v, uint32_t lane) { if (lane == 0) *pr = (uint16_t)v; }
XZ_HD uint32_t xz_bit(XzRc &rc, XzIn &in, uint16_t *pr, uint32_t lane) {
    if (rc.range < (1u << 24)) { rc.range <<= 8; rc.code = (rc.code << 8) | xz_in_byte(in, lane); }
    const uint32_t p = XZ_U(*pr);
    const uint32_t bound = (rc.range >> 11) * p;
    if (rc.code < bound) { rc.range = bound; xz_put_prob(pr, p + ((2048u - p) >> 5), lane); return 0; }
    rc.range -= bound; rc.code -= bound; xz_put_prob(pr, p - (p >> 5), lane);
    return 1;
}
XZ_HD uint32_t xz_tree(XzRc &rc, XzIn &in, uint16_t *pr, uint32_t nbits, uint32_t lane) {
    uint32_t m = 1;
    for (uint32_t i = 0; i < nbits; i++) m = (m << 1) | xz_bit(rc, in, pr + m, lane);
    return m - (1u << nbits);
}
XZ_HD uint32_t xz_tree_rev(XzRc &rc, XzIn &in, uint16_t *pr, uint32_t nbits, uint32_t lane) {
    uint32_t m = 1, r = 0;
    for (uint32_t i = 0; i < nbits; i++) { const uint32_t b = xz_bit(rc, in, pr + m, lane); m = (m << 1) | b; r |= b << i; }
    return r;
}
XZ_HD uint32_t xz_direct(XzRc &rc, XzIn &in, uint32_t nbits, uint32_t lane) {
    uint32_t r = 0;
    for (uint32_t i = 0; i < nbits; i++) {
        if (rc.range < (1u << 24)) { rc.range <<= 8; rc.code = (rc.code << 8) | xz_in_byte(in, lane); }
        rc.range >>= 1;
        rc.code -= rc.range;
        const uint32_t t = 0u - (rc.code >> 31);
        rc.code += rc.range & t;
        r = (r << 1) + (t + 1);
    }
    return r;
}
XZ_HD uint32_t xz_len(XzRc &rc, XzIn &in, uint16_t *L, uint32_t pos_state, uint32_t lane) {
    if (!xz_bit(rc, in, L, lane)) return 2 + xz_tree(rc, in, L + XZP_LEN_LOW + pos_state * 8, 3, lane);
    if (!xz_bit(rc, in, L + 1, lane)) return 10 + xz_tree(rc, in, L + XZP_LEN_MID + pos_state * 8, 3, lane);
    return 18 + xz_tree(rc, in, L + XZP_LEN_HIGH, 8, lane);
}

// One block: src[0, src_len) -> dst[0, dst_len).  probs: room for xz_prob_count(lclp_cap) entries (LDS on the device).  lane: 0 .. XZ_LANES - 1; every
// lane gets the same status.
XZ_HD uint32_t xz_lzma2_block(const uint8_t *src, uint64_t src_len, uint8_t *dst, uint32_t dst_len, uint32_t dict_size, uint16_t *probs, uint32_t lclp_cap,
                              uint32_t lane) {
    XzIn in; in.p = src; in.pos = 0; in.end = src_len; in.lim = src_len; in.bad = 0;
#if XZ_DEV
    in.base = ~0ull - 1024; in.w = 0;                                   // (no window yet: the first read fills it)
#endif
    XzRc rc; rc.range = 0; rc.code = 0;
    uint32_t pos = 0, dict_start = 0, need_dict = 1, need_props = 1;
    uint32_t state = 0, rep0 = 0, rep1 = 0, rep2 = 0, rep3 = 0, lc = 0, lp = 0, pb = 0, prev = 0;
    for (;;) {
        in.lim = in.end;
        const uint32_t ctl = xz_in_byte(in, lane);
        if (in.bad) return XZ_CORRUPT;
        if (ctl == 0) break;
        if (ctl >= 0xE0 || ctl == 1) { need_props = 1; need_dict = 0; dict_start = pos; }
        else if (need_dict) return XZ_CORRUPT;
        if (ctl < 0x80) {                                               // ---- an uncompressed chunk: all lanes copy
            if (ctl > 2) return XZ_CORRUPT;
            uint32_t n = xz_in_byte(in, lane) << 8; n |= xz_in_byte(in, lane); n += 1;
            if (in.bad || n > in.end - in.pos || n > dst_len - pos) return XZ_CORRUPT;
            const uint8_t *s = src + in.pos;
            for (uint32_t i = lane; i < n; i += XZ_LANES) dst[pos + i] = s[i];
            prev = XZ_U(s[n - 1]);
            pos += n; in.pos += n;
            XZ_SYNC();
            continue;
        }
        // ---- an LZMA chunk
        uint32_t usize = (ctl & 31u) << 16; usize |= xz_in_byte(in, lane) << 8; usize |= xz_in_byte(in, lane); usize += 1;
        uint32_t csize = xz_in_byte(in, lane) << 8; csize |= xz_in_byte(in, lane); csize += 1;
        bool reset = false;
        if (ctl >= 0xC0) {
            uint32_t pr = xz_in_byte(in, lane);
            if (in.bad || pr > 224) return XZ_CORRUPT;
            lc = pr % 9; pr /= 9; lp = pr % 5; pb = pr / 5;
            if (lc + lp > 4 || lc + lp > lclp_cap) return XZ_CORRUPT;
            need_props = 0; reset = true;
        } else if (need_props) return XZ_CORRUPT;
        else if (ctl >= 0xA0) reset = true;
        if (in.bad || usize > dst_len - pos || csize > in.end - in.pos) return XZ_CORRUPT;
        if (reset) {
            const uint32_t np = xz_prob_count(lc + lp);
            XZ_SYNC();
            for (uint32_t i = lane; i < np; i += XZ_LANES) probs[i] = 1024;
            XZ_SYNC();
            state = 0; rep0 = rep1 = rep2 = rep3 = 0;
        }
        in.lim = in.pos + csize;
        if (xz_in_byte(in, lane) != 0) return XZ_CORRUPT;               // the range coder's first byte
        rc.range = 0xFFFFFFFFu; rc.code = 0;
        for (int k = 0; k < 4; k++) rc.code = (rc.code << 8) | xz_in_byte(in, lane);
        const uint32_t chunk_end = pos + usize, pb_mask = (1u << pb) - 1, lp_mask = (1u << lp) - 1;
        while (pos < chunk_end) {                                       // every turn writes at least one byte or ends the block
            if (in.bad) return XZ_CORRUPT;
            const uint32_t since = pos - dict_start, pos_state = since & pb_mask;
            if (!xz_bit(rc, in, probs + XZP_IS_MATCH + state * 16 + pos_state, lane)) {      // ---- a literal
                const uint32_t pv = since ? prev : 0u;
                uint16_t *lit = probs + XZP_LIT + 0x300u * (((since & lp_mask) << lc) + (pv >> (8 - lc)));
                uint32_t sym = 1;
                if (state >= 7) {
                    uint32_t mb = XZ_U(dst[pos - rep0 - 1]);
                    do {
                        const uint32_t mbit = (mb >> 7) & 1u; mb <<= 1;
                        const uint32_t bit = xz_bit(rc, in, lit + ((1 + mbit) << 8) + sym, lane);
                        sym = (sym << 1) | bit;
                        if (mbit != bit) break;
                    } while (sym < 0x100);
                }
                while (sym < 0x100) sym = (sym << 1) | xz_bit(rc, in, lit + sym, lane);
                prev = sym & 255u;
                if (lane == 0) dst[pos] = (uint8_t)prev;
                pos++;
                state = state < 4 ? 0 : (state < 10 ? state - 3 : state - 6);
                continue;
            }
            uint32_t len;
            if (!xz_bit(rc, in, probs + XZP_IS_REP + state, lane)) {                         // ---- a match with a new distance
                rep3 = rep2; rep2 = rep1; rep1 = rep0;
                len = xz_len(rc, in, probs + XZP_MATCH_LEN, pos_state, lane);
                state = state < 7 ? 7 : 10;
                const uint32_t slot = xz_tree(rc, in, probs + XZP_POS_SLOT + (len < 6 ? len - 2 : 3) * 64, 6, lane);
                if (slot < 4) rep0 = slot;
                else {
                    const uint32_t nb = (slot >> 1) - 1;
                    rep0 = (2u | (slot & 1u)) << nb;
                    if (slot < 14) rep0 += xz_tree_rev(rc, in, probs + XZP_POS_SPECIAL + rep0 - slot, nb, lane);
                    else { rep0 += xz_direct(rc, in, nb - 4, lane) << 4; rep0 += xz_tree_rev(rc, in, probs + XZP_POS_ALIGN, 4, lane); }
                }
            } else {
                if (!xz_bit(rc, in, probs + XZP_IS_REP0 + state, lane)) {
                    if (!xz_bit(rc, in, probs + XZP_IS_REP0_LONG + state * 16 + pos_state, lane)) {     // ---- a short repeat: one byte
                        if (rep0 >= since || rep0 >= dict_size) return XZ_CORRUPT;
                        XZ_SYNC();
                        prev = XZ_U(dst[pos - rep0 - 1]);
                        if (lane == 0) dst[pos] = (uint8_t)prev;
                        pos++;
                        state = state < 7 ? 9 : 11;
                        continue;
                    }
                } else {
                    uint32_t d;
                    if (!xz_bit(rc, in, probs + XZP_IS_REP1 + state, lane)) d = rep1;
                    else {
                        if (!xz_bit(rc, in, probs + XZP_IS_REP2 + state, lane)) d = rep2;
                        else { d = rep3; rep3 = rep2; }
                        rep2 = rep1;
                    }
                    rep1 = rep0; rep0 = d;
                }
                len = xz_len(rc, in, probs + XZP_REP_LEN, pos_state, lane);
                state = state < 7 ? 8 : 11;
            }
            // ---- the copy: len bytes from rep0 + 1 back, by all lanes; a distance shorter than the length repeats its bytes
            if (rep0 >= since || rep0 >= dict_size || len > chunk_end - pos) return XZ_CORRUPT;     // (the end marker, distance 2^32 - 1, falls here too)
            XZ_SYNC();
            {
                const uint32_t D = rep0 + 1;
                const uint8_t *from = dst + (pos - D);
                uint32_t last = 0;
                for (uint32_t i = lane; i < len; i += XZ_LANES) { last = from[D >= len ? i : i % D]; dst[pos + i] = (uint8_t)last; }
                prev = XZ_LANE_OF(last, (len - 1) & (XZ_LANES - 1));
            }
            pos += len;
            XZ_SYNC();
        }
        if (rc.range < (1u << 24)) { rc.range <<= 8; rc.code = (rc.code << 8) | xz_in_byte(in, lane); }
        if (in.bad || rc.code != 0 || in.pos != in.lim) return XZ_CORRUPT;                       // the chunk's compressed bytes: all of them, no more
    }
    return pos == dst_len && in.pos == in.end ? XZ_OK : XZ_CORRUPT;
}
