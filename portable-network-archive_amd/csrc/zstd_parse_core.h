// zstd_parse_core.h -- the zstd decoder's parse layer (RFC 8878), once: bit readers, FSE table builders, and one parser per header -- frame,
// skippable frame, block, literals section, Huffman tree description, sequences section, one LL / OF / ML table, the Huffman streams' jump table.
// __host__ __device__ inline code: k_zdec.hip runs it in every kernel that reads a header (k_zdec, k_zparse, k_zparse_a, k_zhuf, k_zscan, k_zcount,
// k_zlist, k_zsize); tests/zstd_parse_core builds it with g++ alone into a single-lane decoder (tests/test_zstd_parse_core.py: against two CPU
// decoders, and as a stand-alone program under ASan + UBSan).
//
// Facts and policy: a parser reports what the bytes say -- every field, the header's length, which bytes were missing -- and never a status.  Which
// fact is an error, and which status it gets, is the caller's: the routes differ there (zscan_frame_end tolerates a dictionary id, k_zsize wants the
// window, k_zparse_a only sizes and modes).  The decoding tables are passed in by pointer (LDS on the device): the parsers are force-inlined so that
// the compiler sees the address space.
// Safety: a parser reads p[0 .. len) only, whatever the bytes say.  The one exception is zd_bits on the device (see there).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define ZD_HD __host__ __device__ __forceinline__
#define ZD_FN __host__ __device__ inline
#define ZD_TABLE __constant__
#else
#define ZD_HD static inline __attribute__((always_inline))
#define ZD_FN static inline
#define ZD_TABLE static const
#endif

enum { ZD_OK = 0, ZD_CORRUPT = 1, ZD_UNSUPPORTED = 2, ZD_DSTSIZE = 3, ZD_VOID = 4 };     // ZFrame::status (ZD_VOID: a frame slot that holds nothing)
constexpr int ZD_HUF_MAX = 11;
constexpr uint32_t ZD_MAGIC = 0xFD2FB528u, ZD_SKIP_MAGIC = 0x184D2A50u, ZD_BLOCK_MAX = 128u << 10;

typedef unsigned long long zd_u64u __attribute__((aligned(1)));

ZD_TABLE int16_t ZD_LL_DEF[36] = {4,3,2,2,2,2,2,2,2,2,2,2,2,1,1,1,2,2,2,2,2,2,2,2,2,3,2,1,1,1,1,1,-1,-1,-1,-1};
ZD_TABLE int16_t ZD_ML_DEF[53] = {1,4,3,2,2,2,2,2,2,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,-1,-1,-1,-1,-1,-1,-1};
ZD_TABLE int16_t ZD_OF_DEF[29] = {1,1,1,1,1,1,2,2,2,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,-1,-1,-1,-1,-1};
ZD_TABLE uint32_t ZD_LL_BASE[36] = {0,1,2,3,4,5,6,7,8,9,10,11,12,13,14,15,16,18,20,22,24,28,32,40,48,64,128,256,512,1024,2048,4096,8192,16384,32768,65536};
ZD_TABLE uint8_t  ZD_LL_BITS[36] = {0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,1,1,1,1,2,2,3,3,4,6,7,8,9,10,11,12,13,14,15,16};
ZD_TABLE uint32_t ZD_ML_BASE[53] = {3,4,5,6,7,8,9,10,11,12,13,14,15,16,17,18,19,20,21,22,23,24,25,26,27,28,29,30,31,32,33,34,35,37,39,41,43,47,51,59,67,83,99,131,259,515,1027,2051,4099,8195,16387,32771,65539};
ZD_TABLE uint8_t  ZD_ML_BITS[53] = {0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,1,1,1,1,2,2,3,3,4,4,5,7,8,9,10,11,12,13,14,15,16};

ZD_HD int zd_hb(uint32_t v) { return 31 - (int)__builtin_clz(v); }           // v != 0
ZD_HD uint64_t zd_le(const uint8_t *p, uint32_t n) { uint64_t v = 0; for (uint32_t i = 0; i < n; i++) v |= (uint64_t)p[i] << (8 * i); return v; }   // n <= 8

// ---- bit readers
// n bits (<= 56) at bit offset off >= 0 of the little-endian bit string p[0 .. len).  The device reads 8 bytes at p + off / 8 (the source buffer carries
// 8 bytes of slack behind its last stream); the host build reads byte by byte, bytes behind the string as zero.
ZD_HD uint64_t zd_bits(const uint8_t *p, uint32_t len, int64_t off, uint32_t n) {
#if defined(__HIP_DEVICE_COMPILE__)
    (void)len;
    const uint64_t v = *(const zd_u64u *)(p + (off >> 3)) >> (off & 7);
#else
    const uint64_t at = (uint64_t)(off >> 3);
    const uint64_t v = zd_le(p + (at < len ? at : len), (uint32_t)(at < len ? (len - at < 8 ? len - at : 8) : 0)) >> (off & 7);
#endif
    return v & (((uint64_t)1 << n) - 1);
}
// backward reader: `off` = number of unread bits below the cursor; bits below the start of the string read as zero
struct ZdBits { const uint8_t *p; uint32_t len; int64_t off; };
ZD_HD bool zd_binit(ZdBits &b, const uint8_t *p, uint32_t len) {
    if (len == 0) return false;
    const uint32_t last = p[len - 1];
    if (last == 0) return false;
    b.p = p; b.len = len; b.off = (int64_t)len * 8 - (8 - zd_hb(last));
    return true;
}
ZD_HD uint64_t zd_bread(ZdBits &b, uint32_t n) {
    if (n == 0) return 0;
    b.off -= n;
    if (b.off >= 0) return zd_bits(b.p, b.len, b.off, n);
    const int64_t have = (int64_t)n + b.off;                       // bits that exist
    if (have <= 0) return 0;
    return zd_bits(b.p, b.len, 0, (uint32_t)have) << (uint32_t)(-b.off);
}

// The same reader with a 128-bit window in registers (words k, k+1 of the string, 8 bytes each) and word k-1 already requested.
// `fetch(j)` returns word j of the string: from the LDS copy of the stream when it fits (the serial Huffman / FSE chains then
// never wait for HBM), else straight from global memory; a bounded copy loop on the host.
struct ZdWin { int64_t off; int64_t k; uint64_t lo, hi, pre; };
template <class F> ZD_HD bool zd_winit(ZdWin &w, F &&fetch, uint32_t last_byte, uint32_t len) {
    if (len == 0 || last_byte == 0) return false;
    w.off = (int64_t)len * 8 - (8 - zd_hb(last_byte));
    w.k = ((w.off + 63) >> 6) - 2; if (w.k < 0) w.k = 0;
    w.lo = fetch(w.k); w.hi = fetch(w.k + 1); w.pre = w.k > 0 ? fetch(w.k - 1) : 0;
    return true;
}
// the n (<= 57) bits below the cursor, not consumed
template <class F> ZD_HD uint64_t zd_wpeek(ZdWin &w, F &&fetch, uint32_t n) {
    const int64_t lo_bit = w.off - (int64_t)n;
    const int64_t need = lo_bit < 0 ? 0 : lo_bit;
    while (need < 64 * w.k) { w.hi = w.lo; w.lo = w.pre; w.k--; w.pre = w.k > 0 ? fetch(w.k - 1) : 0; }
    const uint32_t sft = (uint32_t)(need - 64 * w.k);              // 0..127
    uint64_t v = sft < 64 ? (w.lo >> sft) | (sft ? w.hi << (64 - sft) : 0) : w.hi >> (sft - 64);
    if (lo_bit < 0) {                                              // part of the field lies below the start: zero there
        if (w.off <= 0) return 0;
        v = (v & (((uint64_t)1 << (uint32_t)w.off) - 1)) << (uint32_t)(-lo_bit);
    }
    return v & (((uint64_t)1 << n) - 1);
}
template <class F> ZD_HD uint64_t zd_wread(ZdWin &w, F &&fetch, uint32_t n) {
    if (n == 0) return 0;
    const uint64_t v = zd_wpeek(w, fetch, n);
    w.off -= n;
    return v;
}

// ---- FSE
// decoding table (sym | nbits << 8 | base << 16) from a normalised distribution; serial (one thread)
ZD_FN bool zd_fse_build(uint32_t *tab, const int16_t *norm, int nsym, int alog, uint16_t *next /* [256] scratch */) {
    if (alog > 9) return false;
    const int size = 1 << alog;
    int high = size - 1;
    for (int s = 0; s < nsym; s++) {
        if (norm[s] == -1) { tab[high--] = (uint32_t)s; next[s] = 1; }
        else next[s] = (uint16_t)norm[s];
    }
    const int step = (size >> 1) + (size >> 3) + 3, mask = size - 1;
    int pos = 0;
    for (int s = 0; s < nsym; s++)
        for (int i = 0; i < norm[s]; i++) { tab[pos] = (uint32_t)s; do { pos = (pos + step) & mask; } while (pos > high); }
    if (pos != 0) return false;
    for (int u = 0; u < size; u++) {
        const uint32_t s = tab[u] & 0xFF;
        const uint32_t ns = next[s]++;
        const uint32_t nb = (uint32_t)(alog - zd_hb(ns));
        tab[u] = s | (nb << 8) | ((((ns << nb) - (uint32_t)size) & 0xFFFF) << 16);
    }
    return true;
}

// table description (forward bits); returns bytes consumed, 0 on error
ZD_FN uint32_t zd_fse_desc(const uint8_t *src, uint32_t len, int16_t *norm, int *nsym_out, int *alog_out, int max_sym, int max_alog) {
    if (len < 1) return 0;
    uint64_t bitpos = 0;
    auto peek = [&](uint32_t n) -> uint32_t {
        uint64_t v = 0; const uint64_t byte = bitpos >> 3;
        for (int i = 0; i < 5; i++) if (byte + i < len) v |= (uint64_t)src[byte + i] << (8 * i);
        return (uint32_t)((v >> (bitpos & 7)) & (((uint64_t)1 << n) - 1));
    };
    const int alog = (int)peek(4) + 5; bitpos += 4;
    if (alog > max_alog) return 0;
    int remaining = (1 << alog) + 1, threshold = 1 << alog, nbits = alog + 1, sym = 0;
    for (int i = 0; i <= max_sym; i++) norm[i] = 0;
    while (remaining > 1 && sym <= max_sym) {
        const int mx = (2 * threshold - 1) - remaining;
        int count;
        const uint32_t v = peek((uint32_t)nbits);
        if ((int)(v & (uint32_t)(threshold - 1)) < mx) { count = (int)(v & (uint32_t)(threshold - 1)); bitpos += (uint32_t)(nbits - 1); }
        else { count = (int)(v & (uint32_t)(2 * threshold - 1)); if (count >= threshold) count -= mx; bitpos += (uint32_t)nbits; }
        count--;
        remaining -= count < 0 ? -count : count;
        norm[sym++] = (int16_t)count;
        if (count == 0) {
            for (;;) {
                const uint32_t rep = peek(2); bitpos += 2;
                for (uint32_t i = 0; i < rep && sym <= max_sym; i++) norm[sym++] = 0;
                if (rep != 3) break;
            }
        }
        while (remaining < threshold) { nbits--; threshold >>= 1; }
        if ((bitpos + 7) / 8 > len) return 0;
    }
    if (remaining != 1 || sym > max_sym + 1) return 0;
    *nsym_out = sym; *alog_out = alog;
    return (uint32_t)((bitpos + 7) / 8);
}

// ---- frame header (RFC 8878 3.1.1.1) at p[0 .. len)
struct ZdFrameHdr {
    bool have;                              // magic and descriptor (5 bytes) are there; nothing below is set without them
    bool magic, reserved, single, checksum; // the magic is zstd's; Reserved_bit; Single_Segment_flag; Content_Checksum_flag
    bool complete;                          // all `len` bytes are there; fcs and window are set only then
    uint32_t dict_bytes, fcs_bytes, len;    // sizes of Dictionary_ID and Frame_Content_Size; the whole header
    uint64_t fcs, window;                   // Frame_Content_Size (fcs_bytes != 0); Window_Size (the content size of a single-segment frame)
};
ZD_HD uint64_t zd_fcs(const uint8_t *p, uint32_t n) { return zd_le(p, n) + (n == 2 ? 256u : 0u); }
ZD_HD void zd_frame_header(const uint8_t *p, uint64_t len, ZdFrameHdr &h) {
    h = ZdFrameHdr();
    h.have = len >= 5;
    if (!h.have) return;
    h.magic = (uint32_t)zd_le(p, 4) == ZD_MAGIC;
    const uint32_t fhd = p[4], fcs_flag = fhd >> 6, dict = fhd & 3;
    h.single = (fhd >> 5) & 1; h.checksum = (fhd >> 2) & 1; h.reserved = (fhd >> 3) & 1;
    h.dict_bytes = dict == 3 ? 4u : dict;
    h.fcs_bytes = fcs_flag == 0 ? (uint32_t)h.single : 1u << fcs_flag;
    h.len = 5 + (h.single ? 0u : 1u) + h.dict_bytes + h.fcs_bytes;
    h.complete = h.len <= len;
    if (!h.complete) return;
    h.fcs = zd_fcs(p + h.len - h.fcs_bytes, h.fcs_bytes);
    if (h.single) h.window = h.fcs;
    else { const uint32_t wd = p[5]; const uint64_t wbase = 1ull << (10 + (wd >> 3)); h.window = wbase + (wbase >> 3) * (wd & 7); }
}

// ---- skippable frame (3.1.2) at p[0 .. len): 0 the bytes are no skippable frame (or fewer than 4), 1 a whole one of *total bytes, 2 one cut short
enum { ZD_SKIP_NONE = 0, ZD_SKIP_WHOLE = 1, ZD_SKIP_CUT = 2 };
ZD_HD int zd_skippable(const uint8_t *p, uint64_t len, uint64_t *total) {
    if (len < 4 || ((uint32_t)zd_le(p, 4) & 0xFFFFFFF0u) != ZD_SKIP_MAGIC) return ZD_SKIP_NONE;
    if (len < 8) return ZD_SKIP_CUT;
    *total = 8 + zd_le(p + 4, 4);
    return *total > len ? ZD_SKIP_CUT : ZD_SKIP_WHOLE;
}

// ---- block header (3.1.1.2) at p[0 .. len)
struct ZdBlockHdr {
    bool have, fits;                        // the 3 bytes are there; so is the body
    uint32_t last, type, size, body;        // Last_Block, Block_Type, Block_Size; bytes behind the header (1 for an RLE block)
};
ZD_HD void zd_block_header(const uint8_t *p, uint64_t len, ZdBlockHdr &b) {
    b = ZdBlockHdr();
    b.have = len >= 3;
    if (!b.have) return;
    const uint32_t bh = (uint32_t)zd_le(p, 3);
    b.last = bh & 1; b.type = (bh >> 1) & 3; b.size = bh >> 3;
    b.body = b.type == 1 ? 1u : b.size;
    b.fits = (uint64_t)3 + b.body <= len;
}

// ---- literals section header (3.1.1.3.1.1) at p[0 .. len); false: its bytes are not all there
struct ZdLitHdr {
    uint32_t ltype, sf, regen, comp, hdr, streams;   // type, Size_Format, Regenerated_Size, Compressed_Size (types 2, 3), header bytes, 1 or 4 streams
    uint32_t size;                                   // header + payload: where the sequences section starts
};
ZD_HD bool zd_literals_header(const uint8_t *p, uint32_t len, ZdLitHdr &l) {
    l = ZdLitHdr();
    if (len < 1) return false;
    l.ltype = p[0] & 3; l.sf = (p[0] >> 2) & 3; l.streams = 1;
    if (l.ltype < 2) {
        l.hdr = l.sf == 1 ? 2u : (l.sf == 3 ? 3u : 1u);
        if (len < l.hdr) return false;
        l.regen = l.hdr == 1 ? p[0] >> 3 : (uint32_t)(zd_le(p, l.hdr) >> 4);
        l.size = l.hdr + (l.ltype == 0 ? l.regen : 1u);
    } else {
        if (len < 5) return false;
        const uint64_t v = zd_le(p, 5);
        const uint32_t w = l.sf < 2 ? 10u : (l.sf == 2 ? 14u : 18u);          // bits of either size
        l.streams = l.sf == 0 ? 1u : 4u; l.hdr = l.sf < 2 ? 3u : l.sf + 2;
        l.regen = (uint32_t)(v >> 4) & ((1u << w) - 1); l.comp = (uint32_t)(v >> (4 + w)) & ((1u << w) - 1);
        l.size = l.hdr + l.comp;
    }
    return true;
}

// ---- Huffman tree description (4.2.1) at cs[0 .. cl) -> weights[0 .. n) (direct or FSE-coded, the last one implied), the code's depth, bytes used;
// norm[256], nexts[256], wtab[64]: scratch for the weights' FSE table
ZD_HD bool zd_huf_weights(const uint8_t *cs, uint32_t cl, uint8_t *weights, int16_t *norm, uint16_t *nexts, uint32_t *wtab, uint32_t &n, uint32_t &maxbits, uint32_t &used) {
    if (cl < 1) return false;
    const uint32_t hbyte = cs[0];
    uint32_t nw = 0;
    if (hbyte >= 128) {
        nw = hbyte - 127;
        const uint32_t bytes = (nw + 1) / 2;
        if (1 + bytes > cl) return false;
        for (uint32_t i = 0; i < nw; i++) { const uint32_t by = cs[1 + i / 2]; weights[i] = (uint8_t)((i & 1) ? (by & 15) : (by >> 4)); }
        used = 1 + bytes;
    } else {
        const uint32_t csize = hbyte;
        if (csize == 0 || 1 + csize > cl) return false;
        int nsym, alog;
        const uint32_t dl = zd_fse_desc(cs + 1, csize, norm, &nsym, &alog, 255, 6);
        if (!dl || dl >= csize || !zd_fse_build(wtab, norm, nsym, alog, nexts)) return false;
        ZdBits bb;
        if (!zd_binit(bb, cs + 1 + dl, csize - dl)) return false;
        uint32_t s1 = (uint32_t)zd_bread(bb, (uint32_t)alog), s2 = (uint32_t)zd_bread(bb, (uint32_t)alog);
        for (;;) {                                                  // two interleaved states; the stream ends when a state update runs out of bits
            if (nw >= 255) return false;
            weights[nw++] = (uint8_t)(wtab[s1] & 0xFF);
            s1 = (wtab[s1] >> 16) + (uint32_t)zd_bread(bb, (wtab[s1] >> 8) & 0xFF);
            if (bb.off < 0) { if (nw >= 255) return false; weights[nw++] = (uint8_t)(wtab[s2] & 0xFF); break; }
            if (nw >= 255) return false;
            weights[nw++] = (uint8_t)(wtab[s2] & 0xFF);
            s2 = (wtab[s2] >> 16) + (uint32_t)zd_bread(bb, (wtab[s2] >> 8) & 0xFF);
            if (bb.off < 0) { if (nw >= 255) return false; weights[nw++] = (uint8_t)(wtab[s1] & 0xFF); break; }
        }
        used = 1 + csize;
    }
    uint32_t total = 0; bool badw = false;
    for (uint32_t i = 0; i < nw; i++) { if (weights[i] > ZD_HUF_MAX) badw = true; else if (weights[i]) total += 1u << (weights[i] - 1); }
    if (badw || total == 0 || nw < 1) return false;
    maxbits = (uint32_t)zd_hb(total) + 1;
    const uint32_t rest = (1u << maxbits) - total;
    if (maxbits > (uint32_t)ZD_HUF_MAX || rest == 0 || (rest & (rest - 1))) return false;
    weights[nw] = (uint8_t)(zd_hb(rest) + 1);
    n = nw + 1;
    return true;
}

// weights -> decoding table (sym | nbits << 8), by nthreads threads (this one: tid): symbol s of weight w owns 2^(w-1) cells behind all symbols of
// smaller weight and the lower-numbered symbols of its own weight
ZD_HD void zd_huf_fill(uint16_t *tab, const uint8_t *weights, uint32_t n, uint32_t maxbits, uint32_t tid, uint32_t nthreads) {
    for (uint32_t s = tid; s < n; s += nthreads) {
        const uint32_t w = weights[s];
        if (!w) continue;
        uint32_t pos = 0;
        for (uint32_t o = 0; o < n; o++) { const uint32_t wo = weights[o]; if (wo && (wo < w || (wo == w && o < s))) pos += 1u << (wo - 1); }
        const uint32_t cells = 1u << (w - 1), cell = s | ((maxbits + 1 - w) << 8);
        for (uint32_t i = 0; i < cells; i++) tab[pos + i] = (uint16_t)cell;
    }
}

// ---- sequences section header (3.1.1.3.2.1) at p[pos ..) of the block p[0 .. len): the count in 1, 2 or 3 bytes and, where it is not 0, the modes
// byte; pos moves behind what was read.  false: a byte is missing
ZD_HD bool zd_seq_header(const uint8_t *p, uint32_t len, uint32_t &pos, uint32_t &nseq, uint32_t &modes) {
    nseq = 0; modes = 0;
    if (pos >= len) return false;
    const uint32_t b0 = p[pos++];
    if (b0 < 128) nseq = b0;
    else if (b0 < 255) { if (pos >= len) return false; nseq = ((b0 - 128) << 8) + p[pos++]; }
    else { if (pos + 2 > len) return false; nseq = p[pos] + ((uint32_t)p[pos + 1] << 8) + 0x7F00; pos += 2; }
    if (nseq == 0) return true;
    if (pos >= len) return false;
    modes = p[pos++];
    return true;
}
ZD_HD uint32_t zd_seq_mode(uint32_t modes, int k) { return (modes >> (6 - 2 * k)) & 3; }          // k: 0 LL, 1 OF, 2 ML (stream order)

// table k from its mode -- 0 predefined, 1 RLE (one byte at p[pos]), 2 FSE description at p[pos ..) -- into tab[0 .. 1 << alog); pos moves behind what
// was read.  Mode 3 (repeat) is the caller's: it knows what it kept.  norm[256], nexts[256]: scratch
ZD_HD bool zd_seq_table(int k, uint32_t mode, const uint8_t *p, uint32_t len, uint32_t &pos, uint32_t *tab, int16_t *norm, uint16_t *nexts, uint32_t &alog) {
    const int16_t *def = k == 0 ? ZD_LL_DEF : (k == 1 ? ZD_OF_DEF : ZD_ML_DEF);
    const int def_n = k == 0 ? 36 : (k == 1 ? 29 : 53), def_log = k == 1 ? 5 : 6;
    const int max_sym = k == 0 ? 35 : (k == 1 ? 31 : 52), max_log = k == 1 ? 8 : 9;
    if (mode == 0) {
        for (int i = 0; i < def_n; i++) norm[i] = def[i];
        alog = (uint32_t)def_log;
        return zd_fse_build(tab, norm, def_n, def_log, nexts);
    }
    if (mode == 1) {
        if (pos >= len || p[pos] > max_sym) return false;
        tab[0] = p[pos]; pos++; alog = 0;
        return true;
    }
    if (mode != 2) return false;
    int nsym, al;
    const uint32_t used = zd_fse_desc(p + pos, len - pos, norm, &nsym, &al, max_sym, max_log);
    if (!used || !zd_fse_build(tab, norm, nsym, al, nexts)) return false;
    pos += used; alog = (uint32_t)al;
    return true;
}

// ---- the Huffman streams of a literals section (4.2.2): stream q of `streams` (1, or 4 behind a 6-byte jump table) = bytes [off, off + len) of
// cs[0 .. cl), regenerates out_len bytes at out_off of the section's regen.  false: the jump table contradicts the sizes
struct ZdStream { uint32_t off, len, out_off, out_len; };
ZD_HD bool zd_huf_streams(const uint8_t *cs, uint32_t cl, uint32_t regen, uint32_t streams, uint32_t q, ZdStream &s) {
    s.off = 0; s.len = q ? 0 : cl; s.out_off = 0; s.out_len = q ? 0 : regen;
    if (streams != 4) return true;
    if (cl < 6) return false;
    const uint32_t l1 = cs[0] | (cs[1] << 8), l2 = cs[2] | (cs[3] << 8), l3 = cs[4] | (cs[5] << 8);
    const uint32_t seg = (regen + 3) / 4;
    if (6 + l1 + l2 + l3 > cl || seg * 3 > regen) return false;
    s.off = 6 + (q > 0 ? l1 : 0) + (q > 1 ? l2 : 0) + (q > 2 ? l3 : 0);
    s.len = q == 0 ? l1 : (q == 1 ? l2 : (q == 2 ? l3 : cl - 6 - l1 - l2 - l3));
    s.out_off = q * seg; s.out_len = q < 3 ? seg : regen - 3 * seg;
    return true;
}
