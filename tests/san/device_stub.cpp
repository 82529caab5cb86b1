// tests/san/device_stub.cpp -- TEST INFRASTRUCTURE: the launch layer of libpna_gpu.so on the CPU for the sanitizer builds.
// The zstd write path is stubbed with a trivially valid encoder (every segment = one frame of RAW blocks; the empty entry = the
// reference's 9-byte frame), deflate with stored blocks, the LZ launches with a recorder of what was asked of them, the framing kernels (prefix + CRC-32 + FEND, the pieces' raw CRC registers, the CRC patches, the read side's CRC check)
// are restated bytewise, the cipher kernels by keyed hashes that fold in everything the host hands them (CBC decryption: the exact inverse of the
// stub's encryption); everything else aborts: the sanitizer
// driver exercises the HOST code around the kernels, not the codecs (those are checked against the oracle on the GPU).
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <algorithm>
#include <mutex>
#include <string>
#include <vector>
#include "pna_dev.h"                                             // (with aes_core.h: the host code's key schedule, aes256_expand)
#include "../../include/pna_archive.h"

namespace pna {
[[noreturn]] static void nostub(const char *what) { fprintf(stderr, "device_stub: %s is not stubbed\n", what); abort(); }

// The LZ launches leave one text row each while a recorder is open (lz_rows_begin .. lz_rows_take: san_driver's launch matrix): what was asked of the launch
// layer, without pointer values.  "Device" memory is host memory here, so the first and the last descriptor are read through the pointer.
static std::mutex g_rows_mu; static std::string g_rows; static bool g_rows_on = false;
void lz_rows_begin() { std::lock_guard<std::mutex> lk(g_rows_mu); g_rows.clear(); g_rows_on = true; }
std::string lz_rows_take() { std::lock_guard<std::mutex> lk(g_rows_mu); g_rows_on = false; return std::move(g_rows); }
static void lz_row(const char *entry, const LzLaunch &L, int w3) {
    std::lock_guard<std::mutex> lk(g_rows_mu);
    if (!g_rows_on) return;
    static const char *const forms[] = {"one-kernel", "split", "split+waveparse", "match-only", "small"};
    const bool small = L.form == LzForm::Small, grid = L.form == LzForm::Split || L.form == LzForm::SplitWaveParse || small;
    char b[512]; int n = snprintf(b, sizeof b, "%s %s nseg=%u", entry, forms[(int)L.form], L.nseg);
    for (const SegDesc *sd : {L.segs, L.segs + (L.nseg ? L.nseg - 1 : 0)})
        if (L.nseg) n += snprintf(b + n, sizeof b - n, " {%llu,%u,%u,%u,%u,%u}", (unsigned long long)sd->src_off, sd->len, sd->blk_base, sd->blk_log, sd->u0, sd->u1);
    snprintf(b + n, sizeof b - n, " flags=%08x max_off=%ld max_len=%u blk0=%u ctab=%d pbuf=%d gtab=%d ev=%d nb=%ld hist=%d w3=%d\n", L.flags, small ? -1l : (long)L.max_off, L.max_len, L.blk0,
             L.ctab != nullptr, L.pbuf != nullptr, L.gtab != nullptr, L.ev_match != nullptr, grid ? (long)L.pg.nb : -1l, grid && L.pg.hist, w3);
    g_rows += b;
}
void launch_lz(const LzLaunch &L) { lz_row("launch_lz", L, -1); }
void launch_lz_small(const LzLaunch &L, bool w3) { lz_row("launch_lz_small", L, w3); }
void launch_default_tables(hipStream_t) {}
uint32_t lz_gtab_log() { return 19; }
// (the row: whether the entropy stage was told that the parse kernel has counted every segment's sequence codes -- the LZ stage decides that)
void launch_entropy_chunk(const SegDesc *, uint32_t, uint32_t, const uint32_t *, uint32_t, uint32_t, const uint64_t *, const uint8_t *, BlkInfo *, SegTables *,
                          uint8_t *, uint8_t *, uint32_t *, uint32_t, uint32_t, uint32_t *hist, hipStream_t, hipEvent_t *, hipStream_t, hipEvent_t, hipEvent_t, bool, const uint32_t *seq_hist) {
    std::lock_guard<std::mutex> lk(g_rows_mu);
    if (g_rows_on) g_rows += std::string("launch_entropy_chunk hist=") + (hist ? "1" : "0") + " seq_hist=" + (seq_hist ? "1" : "0") + "\n";
}
static uint64_t seg_bytes(const SegDesc &sd) {
    if (sd.len == 0) return 9;
    return 6 + 3ull * seg_nblk(sd) + sd.len;
}
void launch_plan(const SegDesc *segs, uint32_t nseg, BlkInfo *, const SegTables *, uint64_t *seg_size, uint64_t *seg_off, uint32_t, hipStream_t) {
    uint64_t pos = 0;
    for (uint32_t s = 0; s < nseg; s++) { seg_size[s] = seg_bytes(segs[s]); seg_off[s] = pos; pos += seg_size[s]; }
    seg_off[nseg] = pos;
}
void launch_write(const uint8_t *src, const SegDesc *segs, uint32_t nseg, const uint32_t *, uint32_t, const BlkInfo *, const SegTables *,
                  const uint64_t *seg_off, const uint8_t *, const uint8_t *, const uint8_t *, uint8_t *dst, bool, hipStream_t, bool) {
    for (uint32_t s = 0; s < nseg; s++) {
        const SegDesc &sd = segs[s];
        uint8_t *o = dst + seg_off[s];
        if (sd.len == 0) { static const uint8_t e[9] = {0x28, 0xB5, 0x2F, 0xFD, 0x20, 0x00, 0x01, 0x00, 0x00}; memcpy(o, e, 9); continue; }
        static const uint8_t h[6] = {0x28, 0xB5, 0x2F, 0xFD, 0x00, 0x50};
        memcpy(o, h, 6); o += 6;
        const uint32_t bsz = 1u << sd.blk_log;                                      // (small batches run on smaller blocks: latency mode)
        for (uint32_t b0 = 0; b0 < sd.len; b0 += bsz) {
            const uint32_t bl = sd.len - b0 < bsz ? sd.len - b0 : bsz;
            const uint32_t hd = (b0 + bl == sd.len ? 1u : 0u) | (bl << 3);          // last | raw (0) << 1 | size << 3
            o[0] = (uint8_t)hd; o[1] = (uint8_t)(hd >> 8); o[2] = (uint8_t)(hd >> 16);
            memcpy(o + 3, src + sd.src_off + b0, bl); o += 3 + bl;
        }
    }
}
void launch_frame(const FrameDesc *fd, uint32_t n, const uint8_t *blob, const CrcTabs *, uint8_t *dst, uint64_t, uint32_t fend_crc, const char ty[4], bool with_fend, hipStream_t, uint32_t) {
    for (uint32_t i = 0; i < n; i++) {
        const FrameDesc &d = fd[i];
        memcpy(dst + d.arc_off, blob + d.prefix_off, d.prefix_len);
        uint8_t *pay = dst + d.arc_off + d.prefix_len;
        const uint32_t crc = pna_crc32(pna_crc32(0, ty, 4), pay, d.payload_len);
        uint8_t *q = pay + d.payload_len;
        q[0] = (uint8_t)(crc >> 24); q[1] = (uint8_t)(crc >> 16); q[2] = (uint8_t)(crc >> 8); q[3] = (uint8_t)crc;
        if (with_fend && !(d.pad & 2)) {
            const uint8_t fe[12] = {0, 0, 0, 0, 'F', 'E', 'N', 'D', (uint8_t)(fend_crc >> 24), (uint8_t)(fend_crc >> 16), (uint8_t)(fend_crc >> 8), (uint8_t)fend_crc};
            memcpy(q + 4, fe, 12);
        }
    }
}
struct PlaceDesc { uint64_t src_off, dst_off; uint32_t len, pad; };
void launch_place(const void *pd, uint32_t n, const uint8_t *src, uint8_t *dst, hipStream_t) {
    for (uint32_t i = 0; i < n; i++) { const PlaceDesc &d = ((const PlaceDesc *)pd)[i]; memcpy(dst + d.dst_off, src + d.src_off, d.len); }
}
void launch_gather(const void *pd, uint32_t n, const uint8_t *src, uint8_t *dst, hipStream_t st) { launch_place(pd, n, src, dst, st); }
void launch_layout(FrameDesc *fd, uint8_t *blob, const uint32_t *entry_seg, const uint64_t *seg_off, uint32_t nentry, uint32_t nseg, uint64_t out_base,
                   uint64_t *segdst, uint64_t *ent_off, uint64_t *total, hipStream_t) {
    uint64_t pos = out_base;
    for (uint32_t i = 0; i < nentry; i++) {
        const uint32_t s0 = entry_seg[i], s1 = entry_seg[i + 1];
        const uint64_t base = seg_off[s0], plen = seg_off[s1] - base;
        fd[i].arc_off = pos; fd[i].payload_len = (uint32_t)plen;
        uint8_t *lenf = blob + fd[i].prefix_off + fd[i].prefix_len - 8;
        lenf[0] = (uint8_t)(plen >> 24); lenf[1] = (uint8_t)(plen >> 16); lenf[2] = (uint8_t)(plen >> 8); lenf[3] = (uint8_t)plen;
        for (uint32_t sg = s0; sg < s1; sg++) segdst[sg] = pos + fd[i].prefix_len + (seg_off[sg] - base);
        ent_off[i] = pos;
        pos += fd[i].prefix_len + plen + 16;
    }
    segdst[nseg] = pos; ent_off[nentry] = pos; *total = pos - out_base;
}
void launch_link_copy(const uint8_t *src, uint8_t *dst, size_t n, uint32_t, hipStream_t) { memcpy(dst, src, n); }
void launch_link_gather(const void *segs, uint32_t nseg, uint32_t, hipStream_t) {
    struct Seg { const uint8_t *src; uint8_t *dst; uint64_t len; };
    for (uint32_t i = 0; i < nseg; i++) memcpy(((const Seg *)segs)[i].dst, ((const Seg *)segs)[i].src, ((const Seg *)segs)[i].len);
}
void lz_read_stamps(unsigned long long *out) { memset(out, 0, 8 * sizeof *out); }

// deflate as stored blocks, so that a deflate call completes (the launch matrix looks at the LZ launches in front of these, not at the bytes): the zlib header in front of an
// entry's first segment, every segment as stored blocks of at most 65 535 bytes (an empty one: one empty block), BFINAL and four trailer bytes (zeros: no Adler-32) on the entry's last
static uint64_t stored_bytes(const SegDesc &sd) { return (sd.first & 1 ? 2 : 0) + 5ull * std::max<uint32_t>(1, (sd.len + 65534) / 65535) + sd.len + (sd.first & 2 ? 4 : 0); }
void launch_deflate_stage1(const uint8_t *, const SegDesc *segs, uint32_t nseg, const uint32_t *, uint32_t, const uint64_t *, const uint8_t *, BlkInfo *, const uint4 *, DeflTables *,
                           uint8_t *, uint64_t *seg_size, uint64_t *seg_off, hipStream_t, hipEvent_t *, uint32_t, bool, bool) {
    uint64_t pos = 0;
    for (uint32_t s = 0; s < nseg; s++) { seg_size[s] = stored_bytes(segs[s]); seg_off[s] = pos; pos += seg_size[s]; }
    seg_off[nseg] = pos;
}
void launch_deflate_write(const uint8_t *src, const SegDesc *segs, const uint32_t *, uint32_t, const BlkInfo *, const uint64_t *seg_off, const uint64_t *, const uint8_t *, const uint32_t *entry_seg,
                          uint32_t nentry, uint8_t *dst, hipStream_t, bool, bool) {
    for (uint32_t s = 0; s < entry_seg[nentry]; s++) {
        const SegDesc &sd = segs[s];
        uint8_t *o = dst + seg_off[s];
        if (sd.first & 1) { *o++ = 0x78; *o++ = 0x01; }
        for (uint32_t b0 = 0; b0 == 0 || b0 < sd.len; b0 += 65535) {
            const uint32_t bl = std::min<uint32_t>(sd.len - b0, 65535);
            const uint8_t h[5] = {(uint8_t)((sd.first & 2) && b0 + bl == sd.len), (uint8_t)bl, (uint8_t)(bl >> 8), (uint8_t)~bl, (uint8_t)(~bl >> 8)};
            memcpy(o, h, 5); memcpy(o + 5, src + sd.src_off + b0, bl); o += 5 + bl;
        }
        if (sd.first & 2) memset(o, 0, 4);
    }
}
// The read side's CRC check (k_frame in verify mode) over whole chunks: verify[0] counts mismatches, verify[1] keeps the lowest failing descriptor index
void launch_frame_verify(const FrameDesc *fd, uint32_t n, const CrcTabs *, const uint8_t *buf, uint64_t, const char ty[4], uint32_t *verify, hipStream_t, uint32_t) {
    for (uint32_t i = 0; i < n; i++) {
        const FrameDesc &d = fd[i];
        if (d.pad & 4) nostub("frame_verify (pieces)");
        const uint8_t *pay = buf + d.arc_off + d.prefix_len, *q = pay + d.payload_len;
        const uint32_t stored = ((uint32_t)q[0] << 24) | ((uint32_t)q[1] << 16) | ((uint32_t)q[2] << 8) | q[3];
        if (pna_crc32(pna_crc32(0, ty, 4), pay, d.payload_len) != stored) { verify[0]++; if (i < verify[1]) verify[1] = i; }
    }
}
void launch_zdec(ZFrame *, uint32_t, const uint8_t *, uint8_t *, uint8_t *, uint32_t, hipStream_t) { nostub("zdec"); }
void launch_zparse_big_a(ZFrame *, ZFrameX *, const uint32_t *, uint32_t, const uint8_t *, ZBlock *, uint32_t *, void *, hipStream_t) { nostub("zparse"); }
void launch_zparse_big_b(ZFrame *, ZFrameX *, uint32_t, const uint8_t *, ZBlock *, ZTables *, uint32_t *, uint32_t *, void *, const uint32_t *, hipStream_t) { nostub("zparse"); }
struct ZxFrame;
int launch_zexec_par(ZxFrame *, const ZxFrame &, const ZBlock *, const uint8_t *, const uint8_t *, uint64_t *, uint32_t *, uint32_t *, uint8_t *, uint32_t *, uint32_t *, hipStream_t, uint32_t, const uint32_t *, const uint64_t *) { nostub("zexec_par"); return -1; }
void launch_zxxh(ZFrame *, uint32_t, const uint8_t *, const uint8_t *, hipStream_t) { nostub("zxxh"); }
void launch_zscan(const ZEntry *, uint32_t, const uint8_t *, ZFrame *, ZFrameX *, hipStream_t) { nostub("zscan"); }
void launch_zcount(const ZEntry *, uint32_t, const uint8_t *, uint32_t *, hipStream_t) { nostub("zcount"); }
void launch_zlist(const uint8_t *, uint64_t, uint64_t, uint64_t, void *, uint32_t, uint64_t *, hipStream_t) { nostub("zlist"); }
void launch_zparse(ZFrame *, ZFrameX *, uint32_t, const uint8_t *, ZBlock *, ZTables *, uint32_t *, uint32_t *, void *, hipStream_t) { nostub("zparse"); }
void launch_zstreams(uint32_t, uint32_t, const uint32_t *, const uint32_t *, const void *, ZBlock *, const ZFrame *, const ZTables *, const uint8_t *, uint8_t *, uint64_t *, hipStream_t) { nostub("zstreams"); }
void launch_inflate(ZFrame *, ZFrameX *, uint32_t, const uint8_t *, ZBlock *, uint8_t *, uint64_t *, const uint32_t *, hipStream_t) { nostub("inflate"); }
void launch_ispec(const uint8_t *, uint64_t, uint64_t, uint32_t, uint32_t, uint64_t *, hipStream_t) { nostub("inflate (chunk starts)"); }
void launch_inflate_chunks(ZFrame *, ZFrameX *, uint32_t, void *, uint32_t, uint32_t, const uint8_t *, ZBlock *, uint8_t *, uint64_t *, hipStream_t) { nostub("inflate (chunks)"); }
void launch_icount(const uint8_t *, const uint64_t *, const uint64_t *, uint32_t, uint32_t *, uint32_t, hipStream_t) { nostub("inflate"); }
void launch_vinflate(ZFrame *, ZFrameX *, uint32_t, const void *, uint32_t, uint64_t *, uint32_t *, uint32_t *, uint32_t, const uint8_t *, ZBlock *, uint8_t *, uint64_t *, hipStream_t) { nostub("inflate"); }
void launch_iadler(ZFrame *, const ZFrameX *, const ZBlock *, uint32_t, const uint32_t *, uint32_t, const uint8_t *, void *, hipStream_t) { nostub("iadler"); }
void launch_zexec(ZFrame *, const ZFrameX *, uint32_t, ZBlock *, const uint8_t *, const uint8_t *, const uint64_t *, uint8_t *, hipStream_t) { nostub("zexec"); }
void launch_zexec_groups(ZFrame *, const ZFrameX *, uint32_t, ZBlock *, const void *, uint32_t, const uint8_t *, const uint8_t *, const uint64_t *, uint8_t *, hipStream_t) { nostub("zexec"); }
void launch_gcm_verify(const GcmEntry *, uint32_t, const uint8_t *, const uint8_t *, uint32_t *, hipStream_t) { nostub("gcm"); }
// Pieces of chunks (k_frame's piece mode, FrameDesc::pad bit 8 = a later piece): the raw CRC-32 register of "FDAT" || piece with the folded initial value
// (first piece) or of the piece's bytes from register 0 (later piece); pna_crc32(c, ..) = ~register(~c, ..)
void launch_frame_pieces(const FrameDesc *fd, uint32_t n, const CrcTabs *, const uint8_t *buf, uint64_t, const char ty[4], uint32_t *states, hipStream_t) {
    for (uint32_t i = 0; i < n; i++) {
        const FrameDesc &d = fd[i];
        const uint8_t *pay = buf + d.arc_off + d.prefix_len;
        states[i] = (d.pad & 8) ? ~pna_crc32(0xFFFFFFFFu, pay, d.payload_len) : ~pna_crc32(pna_crc32(0, ty, 4), pay, d.payload_len);
    }
}
struct CrcPatch { int64_t off; uint32_t crc, mask; };
void launch_crc_patch(const void *patches, uint32_t n, uint8_t *dst, hipStream_t) {
    for (uint32_t i = 0; i < n; i++) {
        const CrcPatch &q = ((const CrcPatch *)patches)[i];
        for (int j = 0; j < 4; j++) if ((q.mask >> j) & 1) dst[q.off + j] = (uint8_t)(q.crc >> (24 - 8 * j));
    }
}
// The cipher stage: no AES, but every byte written depends on everything the host hands the kernels -- the unit's offset (where it writes) and stream
// position, its IV, the round keys (the call's, or GCM's per-segment ones) -- and a GCM tag on the segment's bytes, length, hash subkey and E(K, J0).
static uint64_t mix64(uint64_t z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31);
}
static uint64_t fold(uint64_t h, const void *p, size_t n) {
    for (size_t i = 0; i < n; i++) h = (h ^ ((const uint8_t *)p)[i]) * 0x100000001B3ull;
    return mix64(h);
}
void launch_aes_ctr(const CipherUnit *units, uint32_t n, const uint8_t *ivs, const AesTabs *, uint8_t *buf, const AesKey &key, const AesKey *keys, hipStream_t) {
    for (uint32_t i = 0; i < n; i++) {
        const CipherUnit &u = units[i];
        const uint64_t seed = fold(fold(0xC7Bull, ivs + 16 * (size_t)u.iv_idx, 16), keys ? keys[u.iv_idx].rk : key.rk, sizeof key.rk);
        for (uint32_t j = 0; j < u.len; j++) { const uint64_t p = u.pos + j; buf[u.off + j] ^= (uint8_t)(mix64(seed + (p >> 3)) >> (8 * (p & 7))); }
    }
}
void launch_aes_cbc_enc(const CipherUnit *units, uint32_t n, const uint8_t *ivs, const AesTabs *, uint8_t *buf, const AesKey &key, hipStream_t) {
    const uint64_t kh = fold(0xCBCull, key.rk, sizeof key.rk);
    for (uint32_t i = 0; i < n; i++) {                          // PKCS#7 padding, then every block XORed with a hash of the block before (the IV first)
        const CipherUnit &u = units[i];
        uint8_t *p = buf + u.off;
        const uint32_t padded = (u.len / 16 + 1) * 16;
        memset(p + u.len, (int)(padded - u.len), padded - u.len);
        uint8_t prev[16]; memcpy(prev, ivs + 16 * (size_t)u.iv_idx, 16);
        for (uint32_t b = 0; b < padded; b += 16) {
            const uint64_t h0 = fold(kh, prev, 16), h1 = mix64(h0 + 1);
            for (int j = 0; j < 16; j++) p[b + j] ^= (uint8_t)((j < 8 ? h0 : h1) >> (8 * (j & 7)));
            memcpy(prev, p + b, 16);
        }
    }
}
// The encryption round keys behind a decryption schedule.  aes256_dec_key (aes_core.h) builds the equivalent inverse cipher's schedule: the
// encryption round keys in reverse order, d.rk[4 r + c] = InvMixColumns(k.rk[4 (14 - r) + c]) for rounds 1 .. 13, rounds 0 and 14 swapped as they
// are.  AES-256's round keys 0 and 1 are the key itself: round 0 is d.rk[56 .. 59], round 1 is MixColumns(d.rk[52 .. 55]); the expansion gives the
// rest.  (The stub's CBC encryption folds the encryption schedule, and its bytes are pinned by the framing matrix.)
static AesKey enc_key_of(const AesKey &dk) {
    auto x2 = [](uint8_t a) { return (uint8_t)((a << 1) ^ ((a & 0x80) ? 0x1B : 0)); };
    uint8_t key[32];
    for (int c4 = 0; c4 < 4; c4++) {
        uint8_t a[4];
        for (int j = 0; j < 4; j++) { key[4 * c4 + j] = (uint8_t)(dk.rk[56 + c4] >> (8 * j)); a[j] = (uint8_t)(dk.rk[52 + c4] >> (8 * j)); }
        for (int j = 0; j < 4; j++) key[16 + 4 * c4 + j] = x2(a[j]) ^ x2(a[(j + 1) & 3]) ^ a[(j + 1) & 3] ^ a[(j + 2) & 3] ^ a[(j + 3) & 3];
    }
    AesKey ek; aes256_expand(key, ek);
    return ek;
}
// the exact inverse of launch_aes_cbc_enc, in place; plain_len: a unit's plaintext length, 0xFFFFFFFF on a bad length or PKCS#7 padding (k_aes_cbc_dec)
void launch_aes_cbc_dec(const CipherUnit *units, uint32_t n, const uint8_t *ivs, const AesDecTabs *, uint8_t *buf, const AesKey &dkey, uint32_t *plain_len, hipStream_t) {
    const AesKey ek = enc_key_of(dkey);
    const uint64_t kh = fold(0xCBCull, ek.rk, sizeof ek.rk);
    for (uint32_t i = 0; i < n; i++) {
        const CipherUnit &u = units[i];
        if (u.len == 0 || (u.len & 15)) { plain_len[i] = 0xFFFFFFFFu; continue; }
        uint8_t *p = buf + u.off;
        uint8_t prev[16]; memcpy(prev, ivs + 16 * (size_t)u.iv_idx, 16);
        for (uint32_t b = 0; b < u.len; b += 16) {
            uint8_t ct[16]; memcpy(ct, p + b, 16);
            const uint64_t h0 = fold(kh, prev, 16), h1 = mix64(h0 + 1);
            for (int j = 0; j < 16; j++) p[b + j] ^= (uint8_t)((j < 8 ? h0 : h1) >> (8 * (j & 7)));
            memcpy(prev, ct, 16);
        }
        const uint32_t pad = p[u.len - 1];
        bool ok = pad >= 1 && pad <= 16;
        for (uint32_t k = 0; ok && k < pad; k++) ok = p[u.len - 1 - k] == pad;
        plain_len[i] = ok ? u.len - pad : 0xFFFFFFFFu;
    }
}
void launch_gcm_tag(const GcmEntry *ents, uint32_t n, uint8_t *buf, hipStream_t) {
    for (uint32_t i = 0; i < n; i++) {
        const GcmEntry &g = ents[i];
        uint64_t h = fold(fold(fold(0x6C3ull, &g.len, 4), &g.pad, 4), g.h, 16);          // (not `off`: a buffer offset, it picks the bytes)
        h = fold(fold(h, g.ej0, 16), buf + g.off, g.len);
        const uint64_t h1 = mix64(h + 1);
        for (int j = 0; j < 16; j++) buf[g.off + g.len + j] = (uint8_t)((j < 8 ? h : h1) >> (8 * (j & 7)));
    }
}
void launch_corpus(int, uint64_t, uint64_t, uint64_t, uint64_t, const uint8_t *, const uint64_t *, const uint32_t *, uint8_t *, hipStream_t) { nostub("corpus"); }
} // namespace pna
