// camellia_core.h -- Camellia-256 (RFC 3713) in one place, for the host code and the kernels of k_cipher.hip: key schedule, the decrypt-order
// schedule, and the block function in two forms -- a byte-wise one straight from the RFC's text (host only: what the tests hold the other against) and
// the table form the kernels run.  Builds with g++ alone (tests/camellia_core); no HIP header is needed.
//
// Replaces the Camellia arm of the reference's cipher choice (Encryption::CAMELLIA = 2, lib/src/cipher.rs:16-77).  The modes around the block function
// -- Ctr128BE, CBC with PKCS#7, GCM STREAM -- are those of the AES path.
//
// The table form: F's P-function is linear over the eight substituted bytes z1 .. z8, so with the 32-bit patterns (most significant byte first)
//     T0[x] = (s1, s1, s1, 0)   T1[x] = (0, s2, s2, s2)   T2[x] = (s3, 0, s3, s3)   T3[x] = (s4, s4, 0, s4)       s_i = SBOX_i[x]
//     D = T0[t1] ^ T1[t2] ^ T2[t3] ^ T3[t4]        U = T1[t5] ^ T2[t6] ^ T3[t7] ^ T0[t8]
// the result is  high word = D ^ U,  low word = D ^ U ^ rotr32(D, 8): eight look-ups in four tables per F.  The table accessor is a parameter
// (tab(i, x) = T_i[x]): host code reads a plain array (CamTabs), a kernel its LDS layout.
#pragma once
#include <stdint.h>
#include <stddef.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define CAM_HD __host__ __device__ __forceinline__
#else
#define CAM_HD inline
#endif

// The 34 64-bit subkeys as (high, low) 32-bit halves -- word 2 i is the high half of subkey i -- in the order the ENCRYPTION network meets them:
// kw1 kw2 | k1..k6 | ke1 ke2 | k7..k12 | ke3 ke4 | k13..k18 | ke5 ke6 | k19..k24 | kw3 kw4.  272 bytes: a kernel argument (scalar registers).
struct CamKey { uint32_t k[68]; };
struct CamTabs { uint32_t T[4][256]; };
struct CamHostTab {                       // the accessor of host code
    const CamTabs *t;
    uint32_t operator()(uint32_t i, uint32_t x) const { return t->T[i][x]; }
};

CAM_HD uint32_t cam_rotl32(uint32_t v, uint32_t n) { return (v << n) | (v >> (32 - n)); }     // n = 1 .. 31

// F(x, k) in halves: (xh, xl) ^ (kh, kl) through the S-boxes and P
template <class Tab>
CAM_HD void cam_f(const Tab &tab, uint32_t xh, uint32_t xl, uint32_t kh, uint32_t kl, uint32_t &yh, uint32_t &yl) {
    const uint32_t a = xh ^ kh, b = xl ^ kl;
    const uint32_t d = tab(0, a >> 24) ^ tab(1, (a >> 16) & 0xFF) ^ tab(2, (a >> 8) & 0xFF) ^ tab(3, a & 0xFF);
    const uint32_t u = tab(1, b >> 24) ^ tab(2, (b >> 16) & 0xFF) ^ tab(3, (b >> 8) & 0xFF) ^ tab(0, b & 0xFF);
    yh = d ^ u;
    yl = yh ^ ((d >> 8) | (d << 24));
}
CAM_HD void cam_fl(uint32_t &x1, uint32_t &x2, uint32_t k1, uint32_t k2) { x2 ^= cam_rotl32(x1 & k1, 1); x1 ^= (x2 | k2); }
CAM_HD void cam_flinv(uint32_t &y1, uint32_t &y2, uint32_t k1, uint32_t k2) { y1 ^= (y2 | k2); y2 ^= cam_rotl32(y1 & k1, 1); }

// One block through the network under the schedule `key` -- the encryption schedule encrypts, the decrypt-order one (cam_dec_key) decrypts.
// In and out: the block as four big-endian words (w0 = bytes 0..3).
template <class Tab>
CAM_HD void cam_block(const Tab &tab, const CamKey &key, uint32_t &w0, uint32_t &w1, uint32_t &w2, uint32_t &w3) {
    const uint32_t *k = key.k;
    uint32_t d1h = w0 ^ k[0], d1l = w1 ^ k[1], d2h = w2 ^ k[2], d2l = w3 ^ k[3];
    uint32_t yh, yl;
#define CAM_ROUND2(i) \
    cam_f(tab, d1h, d1l, k[2 * (i)], k[2 * (i) + 1], yh, yl); d2h ^= yh; d2l ^= yl; \
    cam_f(tab, d2h, d2l, k[2 * (i) + 2], k[2 * (i) + 3], yh, yl); d1h ^= yh; d1l ^= yl;
    CAM_ROUND2(2) CAM_ROUND2(4) CAM_ROUND2(6)
    cam_fl(d1h, d1l, k[16], k[17]); cam_flinv(d2h, d2l, k[18], k[19]);
    CAM_ROUND2(10) CAM_ROUND2(12) CAM_ROUND2(14)
    cam_fl(d1h, d1l, k[32], k[33]); cam_flinv(d2h, d2l, k[34], k[35]);
    CAM_ROUND2(18) CAM_ROUND2(20) CAM_ROUND2(22)
    cam_fl(d1h, d1l, k[48], k[49]); cam_flinv(d2h, d2l, k[50], k[51]);
    CAM_ROUND2(26) CAM_ROUND2(28) CAM_ROUND2(30)
#undef CAM_ROUND2
    w0 = d2h ^ k[64]; w1 = d2l ^ k[65]; w2 = d1h ^ k[66]; w3 = d1l ^ k[67];
}

// The same network with the subkeys reversed (kw1 <-> kw3, kw2 <-> kw4, k1 <-> k24 ..., ke1 <-> ke6 ...): the schedule read backwards, the
// whitening pairs at either end put back in order
CAM_HD void cam_dec_key(const CamKey &e, CamKey &d) {
    for (int i = 0; i < 34; i++) { d.k[2 * i] = e.k[2 * (33 - i)]; d.k[2 * i + 1] = e.k[2 * (33 - i) + 1]; }
    for (int p = 0; p <= 64; p += 64) {
        const uint32_t h = d.k[p], l = d.k[p + 1];
        d.k[p] = d.k[p + 2]; d.k[p + 1] = d.k[p + 3]; d.k[p + 2] = h; d.k[p + 3] = l;
    }
}

CAM_HD uint32_t cam_be32(const uint8_t *p) { return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3]; }
CAM_HD void cam_put_be32(uint8_t *p, uint32_t v) { p[0] = (uint8_t)(v >> 24); p[1] = (uint8_t)(v >> 16); p[2] = (uint8_t)(v >> 8); p[3] = (uint8_t)v; }

// 128-bit value v (four big-endian words) rotated left by n (0 .. 127): its high 64 bits to out[0..1], its low 64 to out[2..3]
CAM_HD void cam_rot128(const uint32_t v[4], uint32_t n, uint32_t out[4]) {
    const uint32_t ws = n >> 5, bs = n & 31;
    for (uint32_t i = 0; i < 4; i++) {
        const uint32_t a = v[(i + ws) & 3], b = v[(i + ws + 1) & 3];
        out[i] = bs ? (a << bs) | (b >> (32 - bs)) : a;
    }
}

// The key schedule of a 256-bit key (RFC 3713 2.2)
template <class Tab>
CAM_HD void cam_expand(const Tab &tab, const uint8_t key[32], CamKey &out) {
    const uint32_t SIG[12] = {0xA09E667Fu, 0x3BCC908Bu, 0xB67AE858u, 0x4CAA73B2u, 0xC6EF372Fu, 0xE94F82BEu,
                              0x54FF53A5u, 0xF1D36F1Cu, 0x10E527FAu, 0xDE682D1Du, 0xB05688C2u, 0xB3E6C1FDu};
    uint32_t KL[4], KR[4], KA[4], KB[4], d[4], yh, yl;
    for (int i = 0; i < 4; i++) { KL[i] = cam_be32(key + 4 * i); KR[i] = cam_be32(key + 16 + 4 * i); d[i] = KL[i] ^ KR[i]; }
    cam_f(tab, d[0], d[1], SIG[0], SIG[1], yh, yl); d[2] ^= yh; d[3] ^= yl;
    cam_f(tab, d[2], d[3], SIG[2], SIG[3], yh, yl); d[0] ^= yh; d[1] ^= yl;
    for (int i = 0; i < 4; i++) d[i] ^= KL[i];
    cam_f(tab, d[0], d[1], SIG[4], SIG[5], yh, yl); d[2] ^= yh; d[3] ^= yl;
    cam_f(tab, d[2], d[3], SIG[6], SIG[7], yh, yl); d[0] ^= yh; d[1] ^= yl;
    for (int i = 0; i < 4; i++) { KA[i] = d[i]; d[i] ^= KR[i]; }
    cam_f(tab, d[0], d[1], SIG[8], SIG[9], yh, yl); d[2] ^= yh; d[3] ^= yl;
    cam_f(tab, d[2], d[3], SIG[10], SIG[11], yh, yl); d[0] ^= yh; d[1] ^= yl;
    for (int i = 0; i < 4; i++) KB[i] = d[i];
    // subkey pairs in the order of the network: which of KL, KR, KA, KB (0 .. 3), rotated by how much
    const uint8_t who[17] = {0, 3, 1, 2, 1, 3, 0, 2, 0, 1, 3, 0, 2, 1, 2, 0, 3};
    const uint8_t rot[17] = {0, 0, 15, 15, 30, 30, 45, 45, 60, 60, 60, 77, 77, 94, 94, 111, 111};
    for (int p = 0; p < 17; p++) {
        const uint32_t *src = who[p] == 0 ? KL : who[p] == 1 ? KR : who[p] == 2 ? KA : KB;
        cam_rot128(src, rot[p], out.k + 4 * p);
    }
}

// ------------------------------------------------------------------ host only: the S-box, the tables, the byte-wise form
static const uint8_t CAM_SBOX1[256] = {
    112,130, 44,236,179, 39,192,229,228,133, 87, 53,234, 12,174, 65,  35,239,107,147, 69, 25,165, 33,237, 14, 79, 78, 29,101,146,189,
    134,184,175,143,124,235, 31,206, 62, 48,220, 95, 94,197, 11, 26, 166,225, 57,202,213, 71, 93, 61,217,  1, 90,214, 81, 86,108, 77,
    139, 13,154,102,251,204,176, 45,116, 18, 43, 32,240,177,132,153, 223, 76,203,194, 52,126,118,  5,109,183,169, 49,209, 23,  4,215,
     20, 88, 58, 97,222, 27, 17, 28, 50, 15,156, 22, 83, 24,242, 34, 254, 68,207,178,195,181,122,145, 36,  8,232,168, 96,252,105, 80,
    170,208,160,125,161,137, 98,151, 84, 91, 30,149,224,255,100,210,  16,196,  0, 72,163,247,117,219,138,  3,230,218,  9, 63,221,148,
    135, 92,131,  2,205, 74,144, 51,115,103,246,243,157,127,191,226,  82,155,216, 38,200, 55,198, 59,129,150,111, 75, 19,190, 99, 46,
    233,121,167,140,159,110,188,142, 41,245,249,182, 47,253,180, 89, 120,152,  6,106,231, 70,113,186,212, 37,171, 66,136,162,141,250,
    114,  7,185, 85,248,238,172, 10, 54, 73, 42,104, 60, 56,241,164,  64, 40,211,123,187,201, 67,193, 21,227,173,244,119,199,128,158};
inline uint8_t cam_rotl8(uint8_t v, int n) { return (uint8_t)((v << n) | (v >> (8 - n))); }
inline uint8_t cam_sbox(int which, uint8_t x) {          // SBOX1 .. SBOX4 (which = 1 .. 4)
    return which == 1 ? CAM_SBOX1[x] : which == 2 ? cam_rotl8(CAM_SBOX1[x], 1) : which == 3 ? cam_rotl8(CAM_SBOX1[x], 7) : CAM_SBOX1[cam_rotl8(x, 1)];
}
inline void cam_build_tabs(CamTabs &t) {
    for (uint32_t x = 0; x < 256; x++) {
        const uint32_t s1 = cam_sbox(1, (uint8_t)x), s2 = cam_sbox(2, (uint8_t)x), s3 = cam_sbox(3, (uint8_t)x), s4 = cam_sbox(4, (uint8_t)x);
        t.T[0][x] = (s1 << 24) | (s1 << 16) | (s1 << 8);
        t.T[1][x] = (s2 << 16) | (s2 << 8) | s2;
        t.T[2][x] = (s3 << 24) | (s3 << 8) | s3;
        t.T[3][x] = (s4 << 24) | (s4 << 16) | s4;
    }
}
inline const CamTabs &cam_host_tabs() { static const CamTabs T = [] { CamTabs x; cam_build_tabs(x); return x; }(); return T; }     // (thread-safe: C++11 static)
inline void cam_expand_host(const uint8_t key[32], CamKey &k) { cam_expand(CamHostTab{&cam_host_tabs()}, key, k); }
// one block on the host, bytes in and out; `k`: the encryption schedule to encrypt, the decrypt-order one to decrypt
inline void cam_block_host(const CamKey &k, const uint8_t in[16], uint8_t out[16]) {
    uint32_t w0 = cam_be32(in), w1 = cam_be32(in + 4), w2 = cam_be32(in + 8), w3 = cam_be32(in + 12);
    cam_block(CamHostTab{&cam_host_tabs()}, k, w0, w1, w2, w3);
    cam_put_be32(out, w0); cam_put_be32(out + 4, w1); cam_put_be32(out + 8, w2); cam_put_be32(out + 12, w3);
}

// ---- the byte-wise form, straight from RFC 3713: 64-bit values, one S-box look-up and one XOR chain per byte
inline uint64_t cam_ref_f(uint64_t x, uint64_t k) {
    x ^= k;
    uint8_t t[8];
    for (int i = 0; i < 8; i++) t[i] = (uint8_t)(x >> (56 - 8 * i));
    const int box[8] = {1, 2, 3, 4, 2, 3, 4, 1};
    for (int i = 0; i < 8; i++) t[i] = cam_sbox(box[i], t[i]);
    const uint8_t y[8] = {(uint8_t)(t[0] ^ t[2] ^ t[3] ^ t[5] ^ t[6] ^ t[7]), (uint8_t)(t[0] ^ t[1] ^ t[3] ^ t[4] ^ t[6] ^ t[7]),
                          (uint8_t)(t[0] ^ t[1] ^ t[2] ^ t[4] ^ t[5] ^ t[7]), (uint8_t)(t[1] ^ t[2] ^ t[3] ^ t[4] ^ t[5] ^ t[6]),
                          (uint8_t)(t[0] ^ t[1] ^ t[5] ^ t[6] ^ t[7]), (uint8_t)(t[1] ^ t[2] ^ t[4] ^ t[6] ^ t[7]),
                          (uint8_t)(t[2] ^ t[3] ^ t[4] ^ t[5] ^ t[7]), (uint8_t)(t[0] ^ t[3] ^ t[4] ^ t[5] ^ t[6])};
    uint64_t r = 0;
    for (int i = 0; i < 8; i++) r = (r << 8) | y[i];
    return r;
}
inline uint64_t cam_ref_fl(uint64_t x, uint64_t ke) {
    uint32_t x1 = (uint32_t)(x >> 32), x2 = (uint32_t)x; const uint32_t k1 = (uint32_t)(ke >> 32), k2 = (uint32_t)ke;
    x2 ^= cam_rotl32(x1 & k1, 1); x1 ^= (x2 | k2);
    return ((uint64_t)x1 << 32) | x2;
}
inline uint64_t cam_ref_flinv(uint64_t y, uint64_t ke) {
    uint32_t y1 = (uint32_t)(y >> 32), y2 = (uint32_t)y; const uint32_t k1 = (uint32_t)(ke >> 32), k2 = (uint32_t)ke;
    y1 ^= (y2 | k2); y2 ^= cam_rotl32(y1 & k1, 1);
    return ((uint64_t)y1 << 32) | y2;
}
struct CamRefKey { uint64_t kw[4], k[24], ke[6]; };
inline void cam_ref_rot(const uint64_t v[2], unsigned n, uint64_t out[2]) {          // 128-bit left rotation, one bit at a time
    uint64_t h = v[0], l = v[1];
    for (unsigned i = 0; i < n; i++) { const uint64_t c = h >> 63; h = (h << 1) | (l >> 63); l = (l << 1) | c; }
    out[0] = h; out[1] = l;
}
inline void cam_ref_expand(const uint8_t key[32], CamRefKey &o) {
    const uint64_t S[6] = {0xA09E667F3BCC908Bull, 0xB67AE8584CAA73B2ull, 0xC6EF372FE94F82BEull, 0x54FF53A5F1D36F1Cull, 0x10E527FADE682D1Dull, 0xB05688C2B3E6C1FDull};
    uint64_t KL[2], KR[2], KA[2], KB[2];
    for (int h = 0; h < 2; h++) { KL[h] = KR[h] = 0; for (int b = 0; b < 8; b++) { KL[h] = (KL[h] << 8) | key[8 * h + b]; KR[h] = (KR[h] << 8) | key[16 + 8 * h + b]; } }
    uint64_t d1 = KL[0] ^ KR[0], d2 = KL[1] ^ KR[1];
    d2 ^= cam_ref_f(d1, S[0]); d1 ^= cam_ref_f(d2, S[1]);
    d1 ^= KL[0]; d2 ^= KL[1];
    d2 ^= cam_ref_f(d1, S[2]); d1 ^= cam_ref_f(d2, S[3]);
    KA[0] = d1; KA[1] = d2;
    d1 = KA[0] ^ KR[0]; d2 = KA[1] ^ KR[1];
    d2 ^= cam_ref_f(d1, S[4]); d1 ^= cam_ref_f(d2, S[5]);
    KB[0] = d1; KB[1] = d2;
    cam_ref_rot(KL, 0, o.kw);     cam_ref_rot(KB, 0, o.k);        cam_ref_rot(KR, 15, o.k + 2);   cam_ref_rot(KA, 15, o.k + 4);
    cam_ref_rot(KR, 30, o.ke);    cam_ref_rot(KB, 30, o.k + 6);   cam_ref_rot(KL, 45, o.k + 8);   cam_ref_rot(KA, 45, o.k + 10);
    cam_ref_rot(KL, 60, o.ke + 2); cam_ref_rot(KR, 60, o.k + 12); cam_ref_rot(KB, 60, o.k + 14);  cam_ref_rot(KL, 77, o.k + 16);
    cam_ref_rot(KA, 77, o.ke + 4); cam_ref_rot(KR, 94, o.k + 18); cam_ref_rot(KA, 94, o.k + 20);  cam_ref_rot(KL, 111, o.k + 22);
    cam_ref_rot(KB, 111, o.kw + 2);
}
inline void cam_ref_dec_key(const CamRefKey &e, CamRefKey &d) {
    d.kw[0] = e.kw[2]; d.kw[1] = e.kw[3]; d.kw[2] = e.kw[0]; d.kw[3] = e.kw[1];
    for (int i = 0; i < 24; i++) d.k[i] = e.k[23 - i];
    for (int i = 0; i < 6; i++) d.ke[i] = e.ke[5 - i];
}
inline void cam_ref_block(const CamRefKey &k, const uint8_t in[16], uint8_t out[16]) {
    uint64_t d1 = 0, d2 = 0;
    for (int b = 0; b < 8; b++) { d1 = (d1 << 8) | in[b]; d2 = (d2 << 8) | in[8 + b]; }
    d1 ^= k.kw[0]; d2 ^= k.kw[1];
    for (int r = 0; r < 24; r++) {
        if (r == 6 || r == 12 || r == 18) { const int j = r / 6 - 1; d1 = cam_ref_fl(d1, k.ke[2 * j]); d2 = cam_ref_flinv(d2, k.ke[2 * j + 1]); }
        if (r % 2 == 0) d2 ^= cam_ref_f(d1, k.k[r]); else d1 ^= cam_ref_f(d2, k.k[r]);
    }
    d2 ^= k.kw[2]; d1 ^= k.kw[3];
    for (int b = 0; b < 8; b++) { out[b] = (uint8_t)(d2 >> (56 - 8 * b)); out[8 + b] = (uint8_t)(d1 >> (56 - 8 * b)); }
}

// ---- the modes on the host (the CPU model the device tests lean on; the host code itself needs single blocks only)
// CTR (Ctr128BE): bytes [pos, pos + n) of the stream whose IV is iv, in place
inline void cam_ctr_host(const CamKey &k, const uint8_t iv[16], uint64_t pos, uint8_t *buf, size_t n) {
    uint64_t hi = 0, lo = 0;
    for (int b = 0; b < 8; b++) { hi = (hi << 8) | iv[b]; lo = (lo << 8) | iv[8 + b]; }
    size_t done = 0;
    while (done < n) {
        const uint64_t blk = (pos + done) >> 4, l = lo + blk, h = hi + (l < lo ? 1u : 0u);
        uint8_t ctr[16], ks[16];
        for (int b = 0; b < 8; b++) { ctr[b] = (uint8_t)(h >> (56 - 8 * b)); ctr[8 + b] = (uint8_t)(l >> (56 - 8 * b)); }
        cam_block_host(k, ctr, ks);
        for (size_t b = (pos + done) & 15; b < 16 && done < n; b++, done++) buf[done] ^= ks[b];
    }
}
// CBC with PKCS#7: n plaintext bytes of `in` become (n / 16 + 1) * 16 bytes of `out` (which may be `in`)
inline void cam_cbc_enc_host(const CamKey &k, const uint8_t iv[16], const uint8_t *in, size_t n, uint8_t *out) {
    uint8_t c[16];
    for (int b = 0; b < 16; b++) c[b] = iv[b];
    const size_t nb = n / 16 + 1;
    for (size_t j = 0; j < nb; j++) {
        const size_t have = j + 1 < nb ? 16 : n - 16 * j;
        for (size_t b = 0; b < 16; b++) c[b] ^= b < have ? in[16 * j + b] : (uint8_t)(16 - have);
        cam_block_host(k, c, c);
        for (int b = 0; b < 16; b++) out[16 * j + b] = c[b];
    }
}
// ... and back: n ciphertext bytes (a positive multiple of 16) under the decrypt-order schedule `dk`; returns the plaintext length or -1 (bad padding)
inline long cam_cbc_dec_host(const CamKey &dk, const uint8_t iv[16], const uint8_t *in, size_t n, uint8_t *out) {
    if (n == 0 || (n & 15)) return -1;
    uint8_t prev[16], cur[16], p[16];
    for (int b = 0; b < 16; b++) prev[b] = iv[b];
    for (size_t j = 0; j < n / 16; j++) {
        for (int b = 0; b < 16; b++) cur[b] = in[16 * j + b];
        cam_block_host(dk, cur, p);
        for (int b = 0; b < 16; b++) { out[16 * j + b] = (uint8_t)(p[b] ^ prev[b]); prev[b] = cur[b]; }
    }
    const uint8_t pad = out[n - 1];
    if (pad < 1 || pad > 16) return -1;
    for (size_t b = 0; b < pad; b++) if (out[n - 1 - b] != pad) return -1;
    return (long)(n - pad);
}
