// kdf_core.h -- the password hashes of the PHSF chunk in one place, for the host code (pna_archive.cpp, pna_kdf.cpp) and the kernels of k_kdf.hip:
// BLAKE2b (RFC 7693, unkeyed) and Argon2's H', Argon2's compression G, the reference-index arithmetic of RFC 9106 3.4 with the address-block generator of
// the data-independent slices, a fill of one segment of one Argon2 lane over caller-provided memory (Argon2d / i / id, version 0x13, no secret, no
// associated data), and SHA-256, HMAC-SHA256 and the one-block PBKDF2 chain (RFC 8018, dkLen = 32).  Builds with g++ alone (tests/kdf_core); no HIP
// header is needed.
//
// Replaces hash::argon2_with_salt and hash::pbkdf2_with_salt of the reference (lib/src/hash.rs:6-45; argon2 0.5, pbkdf2 0.12).
//
// What runs where: the kernels take kdf_mix, kdf_argon_ref, kdf_argon_addr_input and kdf_sha256_block / kdf_pbkdf2_chain from here; G itself is written
// again in k_kdf.hip, spread over 32 wave lanes, and is held against kdf_g by the tests.  BLAKE2b, H', the seed blocks and HMAC's key set-up stay host work.
#pragma once
#include <stdint.h>
#include <stddef.h>
#include <string.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define KDF_HD __host__ __device__ __forceinline__
#else
#define KDF_HD inline
#endif

KDF_HD uint64_t kdf_ror64(uint64_t x, int n) { return (x >> n) | (x << (64 - n)); }
KDF_HD uint32_t kdf_ror32(uint32_t x, int n) { return (x >> n) | (x << (32 - n)); }

// ---------------------------------------------------------------------------------------------------------
// BLAKE2b
struct KdfBlake2b { uint64_t h[8], t; uint8_t buf[128]; size_t fill, outlen; };
KDF_HD uint64_t kdf_b2b_iv(int i) {
    constexpr uint64_t IV[8] = {0x6A09E667F3BCC908ull, 0xBB67AE8584CAA73Bull, 0x3C6EF372FE94F82Bull, 0xA54FF53A5F1D36F1ull,
                                0x510E527FADE682D1ull, 0x9B05688C2B3E6C1Full, 0x1F83D9ABFB41BD6Bull, 0x5BE0CD19137E2179ull};
    return IV[i];
}
KDF_HD void kdf_b2b_init(KdfBlake2b &s, size_t outlen) {
    for (int i = 0; i < 8; i++) s.h[i] = kdf_b2b_iv(i);
    s.h[0] ^= 0x01010000ull ^ (uint64_t)outlen; s.t = 0; s.fill = 0; s.outlen = outlen;
}
KDF_HD void kdf_b2b_compress(KdfBlake2b &s, const uint8_t *blk, bool last) {
    constexpr uint8_t SG[10][16] = {
        {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15}, {14, 10, 4, 8, 9, 15, 13, 6, 1, 12, 0, 2, 11, 7, 5, 3},
        {11, 8, 12, 0, 5, 2, 15, 13, 10, 14, 3, 6, 7, 1, 9, 4}, {7, 9, 3, 1, 13, 12, 11, 14, 2, 6, 5, 10, 4, 0, 15, 8},
        {9, 0, 5, 7, 2, 4, 10, 15, 14, 1, 11, 12, 6, 8, 3, 13}, {2, 12, 6, 10, 0, 11, 8, 3, 4, 13, 7, 5, 15, 14, 1, 9},
        {12, 5, 1, 15, 14, 13, 4, 10, 0, 7, 6, 3, 9, 2, 8, 11}, {13, 11, 7, 14, 12, 1, 3, 9, 5, 0, 15, 4, 8, 6, 2, 10},
        {6, 15, 14, 9, 11, 3, 0, 8, 12, 2, 13, 7, 1, 4, 10, 5}, {10, 2, 8, 4, 7, 6, 1, 5, 15, 11, 9, 14, 3, 12, 13, 0}};
    uint64_t m[16], v[16];
    for (int i = 0; i < 16; i++) { m[i] = 0; for (int b = 0; b < 8; b++) m[i] |= (uint64_t)blk[8 * i + b] << (8 * b); }
    for (int i = 0; i < 8; i++) { v[i] = s.h[i]; v[i + 8] = kdf_b2b_iv(i); }
    v[12] ^= s.t; if (last) v[14] = ~v[14];
#define KDF_B2B_G(a, b, c, d, x, y) \
    { v[a] += v[b] + (x); v[d] = kdf_ror64(v[d] ^ v[a], 32); v[c] += v[d]; v[b] = kdf_ror64(v[b] ^ v[c], 24); \
      v[a] += v[b] + (y); v[d] = kdf_ror64(v[d] ^ v[a], 16); v[c] += v[d]; v[b] = kdf_ror64(v[b] ^ v[c], 63); }
    for (int r = 0; r < 12; r++) {
        const uint8_t *g = SG[r % 10];
        KDF_B2B_G(0, 4, 8, 12, m[g[0]], m[g[1]]) KDF_B2B_G(1, 5, 9, 13, m[g[2]], m[g[3]]) KDF_B2B_G(2, 6, 10, 14, m[g[4]], m[g[5]]) KDF_B2B_G(3, 7, 11, 15, m[g[6]], m[g[7]])
        KDF_B2B_G(0, 5, 10, 15, m[g[8]], m[g[9]]) KDF_B2B_G(1, 6, 11, 12, m[g[10]], m[g[11]]) KDF_B2B_G(2, 7, 8, 13, m[g[12]], m[g[13]]) KDF_B2B_G(3, 4, 9, 14, m[g[14]], m[g[15]])
    }
#undef KDF_B2B_G
    for (int i = 0; i < 8; i++) s.h[i] ^= v[i] ^ v[i + 8];
}
KDF_HD void kdf_b2b_update(KdfBlake2b &s, const void *d, size_t n) {
    const uint8_t *p = (const uint8_t *)d;
    while (n) {
        if (s.fill == 128) { s.t += 128; kdf_b2b_compress(s, s.buf, false); s.fill = 0; }      // (a full buffer waits: the last block is compressed by final)
        const size_t k = n < 128 - s.fill ? n : 128 - s.fill;
        memcpy(s.buf + s.fill, p, k); s.fill += k; p += k; n -= k;
    }
}
KDF_HD void kdf_b2b_u32(KdfBlake2b &s, uint32_t v) { const uint8_t b[4] = {(uint8_t)v, (uint8_t)(v >> 8), (uint8_t)(v >> 16), (uint8_t)(v >> 24)}; kdf_b2b_update(s, b, 4); }
KDF_HD void kdf_b2b_final(KdfBlake2b &s, uint8_t *out) {      // out: outlen bytes
    s.t += s.fill; memset(s.buf + s.fill, 0, 128 - s.fill); kdf_b2b_compress(s, s.buf, true);
    for (size_t i = 0; i < s.outlen; i++) out[i] = (uint8_t)(s.h[i >> 3] >> (8 * (i & 7)));
}
// H' of RFC 9106 3.3: T bytes from 64-byte BLAKE2b digests, 32 bytes kept of each but the last
KDF_HD void kdf_hprime(const uint8_t *in, size_t n, uint8_t *out, uint32_t T) {
    KdfBlake2b b;
    if (T <= 64) { kdf_b2b_init(b, T); kdf_b2b_u32(b, T); kdf_b2b_update(b, in, n); kdf_b2b_final(b, out); return; }
    uint8_t v[64], nx[64];
    kdf_b2b_init(b, 64); kdf_b2b_u32(b, T); kdf_b2b_update(b, in, n); kdf_b2b_final(b, v);
    size_t done = 0;
    for (;;) {
        memcpy(out + done, v, 32); done += 32;
        if (T - done <= 64) break;
        kdf_b2b_init(b, 64); kdf_b2b_update(b, v, 64); kdf_b2b_final(b, nx); memcpy(v, nx, 64);
    }
    kdf_b2b_init(b, T - done); kdf_b2b_update(b, v, 64); kdf_b2b_final(b, out + done);
}

// ---------------------------------------------------------------------------------------------------------
// Argon2's compression.  A block is 128 64-bit words, read as 8 rows of 16; P is the BLAKE2b round with a + b replaced by kdf_mix.
KDF_HD uint64_t kdf_mix(uint64_t x, uint64_t y) { return x + y + 2 * (uint64_t)(uint32_t)x * (uint64_t)(uint32_t)y; }
KDF_HD void kdf_quarter(uint64_t &a, uint64_t &b, uint64_t &c, uint64_t &d) {
    a = kdf_mix(a, b); d = kdf_ror64(d ^ a, 32); c = kdf_mix(c, d); b = kdf_ror64(b ^ c, 24);
    a = kdf_mix(a, b); d = kdf_ror64(d ^ a, 16); c = kdf_mix(c, d); b = kdf_ror64(b ^ c, 63);
}
// P over the 16 words v[base + step_hi * (k / 2) + (k & 1)] -- rows: base = 16 row, step_hi = 2; columns: base = 2 col, step_hi = 16
KDF_HD void kdf_perm(uint64_t *v, int base, int step_hi) {
#define KDF_V(k) v[base + step_hi * ((k) >> 1) + ((k) & 1)]
#define KDF_Q(a, b, c, d) kdf_quarter(KDF_V(a), KDF_V(b), KDF_V(c), KDF_V(d));
    KDF_Q(0, 4, 8, 12) KDF_Q(1, 5, 9, 13) KDF_Q(2, 6, 10, 14) KDF_Q(3, 7, 11, 15) KDF_Q(0, 5, 10, 15) KDF_Q(1, 6, 11, 12) KDF_Q(2, 7, 8, 13) KDF_Q(3, 4, 9, 14)
#undef KDF_Q
#undef KDF_V
}
// next = P(prev ^ ref) ^ prev ^ ref (^ the old next from the second pass on), P on the rows, then on the columns
KDF_HD void kdf_g(const uint64_t *prev, const uint64_t *ref, uint64_t *next, bool xor_old) {
    uint64_t r[128], keep[128];
    for (int i = 0; i < 128; i++) { r[i] = prev[i] ^ ref[i]; keep[i] = xor_old ? r[i] ^ next[i] : r[i]; }
    for (int row = 0; row < 8; row++) kdf_perm(r, 16 * row, 2);
    for (int col = 0; col < 8; col++) kdf_perm(r, 2 * col, 16);
    for (int i = 0; i < 128; i++) next[i] = r[i] ^ keep[i];
}

// The geometry of a fill: m' = 4 p floor(m / 4 p) blocks in p lanes of lane_len = 4 seg columns
struct KdfArgonGeom { uint32_t kind, t_cost, lanes, blocks, lane_len, seg; };
KDF_HD KdfArgonGeom kdf_argon_geom(int kind, uint32_t t_cost, uint32_t m_cost_kib, uint32_t lanes) {
    KdfArgonGeom g; g.kind = (uint32_t)kind; g.t_cost = t_cost; g.lanes = lanes;
    g.blocks = 4 * lanes * (m_cost_kib / (4 * lanes)); g.lane_len = g.blocks / lanes; g.seg = g.lane_len / 4;
    return g;
}
// data-independent addressing: Argon2i everywhere, Argon2id in the first two slices of the first pass
KDF_HD bool kdf_argon_indep(const KdfArgonGeom &g, uint32_t pass, uint32_t slice) { return g.kind == 1 || (g.kind == 2 && pass == 0 && slice < 2); }
// the first column a segment computes: the two seed blocks stand in front of pass 0, slice 0
KDF_HD uint32_t kdf_argon_first(uint32_t pass, uint32_t slice) { return pass == 0 && slice == 0 ? 2u : 0u; }
// RFC 9106 3.4: the block that column i of (pass, slice, lane) refers to, from the 64 pseudo-random bits J1 | J2 << 32
KDF_HD void kdf_argon_ref(const KdfArgonGeom &g, uint32_t pass, uint32_t slice, uint32_t lane, uint32_t i, uint64_t rnd, uint32_t &ref_lane, uint32_t &ref_col) {
    uint32_t rl = (uint32_t)(rnd >> 32) % g.lanes;
    if (pass == 0 && slice == 0) rl = lane;
    const bool same = rl == lane;
    uint64_t area;                                              // the number of blocks that may be referenced (3.4.1.1 / 3.4.2)
    if (pass == 0) area = slice == 0 ? (uint64_t)i - 1 : (same ? (uint64_t)slice * g.seg + i - 1 : (uint64_t)slice * g.seg - (i == 0 ? 1 : 0));
    else area = same ? (uint64_t)g.lane_len - g.seg + i - 1 : (uint64_t)g.lane_len - g.seg - (i == 0 ? 1 : 0);
    uint64_t x = rnd & 0xFFFFFFFFull; x = (x * x) >> 32;
    const uint64_t rel = area - 1 - ((area * x) >> 32);
    const uint64_t start = (pass == 0 || slice == 3) ? 0 : (uint64_t)(slice + 1) * g.seg;
    const uint64_t at = start + rel;                            // start < lane_len and rel < area <= lane_len: one conditional subtraction is the modulo
    ref_lane = rl; ref_col = (uint32_t)(at >= g.lane_len ? at - g.lane_len : at);
}
// the words 0 .. 6 of the address generator's input block (3.4.1.2); the rest of it is zero.  counter: 1 for a segment's first 128 columns, 2 for the next, ...
KDF_HD uint64_t kdf_argon_addr_input(const KdfArgonGeom &g, uint32_t pass, uint32_t slice, uint32_t lane, uint32_t counter, int word) {
    switch (word) {
        case 0: return pass; case 1: return lane; case 2: return slice; case 3: return g.blocks; case 4: return g.t_cost; case 5: return g.kind; case 6: return counter;
        default: return 0;
    }
}
KDF_HD void kdf_argon_addr_block(const KdfArgonGeom &g, uint32_t pass, uint32_t slice, uint32_t lane, uint32_t counter, uint64_t *addr) {
    uint64_t zero[128], in[128], t[128];
    for (int i = 0; i < 128; i++) { zero[i] = 0; in[i] = kdf_argon_addr_input(g, pass, slice, lane, counter, i); }
    kdf_g(zero, in, t, false); kdf_g(zero, t, addr, false);
}
// One segment of one lane.  mem: g.blocks blocks of 128 words, lane l's column c at (l * lane_len + c) * 128; every other lane's earlier slices are complete.
KDF_HD void kdf_argon_fill_segment(uint64_t *mem, const KdfArgonGeom &g, uint32_t pass, uint32_t slice, uint32_t lane) {
    const bool indep = kdf_argon_indep(g, pass, slice);
    uint64_t addr[128];
    const uint32_t first = kdf_argon_first(pass, slice);
    if (indep && first) kdf_argon_addr_block(g, pass, slice, lane, 1, addr);
    for (uint32_t i = first; i < g.seg; i++) {
        const uint32_t col = slice * g.seg + i, pcol = col ? col - 1 : g.lane_len - 1;
        uint64_t *prev = mem + ((size_t)lane * g.lane_len + pcol) * 128;
        uint64_t rnd;
        if (indep) { if (i % 128 == 0) kdf_argon_addr_block(g, pass, slice, lane, i / 128 + 1, addr); rnd = addr[i % 128]; } else rnd = prev[0];
        uint32_t rl, rc;
        kdf_argon_ref(g, pass, slice, lane, i, rnd, rl, rc);
        kdf_g(prev, mem + ((size_t)rl * g.lane_len + rc) * 128, mem + ((size_t)lane * g.lane_len + col) * 128, pass != 0);
    }
}
// H0 (3.2 step 1) with room for the two counters that the seed blocks append: h0[0 .. 63] is the digest
KDF_HD void kdf_argon_h0(const KdfArgonGeom &g, uint32_t m_cost_kib, uint32_t tag_len, const void *password, size_t password_len, const void *salt, size_t salt_len, uint8_t h0[72]) {
    KdfBlake2b b; kdf_b2b_init(b, 64);
    kdf_b2b_u32(b, g.lanes); kdf_b2b_u32(b, tag_len); kdf_b2b_u32(b, m_cost_kib); kdf_b2b_u32(b, g.t_cost); kdf_b2b_u32(b, 0x13); kdf_b2b_u32(b, g.kind);
    kdf_b2b_u32(b, (uint32_t)password_len); kdf_b2b_update(b, password, password_len);
    kdf_b2b_u32(b, (uint32_t)salt_len); kdf_b2b_update(b, salt, salt_len);
    kdf_b2b_u32(b, 0); kdf_b2b_u32(b, 0);
    kdf_b2b_final(b, h0);
    memset(h0 + 64, 0, 8);
}
// B[lane][j] = H'(H0 || LE32(j) || LE32(lane)), j = 0, 1
KDF_HD void kdf_argon_seed(uint8_t h0[72], uint32_t lane, uint32_t j, uint64_t *blk) {
    uint8_t raw[1024];
    for (int k = 0; k < 4; k++) { h0[64 + k] = (uint8_t)(j >> (8 * k)); h0[68 + k] = (uint8_t)(lane >> (8 * k)); }
    kdf_hprime(h0, 72, raw, 1024);
    for (int i = 0; i < 128; i++) { blk[i] = 0; for (int k = 0; k < 8; k++) blk[i] |= (uint64_t)raw[8 * i + k] << (8 * k); }
}
// the tag: H' of the XOR of the lanes' last blocks (fin: that XOR)
KDF_HD void kdf_argon_tag(const uint64_t *fin, uint8_t *tag, uint32_t tag_len) {
    uint8_t raw[1024];
    for (int i = 0; i < 128; i++) for (int k = 0; k < 8; k++) raw[8 * i + k] = (uint8_t)(fin[i] >> (8 * k));
    kdf_hprime(raw, 1024, tag, tag_len);
}

// ---------------------------------------------------------------------------------------------------------
// SHA-256 (FIPS 180-4), HMAC (RFC 2104), PBKDF2's chain (RFC 8018 5.2)
KDF_HD void kdf_sha256_iv(uint32_t h[8]) {
    h[0] = 0x6a09e667u; h[1] = 0xbb67ae85u; h[2] = 0x3c6ef372u; h[3] = 0xa54ff53au; h[4] = 0x510e527fu; h[5] = 0x9b05688cu; h[6] = 0x1f83d9abu; h[7] = 0x5be0cd19u;
}
// one compression: h += f(h, w), w = the block's 16 big-endian words (destroyed)
KDF_HD void kdf_sha256_block(uint32_t h[8], uint32_t w[16]) {
    constexpr uint32_t K[64] = {
        0x428a2f98u, 0x71374491u, 0xb5c0fbcfu, 0xe9b5dba5u, 0x3956c25bu, 0x59f111f1u, 0x923f82a4u, 0xab1c5ed5u, 0xd807aa98u, 0x12835b01u, 0x243185beu, 0x550c7dc3u,
        0x72be5d74u, 0x80deb1feu, 0x9bdc06a7u, 0xc19bf174u, 0xe49b69c1u, 0xefbe4786u, 0x0fc19dc6u, 0x240ca1ccu, 0x2de92c6fu, 0x4a7484aau, 0x5cb0a9dcu, 0x76f988dau,
        0x983e5152u, 0xa831c66du, 0xb00327c8u, 0xbf597fc7u, 0xc6e00bf3u, 0xd5a79147u, 0x06ca6351u, 0x14292967u, 0x27b70a85u, 0x2e1b2138u, 0x4d2c6dfcu, 0x53380d13u,
        0x650a7354u, 0x766a0abbu, 0x81c2c92eu, 0x92722c85u, 0xa2bfe8a1u, 0xa81a664bu, 0xc24b8b70u, 0xc76c51a3u, 0xd192e819u, 0xd6990624u, 0xf40e3585u, 0x106aa070u,
        0x19a4c116u, 0x1e376c08u, 0x2748774cu, 0x34b0bcb5u, 0x391c0cb3u, 0x4ed8aa4au, 0x5b9cca4fu, 0x682e6ff3u, 0x748f82eeu, 0x78a5636fu, 0x84c87814u, 0x8cc70208u,
        0x90befffau, 0xa4506cebu, 0xbef9a3f7u, 0xc67178f2u};
    uint32_t a = h[0], b = h[1], c = h[2], d = h[3], e = h[4], f = h[5], g = h[6], hh = h[7];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int i = 0; i < 64; i++) {
        if (i >= 16) {
            const uint32_t w15 = w[(i + 1) & 15], w2 = w[(i + 14) & 15];
            w[i & 15] += (kdf_ror32(w15, 7) ^ kdf_ror32(w15, 18) ^ (w15 >> 3)) + w[(i + 9) & 15] + (kdf_ror32(w2, 17) ^ kdf_ror32(w2, 19) ^ (w2 >> 10));
        }
        const uint32_t t1 = hh + (kdf_ror32(e, 6) ^ kdf_ror32(e, 11) ^ kdf_ror32(e, 25)) + ((e & f) ^ (~e & g)) + K[i] + w[i & 15];
        const uint32_t t2 = (kdf_ror32(a, 2) ^ kdf_ror32(a, 13) ^ kdf_ror32(a, 22)) + ((a & b) ^ (a & c) ^ (b & c));
        hh = g; g = f; f = e; e = d + t1; d = c; c = b; b = a; a = t1 + t2;
    }
    h[0] += a; h[1] += b; h[2] += c; h[3] += d; h[4] += e; h[5] += f; h[6] += g; h[7] += hh;
}
struct KdfSha256 {
    uint32_t h[8]; uint64_t len; uint8_t buf[64]; size_t fill;
    void init() { kdf_sha256_iv(h); len = 0; fill = 0; }
    void block(const uint8_t *p) {
        uint32_t w[16];
        for (int i = 0; i < 16; i++) w[i] = ((uint32_t)p[4 * i] << 24) | ((uint32_t)p[4 * i + 1] << 16) | ((uint32_t)p[4 * i + 2] << 8) | p[4 * i + 3];
        kdf_sha256_block(h, w);
    }
    void update(const void *d, size_t n) {
        const uint8_t *p = (const uint8_t *)d; len += n;
        while (n) { const size_t k = n < 64 - fill ? n : 64 - fill; memcpy(buf + fill, p, k); fill += k; p += k; n -= k; if (fill == 64) { block(buf); fill = 0; } }
    }
    void final_words(uint32_t out[8]) {
        const uint64_t bits = len * 8; uint8_t pad[72] = {0x80}; const size_t padn = (fill < 56 ? 56 : 120) - fill;
        update(pad, padn);
        uint8_t lb[8]; for (int i = 0; i < 8; i++) lb[i] = (uint8_t)(bits >> (56 - 8 * i));
        update(lb, 8);
        for (int i = 0; i < 8; i++) out[i] = h[i];
    }
    void final(uint8_t out[32]) {
        uint32_t w[8]; final_words(w);
        for (int i = 0; i < 8; i++) { out[4 * i] = (uint8_t)(w[i] >> 24); out[4 * i + 1] = (uint8_t)(w[i] >> 16); out[4 * i + 2] = (uint8_t)(w[i] >> 8); out[4 * i + 3] = (uint8_t)w[i]; }
    }
};
struct KdfHmac {                                               // the inner / outer states after the key pads
    KdfSha256 in0, out0;
    void key(const uint8_t *k, size_t n) {
        uint8_t kb[64] = {0}, pad[64];
        if (n > 64) { KdfSha256 t; t.init(); t.update(k, n); t.final(kb); } else if (n) memcpy(kb, k, n);
        for (int i = 0; i < 64; i++) pad[i] = kb[i] ^ 0x36;
        in0.init(); in0.update(pad, 64);
        for (int i = 0; i < 64; i++) pad[i] = kb[i] ^ 0x5c;
        out0.init(); out0.update(pad, 64);
    }
    void mac(const void *a, size_t an, const void *b, size_t bn, uint8_t out[32]) const {
        KdfSha256 s = in0; if (an) s.update(a, an); if (bn) s.update(b, bn);
        uint8_t inner[32]; s.final(inner);
        KdfSha256 o = out0; o.update(inner, 32); o.final(out);
    }
};
// HMAC of a 32-byte message given as 8 words, from the two pad states: two compressions
KDF_HD void kdf_hmac32(const uint32_t istate[8], const uint32_t ostate[8], uint32_t u[8]) {
    uint32_t w[16], h[8];
    for (int i = 0; i < 8; i++) { w[i] = u[i]; h[i] = istate[i]; }
    w[8] = 0x80000000u; for (int i = 9; i < 15; i++) w[i] = 0; w[15] = (64 + 32) * 8;
    kdf_sha256_block(h, w);
    for (int i = 0; i < 8; i++) { w[i] = h[i]; h[i] = ostate[i]; }
    w[8] = 0x80000000u; for (int i = 9; i < 15; i++) w[i] = 0; w[15] = (64 + 32) * 8;
    kdf_sha256_block(h, w);
    for (int i = 0; i < 8; i++) u[i] = h[i];
}
// T = U_1 ^ U_2 ^ ... ^ U_rounds, U_k = HMAC(U_(k-1)); u1 = U_1 = HMAC(salt || INT(block))
KDF_HD void kdf_pbkdf2_chain(const uint32_t istate[8], const uint32_t ostate[8], const uint32_t u1[8], uint32_t rounds, uint32_t t[8]) {
    uint32_t u[8];
    for (int i = 0; i < 8; i++) { u[i] = u1[i]; t[i] = u1[i]; }
    for (uint32_t r = 1; r < rounds; r++) { kdf_hmac32(istate, ostate, u); for (int i = 0; i < 8; i++) t[i] ^= u[i]; }
}
// what a PBKDF2 job's chain starts from: the pad states of the password and U_1 of block 1
struct KdfPbkdf2Start { uint32_t istate[8], ostate[8], u1[8]; };
inline void kdf_pbkdf2_start(const void *password, size_t password_len, const void *salt, size_t salt_len, uint32_t block, KdfPbkdf2Start &s) {
    KdfHmac hm; hm.key((const uint8_t *)password, password_len);
    const uint8_t be[4] = {(uint8_t)(block >> 24), (uint8_t)(block >> 16), (uint8_t)(block >> 8), (uint8_t)block};
    uint8_t u[32]; hm.mac(salt, salt_len, be, 4, u);
    for (int i = 0; i < 8; i++) { s.istate[i] = hm.in0.h[i]; s.ostate[i] = hm.out0.h[i]; s.u1[i] = ((uint32_t)u[4 * i] << 24) | ((uint32_t)u[4 * i + 1] << 16) | ((uint32_t)u[4 * i + 2] << 8) | u[4 * i + 3]; }
}
inline void kdf_words_be(const uint32_t w[8], uint8_t out[32]) {
    for (int i = 0; i < 8; i++) { out[4 * i] = (uint8_t)(w[i] >> 24); out[4 * i + 1] = (uint8_t)(w[i] >> 16); out[4 * i + 2] = (uint8_t)(w[i] >> 8); out[4 * i + 3] = (uint8_t)w[i]; }
}

// ---------------------------------------------------------------------------------------------------------
// What the host hands the kernels of k_kdf.hip
struct KdfArgonJob { KdfArgonGeom g; uint32_t lane0, pad; uint64_t mem_off; };      // lane0: the job's first lane in the seed / last-block buffers; mem_off: its block 0 in the block memory, in blocks
struct KdfPbkdf2Job { KdfPbkdf2Start s; uint32_t rounds; };
