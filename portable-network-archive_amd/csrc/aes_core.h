// aes_core.h -- AES-256 (FIPS-197) in one place, for the host code and the kernels of k_cipher.hip: the S-box, the round tables, the key schedule, the
// schedule of the equivalent inverse cipher (FIPS-197 5.3.5), and the block function written once for both directions.  The counterpart of
// camellia_core.h: builds with g++ alone (tests/aes_core); no HIP header is needed.
//
// The table accessor is a parameter (tab(i, x) = entry x of table i): host code reads a plain array, a kernel its LDS layout.  Tables 0 .. 3 are the
// round tables (Te or Td); table 4, read by the inverse cipher only, is the inverse S-box -- AesDecTabs holds it behind Td, so one flat accessor of
// 1 280 words serves it.  The types live in namespace pna with the other kernel-argument types; the functions are global, as camellia_core.h's are.
#pragma once
#include <stdint.h>
#include <stddef.h>
#include <string.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define AES_HD __host__ __device__ __forceinline__
#else
#define AES_HD inline
#endif

namespace pna {

struct AesTabs { uint32_t Te[4][256]; };   // Te[0][x] = bytes (2S, S, S, 3S) of S = sbox[x], little-endian; Te[k] = Te[0] rotated left by 8k bits
struct AesKey  { uint32_t rk[60]; };       // AES-256 round keys, word 4r + c = column c of round r, little-endian; 240 bytes: a kernel argument (scalar registers)
struct AesDecTabs { uint32_t Td[4][256]; uint32_t Sd[256]; };   // equivalent inverse cipher: Td[0][x] = bytes (14, 9, 13, 11) x Si[x]; Sd = inverse S-box
} // namespace pna
using pna::AesTabs; using pna::AesKey; using pna::AesDecTabs;

struct AesHostTab {                        // the accessor of host code, over an AesTabs or an AesDecTabs
    const uint32_t *t;
    uint32_t operator()(uint32_t i, uint32_t x) const { return t[(i << 8) + x]; }
};

// The 14 rounds over the state columns s0 .. s3 (little-endian words, byte 0 = row 0).  Column n of a round takes row j from column n + j (forward:
// ShiftRows) or n - j (inverse: InvShiftRows); the last round is (Inv)SubBytes + (Inv)ShiftRows only, its S-box byte 1 of Te0[x] forward, table 4 inverse.
template <bool INV, class Tab>
AES_HD void aes_rounds(const Tab &tab, const AesKey &k, uint32_t &s0, uint32_t &s1, uint32_t &s2, uint32_t &s3) {
    constexpr int J1 = INV ? 3 : 1, J3 = INV ? 1 : 3;
    uint32_t s[4] = {s0 ^ k.rk[0], s1 ^ k.rk[1], s2 ^ k.rk[2], s3 ^ k.rk[3]}, t[4];
#define AES_COL(n, r) t[n] = tab(0, s[n] & 0xFF) ^ tab(1, (s[(n + J1) & 3] >> 8) & 0xFF) ^ tab(2, (s[(n + 2) & 3] >> 16) & 0xFF) ^ tab(3, s[(n + J3) & 3] >> 24) ^ k.rk[4 * (r) + n];
#define AES_ROUND(r) { AES_COL(0, r) AES_COL(1, r) AES_COL(2, r) AES_COL(3, r) s[0] = t[0]; s[1] = t[1]; s[2] = t[2]; s[3] = t[3]; }
    AES_ROUND(1) AES_ROUND(2) AES_ROUND(3) AES_ROUND(4) AES_ROUND(5) AES_ROUND(6) AES_ROUND(7)
    AES_ROUND(8) AES_ROUND(9) AES_ROUND(10) AES_ROUND(11) AES_ROUND(12) AES_ROUND(13)
#undef AES_ROUND
#undef AES_COL
#define AES_SB(v) (INV ? tab(4, (v) & 0xFF) : (tab(0, (v) & 0xFF) >> 8) & 0xFF)
#define AES_LAST(n) t[n] = (AES_SB(s[n]) | (AES_SB(s[(n + J1) & 3] >> 8) << 8) | (AES_SB(s[(n + 2) & 3] >> 16) << 16) | (AES_SB(s[(n + J3) & 3] >> 24) << 24)) ^ k.rk[56 + n];
    AES_LAST(0) AES_LAST(1) AES_LAST(2) AES_LAST(3)
#undef AES_LAST
#undef AES_SB
    s0 = t[0]; s1 = t[1]; s2 = t[2]; s3 = t[3];
}
// One block under the encryption schedule (tab: Te) / under the schedule of aes256_dec_key (tab: Td and, as table 4, Sd).  In and out: the block as
// four little-endian words, as it lies in memory.
template <class Tab>
AES_HD void aes_block(const Tab &tab, const AesKey &k, uint32_t &s0, uint32_t &s1, uint32_t &s2, uint32_t &s3) { aes_rounds<false>(tab, k, s0, s1, s2, s3); }
template <class Tab>
AES_HD void aes_block_inv(const Tab &tab, const AesKey &k, uint32_t &s0, uint32_t &s1, uint32_t &s2, uint32_t &s3) { aes_rounds<true>(tab, k, s0, s1, s2, s3); }

// ------------------------------------------------------------------ host only: the S-box, the tables, the schedules
inline uint8_t aes_xtime(uint8_t a) { return (uint8_t)((a << 1) ^ ((a & 0x80) ? 0x1B : 0)); }
inline uint8_t aes_gf_mul(uint8_t a, uint8_t b) { uint8_t r = 0; while (b) { if (b & 1) r ^= a; a = aes_xtime(a); b >>= 1; } return r; }
inline void aes_sbox(uint8_t sb[256]) {
    uint8_t p = 1, q = 1;                                      // p walks the multiplicative group of GF(2^8), q is its inverse
    do {
        p = (uint8_t)(p ^ aes_xtime(p));
        q ^= (uint8_t)(q << 1); q ^= (uint8_t)(q << 2); q ^= (uint8_t)(q << 4); if (q & 0x80) q ^= 0x09;
        const uint8_t r1 = (uint8_t)((q << 1) | (q >> 7)), r2 = (uint8_t)((q << 2) | (q >> 6)), r3 = (uint8_t)((q << 3) | (q >> 5)), r4 = (uint8_t)((q << 4) | (q >> 4));
        sb[p] = (uint8_t)(q ^ r1 ^ r2 ^ r3 ^ r4 ^ 0x63);
    } while (p != 1);
    sb[0] = 0x63;
}
inline uint32_t aes_rotl(uint32_t w, int n) { return (w << n) | (w >> (32 - n)); }     // n = 8, 16, 24
inline void build_aes_tabs(AesTabs &t) {
    uint8_t sb[256]; aes_sbox(sb);
    for (uint32_t x = 0; x < 256; x++) {
        const uint32_t s1 = sb[x], s2 = aes_xtime((uint8_t)s1), s3 = s2 ^ s1;
        const uint32_t w = s2 | (s1 << 8) | (s1 << 16) | (s3 << 24);
        t.Te[0][x] = w; t.Te[1][x] = aes_rotl(w, 8); t.Te[2][x] = aes_rotl(w, 16); t.Te[3][x] = aes_rotl(w, 24);
    }
}
// InvMixColumns of one column
inline uint32_t aes_inv_mix(uint32_t w) {
    const uint8_t a[4] = {(uint8_t)w, (uint8_t)(w >> 8), (uint8_t)(w >> 16), (uint8_t)(w >> 24)};
    uint32_t r = 0;
    for (int j = 0; j < 4; j++) r |= (uint32_t)(uint8_t)(aes_gf_mul(a[j], 14) ^ aes_gf_mul(a[(j + 1) & 3], 11) ^ aes_gf_mul(a[(j + 2) & 3], 13) ^ aes_gf_mul(a[(j + 3) & 3], 9)) << (8 * j);
    return r;
}
// equivalent inverse cipher (FIPS-197 5.3.5): tables of InvSubBytes + InvMixColumns, round keys reversed with InvMixColumns applied to the middle ones
inline void build_aes_dec_tabs(AesDecTabs &t) {
    uint8_t sb[256]; aes_sbox(sb);
    for (uint32_t x = 0; x < 256; x++) t.Sd[sb[x]] = x;
    for (uint32_t x = 0; x < 256; x++) {
        const uint32_t w = aes_inv_mix(t.Sd[x]);
        t.Td[0][x] = w; t.Td[1][x] = aes_rotl(w, 8); t.Td[2][x] = aes_rotl(w, 16); t.Td[3][x] = aes_rotl(w, 24);
    }
}
inline const AesTabs &aes_host_tabs() { static const AesTabs T = [] { AesTabs x; build_aes_tabs(x); return x; }(); return T; }     // (thread-safe: C++11 static)
inline const AesDecTabs &aes_host_dec_tabs() { static const AesDecTabs T = [] { AesDecTabs x; build_aes_dec_tabs(x); return x; }(); return T; }
inline void aes256_expand(const uint8_t key[32], AesKey &k) {
    uint8_t sb[256]; aes_sbox(sb);
    uint8_t w[60][4]; uint8_t rc = 1;
    memcpy(w, key, 32);
    for (int i = 8; i < 60; i++) {
        uint8_t t[4]; memcpy(t, w[i - 1], 4);
        if (i % 8 == 0) { const uint8_t t0 = t[0]; t[0] = (uint8_t)(sb[t[1]] ^ rc); t[1] = sb[t[2]]; t[2] = sb[t[3]]; t[3] = sb[t0]; rc = aes_xtime(rc); }
        else if (i % 8 == 4) for (int j = 0; j < 4; j++) t[j] = sb[t[j]];
        for (int j = 0; j < 4; j++) w[i][j] = (uint8_t)(w[i - 8][j] ^ t[j]);
    }
    for (int i = 0; i < 60; i++) k.rk[i] = (uint32_t)w[i][0] | ((uint32_t)w[i][1] << 8) | ((uint32_t)w[i][2] << 16) | ((uint32_t)w[i][3] << 24);
}
inline void aes256_dec_key(const AesKey &k, AesKey &d) {
    for (int c4 = 0; c4 < 4; c4++) { d.rk[c4] = k.rk[56 + c4]; d.rk[56 + c4] = k.rk[c4]; }
    for (int r = 1; r < 14; r++) for (int c4 = 0; c4 < 4; c4++) d.rk[4 * r + c4] = aes_inv_mix(k.rk[4 * (14 - r) + c4]);
}
// one block on the host, bytes in and out (GCM: hash subkey and E(K, J0) of a segment); `inv`: k is aes256_dec_key's schedule
inline void aes256_block_host(const AesKey &k, const uint8_t in[16], uint8_t out[16], bool inv = false) {
    uint32_t s[4];
    memcpy(s, in, 16);                                         // (little-endian host, as the device)
    if (inv) aes_block_inv(AesHostTab{&aes_host_dec_tabs().Td[0][0]}, k, s[0], s[1], s[2], s[3]);
    else aes_block(AesHostTab{&aes_host_tabs().Te[0][0]}, k, s[0], s[1], s[2], s[3]);
    memcpy(out, s, 16);
}
