// aes_host.cpp -- csrc/aes_core.h on the CPU (tests/test_aes_core.py): a C interface for ctypes, and -- with -DAES_HOST_MAIN -- a stand-alone program
// that runs the schedules, both directions of the block function and CTR / CBC over them against the FIPS-197 and SP 800-38A known answers and over
// seeded random data, with heap buffers of exactly the needed sizes (built under -fsanitize=address,undefined by the Makefile).
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../../portable-network-archive_amd/csrc/aes_core.h"
using namespace pna;

extern "C" {
void aes_expand_c(const uint8_t key[32], uint32_t out[60]) { AesKey k; aes256_expand(key, k); memcpy(out, k.rk, sizeof k.rk); }
void aes_dec_key_c(const uint32_t in[60], uint32_t out[60]) { AesKey e, d; memcpy(e.rk, in, sizeof e.rk); aes256_dec_key(e, d); memcpy(out, d.rk, sizeof d.rk); }
// one block under a schedule: aes_block under the encryption schedule, or (inv) aes_block_inv under aes256_dec_key's
void aes_block_c(const uint32_t sched[60], int inv, const uint8_t in[16], uint8_t out[16]) { AesKey k; memcpy(k.rk, sched, sizeof k.rk); aes256_block_host(k, in, out, inv != 0); }
// CTR (Ctr128BE): bytes [pos, pos + n) of the stream whose IV is iv, in place -- the counter arithmetic of the kernels' ctr_body
void aes_ctr_c(const uint8_t key[32], const uint8_t iv[16], uint64_t pos, uint8_t *buf, size_t n) {
    AesKey k; aes256_expand(key, k);
    uint64_t hi = 0, lo = 0;
    for (int b = 0; b < 8; b++) { hi = (hi << 8) | iv[b]; lo = (lo << 8) | iv[8 + b]; }
    for (size_t done = 0; done < n;) {
        const uint64_t l = lo + ((pos + done) >> 4), h = hi + (l < lo ? 1u : 0u);
        uint8_t ctr[16], ks[16];
        for (int b = 0; b < 8; b++) { ctr[b] = (uint8_t)(h >> (56 - 8 * b)); ctr[8 + b] = (uint8_t)(l >> (56 - 8 * b)); }
        aes256_block_host(k, ctr, ks);
        for (size_t b = (pos + done) & 15; b < 16 && done < n; b++, done++) buf[done] ^= ks[b];
    }
}
// CBC over whole blocks, no padding (SP 800-38A's vectors have none; the padding is the mode bodies', checked on the device)
void aes_cbc_c(const uint8_t key[32], const uint8_t iv[16], int decrypt, const uint8_t *in, size_t nblocks, uint8_t *out) {
    AesKey e, d; aes256_expand(key, e); aes256_dec_key(e, d);
    uint8_t prev[16], cur[16], x[16];
    memcpy(prev, iv, 16);
    for (size_t j = 0; j < nblocks; j++) {
        memcpy(cur, in + 16 * j, 16);
        if (decrypt) { aes256_block_host(d, cur, x, true); for (int b = 0; b < 16; b++) out[16 * j + b] = (uint8_t)(x[b] ^ prev[b]); memcpy(prev, cur, 16); }
        else { for (int b = 0; b < 16; b++) x[b] = (uint8_t)(cur[b] ^ prev[b]); aes256_block_host(e, x, prev); memcpy(out + 16 * j, prev, 16); }
    }
}
}

#ifdef AES_HOST_MAIN
struct Bytes {                             // a heap buffer of exactly n bytes (at least one is allocated, none beyond n is ever touched)
    uint8_t *p; size_t n;
    explicit Bytes(size_t len) : p((uint8_t *)malloc(len ? len : 1)), n(len) {}
    explicit Bytes(const char *hex) : Bytes(strlen(hex) / 2) { for (size_t i = 0; i < n; i++) { unsigned v; sscanf(hex + 2 * i, "%2x", &v); p[i] = (uint8_t)v; } }
    Bytes(const Bytes &) = delete; Bytes &operator=(const Bytes &) = delete;
    ~Bytes() { free(p); }
    bool eq(const Bytes &o) const { return n == o.n && memcmp(p, o.p, n) == 0; }
};
static int checks = 0, bad = 0;
static void check(bool ok, const char *what) { checks++; if (!ok) { bad++; printf("BAD %s\n", what); } }
int main() {
    {   // FIPS-197 C.3
        Bytes key("000102030405060708090a0b0c0d0e0f101112131415161718191a1b1c1d1e1f"), pt("00112233445566778899aabbccddeeff"), ct("8ea2b7ca516745bfeafc49904b496089"), a(16), b(16);
        aes_cbc_c(key.p, Bytes("00000000000000000000000000000000").p, 0, pt.p, 1, a.p);
        aes_cbc_c(key.p, Bytes("00000000000000000000000000000000").p, 1, a.p, 1, b.p);
        check(a.eq(ct) && b.eq(pt), "FIPS-197 C.3");
    }
    Bytes key("603deb1015ca71be2b73aef0857d77811f352c073b6108d72d9810a30914dff4");
    Bytes pt("6bc1bee22e409f96e93d7e117393172aae2d8a571e03ac9c9eb76fac45af8e5130c81c46a35ce411e5fbc1191a0a52eff69f2445df4f9b17ad2b417be66c3710");
    {   // SP 800-38A F.2.5 / F.2.6
        Bytes iv("000102030405060708090a0b0c0d0e0f"), a(64), b(64);
        Bytes ct("f58c4c04d6e5f1ba779eabfb5f7bfbd69cfc4e967edb808d679f777bc6702c7d39f23369a9d9bacfa530e26304231461b2eb05e2c39be9fcda6c19078c6a9d1b");
        aes_cbc_c(key.p, iv.p, 0, pt.p, 4, a.p);
        aes_cbc_c(key.p, iv.p, 1, ct.p, 4, b.p);
        check(a.eq(ct) && b.eq(pt), "SP 800-38A F.2.5/F.2.6");
    }
    {   // SP 800-38A F.5.5 / F.5.6, whole and from every byte position on
        Bytes iv("f0f1f2f3f4f5f6f7f8f9fafbfcfdfeff");
        Bytes ct("601ec313775789a5b7a7f504bbf3d228f443e3ca4d62b59aca84e990cacaf5c52b0930daa23de94ce87017ba2d84988ddfc9c58db67aada613c2dd08457941a6");
        bool ok = true;
        for (size_t at = 0; at < 64; at++) {
            Bytes t(64 - at);
            memcpy(t.p, pt.p + at, 64 - at);
            aes_ctr_c(key.p, iv.p, at, t.p, 64 - at);
            ok = ok && memcmp(t.p, ct.p + at, 64 - at) == 0;
        }
        check(ok, "SP 800-38A F.5.5/F.5.6");
    }
    uint64_t seed = 0x9E3779B97F4A7C15ull;
    auto rnd = [&]() { seed ^= seed << 13; seed ^= seed >> 7; seed ^= seed << 17; return (uint8_t)(seed >> 32); };
    for (int t = 0; t < 200; t++) {        // aes_block_inv under aes256_dec_key inverts aes_block; CBC and CTR come back, the low counter half wraps
        Bytes k(32), iv(16), in(16 * (size_t)(t % 5)), a(in.n), b(in.n);
        for (size_t i = 0; i < 32; i++) k.p[i] = rnd();
        for (size_t i = 0; i < 16; i++) iv.p[i] = t % 3 == 0 && i >= 8 ? 0xFF : rnd();
        for (size_t i = 0; i < in.n; i++) in.p[i] = rnd();
        aes_cbc_c(k.p, iv.p, 0, in.p, in.n / 16, a.p);
        aes_cbc_c(k.p, iv.p, 1, a.p, in.n / 16, b.p);
        check(b.eq(in) && (in.n == 0 || !a.eq(in)), "CBC round trip");
        memcpy(a.p, in.p, in.n);
        aes_ctr_c(k.p, iv.p, (uint64_t)t, a.p, in.n);
        aes_ctr_c(k.p, iv.p, (uint64_t)t, a.p, in.n);
        check(a.eq(in), "CTR round trip");
    }
    printf("%d checks, %d bad\n", checks, bad);
    return bad || checks == 0 ? 1 : 0;
}
#endif
