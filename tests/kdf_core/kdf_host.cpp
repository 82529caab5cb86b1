// kdf_host.cpp -- csrc/kdf_core.h on the CPU (tests/test_kdf_core.py): a C interface for ctypes, and -- with -DKDF_HOST_MAIN -- a stand-alone program
// that derives every case of a case file with buffers of exactly the needed sizes (built under -fsanitize=address,undefined by the Makefile).
// A case file is lines of
//     argon2 <kind> <t> <m KiB> <p> <password hex | -> <salt hex | -> <key hex>
//     pbkdf2 <rounds> <password hex | -> <salt hex | -> <key hex>
// ("-": no bytes), written by the test from answers of the oracle's Argon2 and of hashlib.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include "../../portable-network-archive_amd/csrc/kdf_core.h"

extern "C" {
// Argon2 (d / i / id by kind 0 / 1 / 2) over block memory of exactly m' KiB; -1: parameters out of range, -2: no memory
int kdf_argon2_c(int kind, const uint8_t *pw, size_t pw_len, const uint8_t *salt, size_t salt_len, uint32_t t, uint32_t m, uint32_t p, uint8_t *tag, uint32_t tag_len) {
    if (kind < 0 || kind > 2 || p < 1 || t < 1 || m < 8 * p || tag_len < 4) return -1;
    const KdfArgonGeom g = kdf_argon_geom(kind, t, m, p);
    uint64_t *mem = (uint64_t *)malloc((size_t)g.blocks * 1024);
    if (!mem) return -2;
    uint8_t h0[72];
    kdf_argon_h0(g, m, tag_len, pw, pw_len, salt, salt_len, h0);
    for (uint32_t l = 0; l < p; l++) for (uint32_t j = 0; j < 2; j++) kdf_argon_seed(h0, l, j, mem + ((size_t)l * g.lane_len + j) * 128);
    for (uint32_t pass = 0; pass < t; pass++) for (uint32_t slice = 0; slice < 4; slice++) for (uint32_t l = 0; l < p; l++) kdf_argon_fill_segment(mem, g, pass, slice, l);
    uint64_t fin[128];
    memcpy(fin, mem + ((size_t)g.lane_len - 1) * 128, sizeof fin);
    for (uint32_t l = 1; l < p; l++) for (int i = 0; i < 128; i++) fin[i] ^= mem[((size_t)l * g.lane_len + g.lane_len - 1) * 128 + i];
    kdf_argon_tag(fin, tag, tag_len);
    free(mem);
    return 0;
}
void kdf_pbkdf2_c(const uint8_t *pw, size_t pw_len, const uint8_t *salt, size_t salt_len, uint32_t rounds, uint8_t key[32]) {
    KdfPbkdf2Start s; kdf_pbkdf2_start(pw, pw_len, salt, salt_len, 1, s);
    uint32_t t[8]; kdf_pbkdf2_chain(s.istate, s.ostate, s.u1, rounds, t); kdf_words_be(t, key);
}
void kdf_blake2b_c(const uint8_t *in, size_t n, uint8_t *out, size_t outlen) { KdfBlake2b b; kdf_b2b_init(b, outlen); kdf_b2b_update(b, in, n); kdf_b2b_final(b, out); }
void kdf_sha256_c(const uint8_t *in, size_t n, uint8_t out[32]) { KdfSha256 s; s.init(); s.update(in, n); s.final(out); }
void kdf_hmac_sha256_c(const uint8_t *key, size_t key_len, const uint8_t *msg, size_t n, uint8_t out[32]) { KdfHmac h; h.key(key, key_len); h.mac(msg, n, nullptr, 0, out); }
// one compression, blocks of 128 words
void kdf_g_c(const uint64_t *prev, const uint64_t *ref, uint64_t *next, int xor_old) { kdf_g(prev, ref, next, xor_old != 0); }
}

#ifdef KDF_HOST_MAIN
// hex -> a heap buffer of exactly that many bytes (at least one is allocated, none of it beyond the length is ever touched)
struct Bytes {
    uint8_t *p; size_t n;
    explicit Bytes(size_t len) : p((uint8_t *)malloc(len ? len : 1)), n(len) {}
    explicit Bytes(const std::string &hex) : Bytes(hex == "-" ? 0 : hex.size() / 2) { for (size_t i = 0; i < n; i++) p[i] = (uint8_t)strtoul(hex.substr(2 * i, 2).c_str(), nullptr, 16); }
    Bytes(const Bytes &) = delete; Bytes &operator=(const Bytes &) = delete;
    ~Bytes() { free(p); }
    bool eq(const Bytes &o) const { return n == o.n && (n == 0 || memcmp(p, o.p, n) == 0); }
};
int main(int argc, char **argv) {
    if (argc < 2) { fprintf(stderr, "usage: %s cases.txt\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "r");
    if (!f) { perror(argv[1]); return 2; }
    static char algo[16], a[4096], b[4096], k[4096];
    int n = 0, bad = 0;
    while (fscanf(f, "%15s", algo) == 1) {
        bool ok = false;
        if (!strcmp(algo, "argon2")) {
            int kind; unsigned t, m, p;
            if (fscanf(f, "%d %u %u %u %4095s %4095s %4095s", &kind, &t, &m, &p, a, b, k) != 7) { fprintf(stderr, "bad case line\n"); return 2; }
            Bytes pw{std::string(a)}, salt{std::string(b)}, want{std::string(k)}, got(want.n);
            ok = kdf_argon2_c(kind, pw.p, pw.n, salt.p, salt.n, t, m, p, got.p, (uint32_t)got.n) == 0 && got.eq(want);
        } else if (!strcmp(algo, "pbkdf2")) {
            unsigned rounds;
            if (fscanf(f, "%u %4095s %4095s %4095s", &rounds, a, b, k) != 4) { fprintf(stderr, "bad case line\n"); return 2; }
            Bytes pw{std::string(a)}, salt{std::string(b)}, want{std::string(k)}, got(32);
            kdf_pbkdf2_c(pw.p, pw.n, salt.p, salt.n, rounds, got.p);
            ok = got.eq(want);
        } else { fprintf(stderr, "unknown case kind %s\n", algo); return 2; }
        n++;
        if (!ok) { bad++; printf("BAD case %d (%s)\n", n, algo); }
    }
    fclose(f);
    printf("%d cases, %d bad\n", n, bad);
    return bad || n == 0 ? 1 : 0;
}
#endif
