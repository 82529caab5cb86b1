// crc_core.h -- the algebra of the chunk CRC-32 (reflected 0xEDB88320) in one place, for the host code and the kernels of k_store.hip: the raw register
// update, the multiplication by x^(8k) mod P, and the fold that turns the raw registers of consecutive pieces of a chunk's data into the chunk's CRC.
// The counterpart of aes_core.h / xz_core.h: builds with g++ alone (tests/store_core); no HIP header is needed.
//
// With R(s, M) the raw register update (no initial value, no final xor) the map R is linear over GF(2), and the three identities that k_frame.hip states
// at its head hold; restated once for what is built on them here:
//   (1) R(0xFFFFFFFF, M) = R(0, M ^ FF FF FF FF 00 00 ...)   |M| >= 4: the initial value folds into the first four bytes
//   (2) R(0, 0^k || M)   = R(0, M)                            zero bytes in front of a message are free
//   (3) R(s, A || B)     = Z_|B|(R(s, A)) ^ R(0, B)           Z_k = "append k zero bytes" = multiply the register by x^(8k) mod P
// A chunk's CRC is chunk_crc (lib/src/format/chunk.rs:7-12): crc32(type || data) = ~R(0xFFFFFFFF, type || data).  By (3), with the data cut into
// pieces D_0 .. D_{m-1} anywhere:   s_0 = R(0xFFFFFFFF, type),   s_{i+1} = Z_|D_i|(s_i) ^ R(0, D_i),   crc = ~s_m.
// A piece's R(0, D_i) depends on its bytes alone, so whoever moves the bytes can leave it behind (k_store), and whoever knows the cut folds (k_store_fold,
// the host).  Registers are in the reflected bit order of the table-driven CRC: bit 31 is x^0.
#pragma once
#include <stdint.h>
#include <stddef.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define CRC_HD __host__ __device__ __forceinline__
#else
#define CRC_HD inline
#endif

constexpr uint32_t CRC_POLY = 0xEDB88320u;
constexpr uint32_t CRC_ONE = 0x80000000u;           // the polynomial 1 (x^0)

// R(s, one byte), bit by bit: the definition every table is built from
CRC_HD uint32_t crc_raw_byte(uint32_t s, uint8_t b) {
    s ^= b;
    for (int k = 0; k < 8; k++) s = (s & 1) ? (s >> 1) ^ CRC_POLY : s >> 1;
    return s;
}
// R(s, M) over n bytes (no table: the host's few bytes -- a chunk type -- and the tests' reference)
CRC_HD uint32_t crc_raw_update(uint32_t s, const uint8_t *m, size_t n) {
    for (size_t i = 0; i < n; i++) s = crc_raw_byte(s, m[i]);
    return s;
}
// a * b mod P
CRC_HD uint32_t crc_mulmod(uint32_t a, uint32_t b) {
    uint32_t p = 0;
    for (int i = 0; i < 32; i++) {
        if (a & CRC_ONE) p ^= b;
        a <<= 1;
        b = (b & 1) ? (b >> 1) ^ CRC_POLY : b >> 1;
    }
    return p;
}
// x^e mod P (square and multiply: 2 log2(e) multiplications at most)
CRC_HD uint32_t crc_xpow(uint64_t e) {
    uint32_t r = CRC_ONE, base = CRC_ONE >> 1;
    while (e) { if (e & 1) r = crc_mulmod(base, r); base = crc_mulmod(base, base); e >>= 1; }
    return r;
}
// Z_k(s): the register after k more zero bytes = s * x^(8k) mod P
CRC_HD uint32_t crc_shift(uint32_t s, uint64_t k) { return s ? crc_mulmod(crc_xpow(8 * k), s) : 0u; }

// The fold of a chunk.  begin: s_0 = R(0xFFFFFFFF, type); step: one more piece of `len` bytes whose raw register R(0, piece) is `piece_state`
// (xp = x^(8 len) mod P when the caller has it at hand -- pieces mostly share one length --, 0: computed here); end: the chunk's CRC.
CRC_HD uint32_t crc_fold_begin(const uint8_t type[4]) { return crc_raw_update(0xFFFFFFFFu, type, 4); }
CRC_HD uint32_t crc_fold_step(uint32_t s, uint32_t piece_state, uint64_t len, uint32_t xp = 0) {
    return crc_mulmod(xp ? xp : crc_xpow(8 * len), s) ^ piece_state;
}
CRC_HD uint32_t crc_fold_end(uint32_t s) { return ~s; }

// The same fold on `lanes` lanes (k_store_fold: a wave), for a chunk of `len` data bytes cut into npieces pieces of `piece` bytes each but the last, which
// holds the rest (1 .. piece bytes).  Lane l takes the pieces l, l + lanes, ... : between the ends of two FULL pieces of a lane lie lanes * piece bytes, so
// their registers combine in Horner form with the one multiplier xstride = x^(8 * lanes * piece), and the sum is shifted from the end of the lane's last
// full piece to the chunk's end once.  The chunk's LAST piece ends at the chunk's end whatever its length: it is not part of the Horner sum -- the lane that
// owns it adds its register unshifted.  The XOR of all lanes' values and of Z_len(crc_fold_begin(type)) is the register crc_fold_end takes.
CRC_HD uint32_t crc_fold_lane(const uint32_t *states, uint32_t npieces, uint64_t len, uint64_t piece, uint32_t lane, uint32_t lanes, uint32_t xstride) {
    uint32_t acc = 0, tail = 0, last = 0xFFFFFFFFu;
    for (uint32_t j = lane; j < npieces; j += lanes) {
        if (j + 1 == npieces) { tail = states[j]; break; }
        acc = (acc ? crc_mulmod(xstride, acc) : 0u) ^ states[j];
        last = j;
    }
    if (last == 0xFFFFFFFFu) return tail;
    return crc_shift(acc, len - (uint64_t)(last + 1) * piece) ^ tail;       // (last < npieces - 1: the piece is full and ends inside the chunk)
}
