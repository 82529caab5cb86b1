// The chunk CRC algebra of csrc/crc_core.h on the CPU (tests/test_store_core.py): the message "FDAT" || data is split into pieces at every cut of a list,
// each piece's raw register R(0, piece) is taken on its own, the registers are folded (crc_fold_begin / _step / _end over the data pieces, and the general
// identity (3) where a cut falls inside the type), and the result is compared with a bitwise CRC-32 of the whole message written here.  Buffers have
// exactly the needed sizes: the program is also built with -fsanitize=address,undefined.  Prints "sample <len> <crc>" lines for the pytest side (which
// compares them with zlib.crc32) and "<n> checks, <bad> bad".
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../../portable-network-archive_amd/csrc/crc_core.h"

static uint64_t checks = 0, bad = 0;
#define CHECK(cond, ...) do { checks++; if (!(cond)) { bad++; if (bad < 20) { printf("BAD %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } } while (0)

// the reference: CRC-32 (reflected 0xEDB88320, init and final xor 0xFFFFFFFF), one bit at a time, nothing shared with crc_core.h
static uint32_t crc32_bitwise(const uint8_t *p, size_t n) {
    uint32_t c = 0xFFFFFFFFu;
    for (size_t i = 0; i < n; i++) {
        c ^= p[i];
        for (int k = 0; k < 8; k++) c = (c >> 1) ^ (0xEDB88320u & (0u - (c & 1u)));
    }
    return ~c;
}
// a faster raw register for the long messages: byte table built from crc_raw_byte (the pieces of 1 MiB would take seconds bit by bit under the sanitizers)
static uint32_t T8[256];
static uint32_t raw_table(uint32_t s, const uint8_t *p, size_t n) {
    for (size_t i = 0; i < n; i++) s = T8[(s ^ p[i]) & 0xFF] ^ (s >> 8);
    return s;
}
// data byte i of the message of `len` data bytes (the pytest side rebuilds the samples from this formula)
static uint8_t data_byte(size_t i, size_t len) { return (uint8_t)((((uint32_t)i * 2654435761u) >> 13) ^ (uint32_t)len); }

// the cuts of the MESSAGE (type included) for one scheme; a scheme returns piece lengths that sum to n
static std::vector<size_t> cut_scheme(int scheme, size_t n) {
    std::vector<size_t> out;
    size_t left = n;
    auto take = [&](size_t k) { k = k < left ? k : left; if (k) { out.push_back(k); left -= k; } };
    switch (scheme) {
        case 0: take(n); break;                                            // one piece
        case 1: while (left) take(1); break;                               // 1-byte pieces
        case 2: take(2); while (left) take(7); break;                      // a cut inside the type, then sevens
        case 3: take(4); while (left) take(1u << 20); break;               // the type, then pieces of 1 MiB (k_store's cut)
        case 4: take(4); while (left) take(5); break;                      // max_chunk_size = 5's pieces
        case 5: { size_t k = 1; take(3); while (left) { take(k); k = k * 3 + 1; } break; }   // uneven, growing
        case 6: take(4); take(left / 2); take(left); break;                // two halves
        case 7: take(4); take(left > 16380 ? 16380 : left); while (left) take(65536 + 1); break;
    }
    return out;
}
static const int NSCHEME = 8;

static void one_length(size_t len) {
    std::vector<uint8_t> msg(4 + len);
    memcpy(msg.data(), "FDAT", 4);
    for (size_t i = 0; i < len; i++) msg[4 + i] = data_byte(i, len);
    const uint32_t want = crc32_bitwise(msg.data(), msg.size());
    if (len == 0 || len == 1 || len == 300 || len == 4097 || len == 1048577 || len == 3145745) printf("sample %zu %08x\n", len, want);
    for (int sc = 0; sc < NSCHEME; sc++) {
        const std::vector<size_t> cuts = cut_scheme(sc, msg.size());
        // identity (3) over the whole message, pieces anywhere: s = Z_|piece|(s) ^ R(0, piece) from s = R(0xFFFFFFFF, "") = 0xFFFFFFFF
        uint32_t s = 0xFFFFFFFFu; size_t pos = 0;
        for (size_t pl : cuts) {
            std::vector<uint8_t> piece(msg.begin() + pos, msg.begin() + pos + pl);           // its own buffer: a read past the piece is a sanitizer error
            const uint32_t st = pl <= 64 ? crc_raw_update(0u, piece.data(), pl) : raw_table(0u, piece.data(), pl);
            s = crc_fold_step(s, st, pl);
            pos += pl;
        }
        CHECK(pos == msg.size() && crc_fold_end(s) == want, "len %zu scheme %d: %08x != %08x", len, sc, crc_fold_end(s), want);
        // the data chunk's fold as k_store_fold runs it: begin with the type, then the data pieces (schemes that cut behind the type)
        if (!cuts.empty() && cuts[0] == 4) {
            uint32_t f = crc_fold_begin((const uint8_t *)"FDAT"); pos = 4;
            const uint32_t xp_mib = crc_xpow(8ull << 20);
            for (size_t q = 1; q < cuts.size(); q++) {
                const size_t pl = cuts[q];
                const uint32_t st = raw_table(0u, msg.data() + pos, pl);
                f = crc_fold_step(f, st, pl, pl == (1u << 20) ? xp_mib : 0u);
                pos += pl;
            }
            CHECK(crc_fold_end(f) == want, "len %zu scheme %d (fold): %08x != %08x", len, sc, crc_fold_end(f), want);
        }
    }
    // Z_k: shifting the whole register at once equals k single zero bytes
    if (len <= 300) {
        uint32_t a = raw_table(0x12345678u ^ (uint32_t)len, msg.data(), msg.size()), b = a;
        for (size_t i = 0; i < len; i++) b = crc_raw_byte(b, 0);
        CHECK(crc_shift(a, len) == b, "shift by %zu", len);
    }
}

// k_store_fold's schedule (crc_fold_lane on 64 lanes, pieces of `piece` bytes, the last one the rest) against the CRC of the whole chunk: more than 64 pieces
// with a short last piece is where a lane's Horner sum must leave the last piece out
static void lane_schedule(size_t len, size_t piece) {
    std::vector<uint8_t> data(len);
    for (size_t i = 0; i < len; i++) data[i] = data_byte(i, len);
    const uint32_t ty = crc_fold_begin((const uint8_t *)"FDAT");
    const uint32_t want = ~raw_table(ty, data.data(), len);                      // (the table form is held against the bitwise one in main and one_length)
    const uint32_t np = (uint32_t)((len + piece - 1) / piece);
    std::vector<uint32_t> states(np);
    for (uint32_t j = 0; j < np; j++) states[j] = raw_table(0u, data.data() + (size_t)j * piece, j + 1 == np ? len - (size_t)j * piece : piece);
    const uint32_t xs = np > 64 ? crc_xpow((uint64_t)8 * 64 * piece) : 0u;
    uint32_t x = crc_shift(ty, len);
    for (uint32_t lane = 0; lane < 64; lane++) x ^= crc_fold_lane(states.data(), np, len, piece, lane, 64u, xs);
    CHECK(crc_fold_end(x) == want, "lane schedule: len %zu piece %zu: %08x != %08x", len, piece, crc_fold_end(x), want);
    if (piece == (1u << 20)) printf("lanes %zu %08x\n", len, crc_fold_end(x));
}

int main() {
    for (uint32_t i = 0; i < 256; i++) T8[i] = crc_raw_byte(0u, (uint8_t)i);
    { const uint8_t d[9] = {'1', '2', '3', '4', '5', '6', '7', '8', '9'}; CHECK(crc32_bitwise(d, 9) == 0xCBF43926u, "check value"); CHECK(~raw_table(0xFFFFFFFFu, d, 9) == 0xCBF43926u, "table"); }
    CHECK(crc_xpow(0) == CRC_ONE && crc_mulmod(CRC_ONE, 0xDEADBEEFu) == 0xDEADBEEFu && crc_xpow(32) == CRC_POLY, "x^0, 1 * a, x^32 mod P");
    CHECK(crc_mulmod(crc_xpow(1000), crc_xpow(24)) == crc_xpow(1024), "x^a x^b = x^(a + b)");
    for (size_t len = 0; len <= 300; len++) one_length(len);
    for (size_t len : {(size_t)4095, (size_t)4096, (size_t)4097, (size_t)65535, (size_t)1048575, (size_t)1048576, (size_t)1048577, (size_t)3145745}) one_length(len);
    for (size_t np = 1; np <= 200; np++)                                         // pieces of 1 000 bytes: every piece count around one, two and three rounds of the lanes
        for (size_t r : {(size_t)1, (size_t)5, (size_t)999, (size_t)1000}) lane_schedule((np - 1) * 1000 + r, 1000);
    for (size_t len : {((size_t)3 << 20) + 17, (size_t)64 << 20, ((size_t)64 << 20) + 5, ((size_t)65 << 20) - 16, (size_t)65 << 20, ((size_t)130 << 20) + 7}) lane_schedule(len, 1u << 20);
    printf("%llu checks, %llu bad\n", (unsigned long long)checks, (unsigned long long)bad);
    return bad ? 1 : 0;
}
