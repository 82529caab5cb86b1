// k_store.hip -- Compression::No on the device: a stored payload goes from the source buffer to its place in the archive in ONE pass that also leaves
// the CRC-32 of what it moved, and a second, small kernel folds those into the chunks' CRC fields (crc_core.h has the algebra).
//
//   k_store<true>   one 256-thread workgroup per PIECE of at most 1 MiB of one data chunk: dst[dst_off .. +len) = src[src_off .. +len) at any byte
//                   alignment on either side, and states[piece] = R(0, piece), the raw CRC register of the piece's bytes alone.
//   k_store<false>  the copy alone, for payloads that a cipher changes where they stand: their CRC is over the ciphertext and stays with k_frame.
//   k_store_fold    one WAVE per data chunk: the states of the chunk's pieces and the chunk type -> the big-endian CRC behind the payload, and FEND
//                   behind it where the chunk is its entry's last.
// Neither k_store form writes a byte outside [dst_off, dst_off + len) or reads one outside [src_off, src_off + len): chunk cuts by max_chunk_size and
// name lengths put both anywhere, and the neighbours of a piece are other workgroups' bytes.
//
// The piece's message is anchored at its END, as k_frame's is: it is front-padded with zero bytes (free, identity (2)) to whole tiles of 16 KiB, lane t
// owns the 64 bytes t of every tile -- four 16-byte loads and four 16-byte stores at byte addresses --, advances its register between tiles by Z_16320
// (four look-ups in LDS) and takes its 64 bytes through the slice-by-4 tables (LDS as well).  A log-step tree folds the 256 lane registers with the
// fixed shifts 64 * 2^j.  A piece of at most 256 bytes (max_chunk_size = 5 makes hundreds per entry) loads no table: a byte per lane, each shifted to
// the piece's end by one multiplication.
#include <hip/hip_runtime.h>
#include "pna_dev.h"
#include "crc_core.h"

namespace pna {

constexpr uint32_t ST_THREADS = 256;
constexpr uint32_t ST_TILE = ST_THREADS * 64;
constexpr uint32_t ST_TINY = 256;                          // pieces up to this many bytes take the table-free form

struct __attribute__((packed, aligned(1))) U4 { uint32_t x, y, z, w; };         // 16 bytes at any byte address

// XOR over the workgroup's 256 values (every thread calls; the result is valid on thread 0)
__device__ __forceinline__ uint32_t wg_xor(uint32_t v, uint32_t *part) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v ^= (uint32_t)__shfl_xor((int)v, o);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
    __syncthreads();
    return part[0] ^ part[1] ^ part[2] ^ part[3];
}

template <bool CRC>
__global__ __launch_bounds__(ST_THREADS)
void k_store(const StorePiece *__restrict__ pd, const uint8_t *__restrict__ src, uint8_t *__restrict__ dst, const CrcTabs *__restrict__ ct,
             uint32_t *__restrict__ states) {
    const StorePiece d = pd[blockIdx.x];
    const uint32_t tid = threadIdx.x;
    const uint8_t *s = src + d.src_off;
    uint8_t *o = dst + d.dst_off;
    if (!CRC) {
        const uint32_t n16 = d.len >> 4;
        for (uint32_t i = tid; i < n16; i += ST_THREADS) *(U4 *)(o + 16 * (size_t)i) = *(const U4 *)(s + 16 * (size_t)i);
        const uint32_t done = n16 << 4;
        if (tid < d.len - done) o[done + tid] = s[done + tid];
        return;
    }
    __shared__ uint32_t part[ST_THREADS];
    if (d.len <= ST_TINY) {
        uint32_t v = 0;
        if (tid < d.len) { const uint8_t b = s[tid]; o[tid] = b; v = crc_shift(crc_raw_byte(0u, b), d.len - 1 - tid); }
        v = wg_xor(v, part);
        if (tid == 0) states[blockIdx.x] = v;
        return;
    }
    __shared__ uint32_t sT[4][256], sZ[4][256];
    for (uint32_t i = tid; i < 1024; i += ST_THREADS) { (&sT[0][0])[i] = (&ct->T[0][0])[i]; (&sZ[0][0])[i] = (&ct->Z[0][0])[i]; }
    __syncthreads();
    const uint32_t ntile = (d.len + ST_TILE - 1) / ST_TILE;           // (len <= 1 MiB: 64 tiles at most)
    const uint32_t pad = ntile * ST_TILE - d.len;                     // zero bytes in front, < ST_TILE
    uint32_t state = 0;
    for (uint32_t k = 0; k < ntile; k++) {
        const int32_t g0 = (int32_t)(k * ST_TILE + tid * 64) - (int32_t)pad;   // piece offset of the lane's 64 bytes; they end at or before len (len - g0 is a multiple of 64)
        if (g0 + 64 <= 0) continue;                                   // all padding: the register is still zero
        uint32_t w[16];
#pragma unroll
        for (int g = 0; g < 4; g++) {
            const int32_t gp = g0 + 16 * g;
            U4 v = {0, 0, 0, 0};
            if (gp >= 0) { v = *(const U4 *)(s + gp); *(U4 *)(o + gp) = v; }
            else if (gp + 16 > 0) {                                   // the group that straddles the piece's first byte: its bytes singly
                uint32_t q[4] = {0, 0, 0, 0};
                for (int b = -gp; b < 16; b++) { const uint8_t x = s[gp + b]; o[gp + b] = x; q[b >> 2] |= (uint32_t)x << (8 * (b & 3)); }
                v.x = q[0]; v.y = q[1]; v.z = q[2]; v.w = q[3];
            }
            w[4 * g] = v.x; w[4 * g + 1] = v.y; w[4 * g + 2] = v.z; w[4 * g + 3] = v.w;
        }
        state = sZ[0][state & 0xFF] ^ sZ[1][(state >> 8) & 0xFF] ^ sZ[2][(state >> 16) & 0xFF] ^ sZ[3][state >> 24];
#pragma unroll
        for (int j = 0; j < 16; j++) {
            const uint32_t c = state ^ w[j];
            state = sT[3][c & 0xFF] ^ sT[2][(c >> 8) & 0xFF] ^ sT[1][(c >> 16) & 0xFF] ^ sT[0][c >> 24];
        }
    }
    part[tid] = state;
    __syncthreads();
    for (uint32_t j = 0; j < 8; j++) {
        const uint32_t st = 1u << j;
        if ((tid & (2 * st - 1)) == 0) { const uint32_t pv = part[tid]; part[tid] = (pv ? crc_mulmod(ct->sh[j], pv) : 0u) ^ part[tid + st]; }
        __syncthreads();
    }
    if (tid == 0) states[blockIdx.x] = part[0];
}

// One wave per chunk.  Lane l takes the pieces l, l + 64, ... in Horner form -- between two of them lie 64 pieces of STORE_PIECE bytes, one fixed
// multiplier --, shifts its sum to the chunk's end once, and the wave XORs: a chunk of 4 GiB (4 096 pieces) costs a lane 64 + ~70 multiplications.
// A chunk whose pieces are not all STORE_PIECE long but the last (flags bit 1: a solid stream's SDAT cut fell into it) is folded piece by piece on
// lane 0 with the lengths of the piece list.  ty_state = R(0xFFFFFFFF, type) (crc_fold_begin), the same for every chunk of a launch.
// sd_ch != 0: the chunks are the inner records' of a stored solid stream -- crc_off is a position in that stream, and stream position p stands at
// sd_base + p + sd_ovh * (p / sd_ch) of dst (SDAT chunks of sd_ch data bytes, sd_ovh bytes of framing between two of them): the field may straddle one.
__global__ __launch_bounds__(256)
void k_store_fold(const StoreChunk *__restrict__ cf, uint32_t nchunk, const uint32_t *__restrict__ states, const StorePiece *__restrict__ pd,
                  uint32_t ty_state, uint32_t fend_crc, uint8_t *__restrict__ dst, uint64_t sd_base, uint64_t sd_ch, uint64_t sd_ovh) {
    const uint32_t lane = threadIdx.x & 63, ch = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (ch >= nchunk) return;
    const StoreChunk f = cf[ch];
    uint32_t x = 0;
    if (f.flags & 2) {
        if (lane == 0) {
            const uint32_t x1 = crc_xpow((uint64_t)8 * STORE_PIECE);
            x = ty_state;
            for (uint32_t j = 0; j < f.npieces; j++) { const uint32_t pl = pd[f.first + j].len; x = crc_fold_step(x, states[f.first + j], pl, pl == STORE_PIECE ? x1 : 0u); }
        }
    } else {
        // (crc_core.h crc_fold_lane: the chunk's last piece, which may be short, stays out of the Horner sum -- the tests run this schedule on the CPU too)
        const uint32_t x64 = f.npieces > 64 ? crc_xpow((uint64_t)8 * 64 * STORE_PIECE) : 0u;
        x = crc_fold_lane(states + f.first, f.npieces, f.len, STORE_PIECE, lane, 64u, x64);
        if (lane == 0) x ^= crc_shift(ty_state, f.len);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x ^= (uint32_t)__shfl_xor((int)x, o);
    if (lane < ((f.flags & 1) ? 16u : 4u)) {
        const uint32_t crc = crc_fold_end(x);
        const uint32_t fe = 0x444E4546u;                              // "FEND" little-endian
        uint8_t v;                                                    // crc BE | 00 00 00 00 | "FEND" | crc("FEND") BE
        if (lane < 4) v = (uint8_t)(crc >> (24 - 8 * lane));
        else if (lane < 8) v = 0;
        else if (lane < 12) v = (uint8_t)(fe >> (8 * (lane - 8)));
        else v = (uint8_t)(fend_crc >> (24 - 8 * (lane - 12)));
        const uint64_t p = f.crc_off + lane;
        dst[sd_ch ? sd_base + p + sd_ovh * (p / sd_ch) : p] = v;
    }
}

// pieces: StorePiece x n in device memory; with_crc: the fused form (states: n words)
void launch_store(const void *pieces, uint32_t n, const uint8_t *src, uint8_t *dst, const CrcTabs *ct, uint32_t *states, bool with_crc, hipStream_t st) {
    if (!n) return;
    if (with_crc) hipLaunchKernelGGL(k_store<true>, dim3(n), dim3(ST_THREADS), 0, st, (const StorePiece *)pieces, src, dst, ct, states);
    else hipLaunchKernelGGL(k_store<false>, dim3(n), dim3(ST_THREADS), 0, st, (const StorePiece *)pieces, src, dst, ct, (uint32_t *)nullptr);
}
void launch_store_fold(const void *chunks, uint32_t n, const uint32_t *states, const void *pieces, const char ty[4], uint32_t fend_crc, uint8_t *dst, hipStream_t st,
                       uint64_t sd_base, uint64_t sd_ch, uint64_t sd_ovh) {
    if (n) hipLaunchKernelGGL(k_store_fold, dim3((n + 3) / 4), dim3(256), 0, st, (const StoreChunk *)chunks, n, states, (const StorePiece *)pieces,
                              crc_fold_begin((const uint8_t *)ty), fend_crc, dst, sd_base, sd_ch, sd_ovh);
}

} // namespace pna
