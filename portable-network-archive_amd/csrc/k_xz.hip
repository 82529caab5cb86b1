// k_xz.hip -- Compression::XZ on the read side (liblzma::bufread::XzDecoder, lib/src/entry/read.rs:171-190): .xz streams with LZMA2 blocks, decode only.
// The algorithm itself is xz_core.h (shared with the CPU test build); this file is how it is spread over the chip:
//   k_xzscan   one thread per stream: the container walk -- header, footer, Index, block headers, the chunk headers of every block.  Pass 1 (blocks == null)
//              counts: status, blocks, decoded size, largest lc + lp.  The host reads that back once, makes room, and pass 2 writes one XzBlock per block
//              and the check kernel's piece list.
//   k_lzma2    one wave per block, one wave per workgroup; the probability model (2 * xz_prob_count(lc + lp) bytes: 16 KiB at liblzma's lc = 3, 28 KiB at
//              most) is the workgroup's dynamic LDS, so the launch is sized by the largest lc + lp of its blocks and a CU holds as many blocks as its
//              160 KiB of LDS take.  The range decoder is a serial chain over wave-uniform values (scalar unit); matches and uncompressed chunks are
//              copied by all 64 lanes; the dictionary is the output buffer.
//   k_xzcheck  CRC32 / CRC64 of every block's decoded bytes: a workgroup per piece of 256 KiB, a thread per KiB; each thread's raw register is carried
//              to the block's end by a multiplication with x^(8 * bytes behind it) mod P and the shares are xor-ed into the block's accumulator.
//   k_xzfin    a thread per block: the accumulator finished (initial value, final xor) against the stored check; the blocks' statuses folded per stream.
// Bounds: k_xzscan reads inside [src_off, src_off + src_len) of its stream only; k_lzma2 reads the block's compressed bytes and reads and writes the
// block's decoded range only (xz_core.h); k_xzcheck reads decoded ranges; k_xzfin reads the stored check inside its block.
#include <hip/hip_runtime.h>
#include "pna_dev.h"
#include "xz_core.h"

namespace pna {

struct XzStreamIn { uint64_t src_off, src_len, dst_off; uint32_t blk_base, blk_cap, piece_base, piece_cap; };   // = XzStreamInH of pna_decode.cpp
struct XzPiece { uint32_t blk, idx; };
constexpr uint32_t XZ_PIECE = 256u << 10, XZ_SUB = 1024;

__global__ __launch_bounds__(64)
void k_xzscan(const XzStreamIn *__restrict__ in, uint32_t n, const uint8_t *__restrict__ src, XzScan *__restrict__ out, XzBlock *__restrict__ blocks,
              XzPiece *__restrict__ pieces) {
    const uint32_t i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    const XzStreamIn s = in[i];
    XzScan sc;
    if (!blocks) { xz_scan(src + s.src_off, s.src_len, s.src_off, s.dst_off, i, &sc, nullptr, 0); out[i] = sc; return; }
    if (s.blk_cap == 0 && s.piece_cap == 0) return;                     // (refused by pass 1, or no block: nothing to write)
    xz_scan(src + s.src_off, s.src_len, s.src_off, s.dst_off, i, &sc, blocks + s.blk_base, s.blk_cap);
    if (sc.status != XZ_OK || sc.nblk != s.blk_cap) {                   // (cannot be: the same bytes as in pass 1)
        for (uint32_t r = 0; r < s.blk_cap; r++) { XzBlock &b = blocks[s.blk_base + r]; b = XzBlock{}; b.stream = i; b.status = XZ_CORRUPT; }
        sc.nblk = 0;
    }
    uint32_t pc = 0;
    for (uint32_t r = 0; r < sc.nblk; r++) {
        const XzBlock &b = blocks[s.blk_base + r];
        if (b.check == XZ_CHECK_NONE) continue;
        const uint32_t np = (uint32_t)(((uint64_t)b.dst_len + XZ_PIECE - 1) / XZ_PIECE);
        for (uint32_t k = 0; k < np && pc < s.piece_cap; k++) pieces[s.piece_base + pc++] = XzPiece{s.blk_base + r, k};
    }
    for (; pc < s.piece_cap; pc++) pieces[s.piece_base + pc] = XzPiece{0xFFFFFFFFu, 0};
}

__global__ __launch_bounds__(64)
void k_lzma2(XzBlock *blocks, uint32_t nblk, const uint8_t *src, uint8_t *dst, uint32_t lclp_cap) {
    extern __shared__ __attribute__((aligned(16))) uint16_t xz_probs[];
    const uint32_t i = blockIdx.x, lane = threadIdx.x;
    if (i >= nblk) return;
    const XzBlock b = blocks[i];
    if (b.status != XZ_OK) return;
    const uint32_t st = xz_lzma2_block(src + b.src, b.src_len, dst + b.dst, b.dst_len, b.dict, xz_probs, lclp_cap, lane);
    if (lane == 0) blocks[i].status = st;
}

__global__ __launch_bounds__(256)
void k_xzcheck(const XzPiece *__restrict__ pieces, uint32_t npieces, const XzBlock *__restrict__ blocks, const uint8_t *__restrict__ dst,
               unsigned long long *__restrict__ acc) {
    __shared__ uint64_t tab[256];
    __shared__ uint64_t part[4];
    if (blockIdx.x >= npieces) return;
    const XzPiece pc = pieces[blockIdx.x];
    if (pc.blk == 0xFFFFFFFFu) return;                                   // (the whole workgroup leaves: no barrier passed yet)
    const XzBlock b = blocks[pc.blk];
    if (b.status != XZ_OK || b.check == XZ_CHECK_NONE) return;
    const uint32_t t = threadIdx.x;
    tab[t] = xz_crc_tab_entry(t, xz_poly_low(b.check));
    __syncthreads();
    const uint64_t at = (uint64_t)pc.idx * XZ_PIECE + (uint64_t)t * XZ_SUB;     // this thread's KiB of the block
    uint64_t share = 0;
    if (at < b.dst_len) {
        const uint64_t len = min((uint64_t)XZ_SUB, (uint64_t)b.dst_len - at);
        const uint64_t raw = xz_crc_raw(dst + b.dst + at, len, tab, 0);
        share = xz_crc_share(xz_crc_top(raw, b.check), (uint64_t)b.dst_len - at - len, b.check);
    }
    for (int d = 32; d >= 1; d >>= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)share, d), hi = (uint32_t)__shfl_xor((int)(uint32_t)(share >> 32), d);
        share ^= ((uint64_t)hi << 32) | lo;
    }
    if ((t & 63) == 0) part[t >> 6] = share;
    __syncthreads();
    if (t == 0) atomicXor(&acc[pc.blk], (unsigned long long)(part[0] ^ part[1] ^ part[2] ^ part[3]));
}

__global__ __launch_bounds__(256)
void k_xzfin(const XzBlock *__restrict__ blocks, uint32_t nblk, const uint8_t *__restrict__ src, const unsigned long long *__restrict__ acc,
             uint32_t *__restrict__ stream_status) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= nblk) return;
    const XzBlock b = blocks[i];
    uint32_t st = b.status;
    if (st == XZ_OK && b.check != XZ_CHECK_NONE) {
        const uint32_t cs = xz_check_size(b.check);
        uint64_t stored = 0;
        for (uint32_t k = 0; k < cs; k++) stored |= (uint64_t)src[b.check_off + k] << (8 * k);
        if (xz_crc_finish(acc[i], b.dst_len, b.check) != stored) st = XZ_CORRUPT;
    }
    if (st) atomicMax(&stream_status[b.stream], st);
}

void launch_xzscan(const void *streams, uint32_t n, const uint8_t *src, XzScan *out, XzBlock *blocks, void *pieces, hipStream_t st) {
    if (n) hipLaunchKernelGGL(k_xzscan, dim3((n + 63) / 64), dim3(64), 0, st, (const XzStreamIn *)streams, n, src, out, blocks, (XzPiece *)pieces);
}
void launch_lzma2(XzBlock *blocks, uint32_t nblk, const uint8_t *src, uint8_t *dst, uint32_t lclp, hipStream_t st) {
    if (nblk) hipLaunchKernelGGL(k_lzma2, dim3(nblk), dim3(64), (size_t)xz_prob_count(lclp) * 2, st, blocks, nblk, src, dst, lclp);
}
void launch_xzcheck(const void *pieces, uint32_t npieces, const XzBlock *blocks, uint32_t nblk, const uint8_t *src, const uint8_t *dst, uint64_t *acc,
                    uint32_t *stream_status, hipStream_t st) {
    if (npieces) hipLaunchKernelGGL(k_xzcheck, dim3(npieces), dim3(256), 0, st, (const XzPiece *)pieces, npieces, blocks, dst, (unsigned long long *)acc);
    if (nblk) hipLaunchKernelGGL(k_xzfin, dim3((nblk + 255) / 256), dim3(256), 0, st, blocks, nblk, src, (const unsigned long long *)acc, stream_status);
}

}
