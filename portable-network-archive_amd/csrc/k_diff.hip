// k_diff.hip -- `pna experimental diff` on the device (cli/src/command/diff.rs streams_equal): where do an entry's decoded bytes and the file's bytes
// first differ?  Both sides lie in HBM -- `a` the decoded bytes where the decoders left them, `b` the file bytes the driver copied in -- and the
// work is a list of pieces (DiffPiece, pna_dev.h): bytes [base, base + len) of entry `entry`, a at a_off, b at b_off.  first[entry] starts as all-ones
// and ends as the smallest base + i with a[a_off + i] != b[b_off + i] over the entry's pieces.
//
// Memory-bound: two reads per byte and nothing written but one 64-bit atomicMin per wave that found a difference.  A piece is cut into tiles of
// DIFF_TILE bytes, one wave per tile, four tiles per workgroup; tile -> piece by binary search over the pieces' first-tile numbers (prefix sums
// made by the driver), so one 5 GiB entry and 10^6 entries of 100 bytes both fill the chip.  The driver places the b side so that a_off and b_off
// are congruent mod 16 (inner entries of a solid stream start at any byte): the unaligned head and tail of a tile are compared bytewise, one byte
// per lane, the body with 16-byte loads on both sides, four per lane in flight (4 KiB per wave and step).  Within a step the lanes that differ are
// found by ballot, the first one's first differing byte by ctz of the XOR.  A piece whose sides are not congruent is compared bytewise.
#include <hip/hip_runtime.h>
#include "pna_dev.h"

namespace pna {

static_assert(DIFF_TILE % 4096 == 0, "a tile is a whole number of 4 KiB steps");

__device__ __forceinline__ uint32_t first_diff_byte(const uint4 x, const uint4 y) {      // the sides differ: index of the first byte that does
    const uint32_t d0 = x.x ^ y.x, d1 = x.y ^ y.y, d2 = x.z ^ y.z, d3 = x.w ^ y.w;
    if (d0) return (uint32_t)__builtin_ctz(d0) >> 3;
    if (d1) return 4u + ((uint32_t)__builtin_ctz(d1) >> 3);
    if (d2) return 8u + ((uint32_t)__builtin_ctz(d2) >> 3);
    return 12u + ((uint32_t)__builtin_ctz(d3) >> 3);
}

__global__ __launch_bounds__(256)
void k_diff(const DiffPiece *__restrict__ pieces, uint32_t npieces, uint32_t ntiles, const uint8_t *__restrict__ a, const uint8_t *__restrict__ b,
            unsigned long long *first) {
    const uint32_t lane = threadIdx.x & 63, tile = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (tile >= ntiles) return;                                      // (whole waves leave: no barrier below)
    uint32_t lo = 0, hi = npieces - 1;                               // the last piece whose first tile is <= tile
    while (lo < hi) { const uint32_t mid = (lo + hi + 1) >> 1; if (pieces[mid].tile0 <= tile) lo = mid; else hi = mid - 1; }
    const DiffPiece p = pieces[lo];
    const uint64_t s = (uint64_t)(tile - p.tile0) * DIFF_TILE;       // the tile's offset in its piece
    if (s >= p.len) return;
    // a difference in front of this tile is already known (a stale value only costs the work)
    if (__hip_atomic_load(&first[p.entry], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) <= p.base + s) return;
    const uint32_t n = (uint32_t)min((uint64_t)DIFF_TILE, p.len - s);
    const uint8_t *pa = a + p.a_off + s, *pb = b + p.b_off + s;
    const bool congruent = (((uintptr_t)pa ^ (uintptr_t)pb) & 15) == 0;
    const uint32_t head = congruent ? min(n, (uint32_t)((16 - ((uintptr_t)pa & 15)) & 15)) : n;
    uint32_t found = 0xFFFFFFFFu;                                    // wave-uniform: offset of the first difference in the tile
    for (uint32_t i0 = 0; i0 < head && found == 0xFFFFFFFFu; i0 += 64) {      // the head (<= 15 bytes; the whole tile when the sides are not congruent)
        const uint32_t i = i0 + lane;
        const uint64_t m = __ballot(i < head && pa[i] != pb[i]);
        if (m) found = i0 + (uint32_t)__builtin_ctzll(m);
    }
    const uint32_t nvec = (n - head) >> 4;
    const uint4 *va = (const uint4 *)(pa + head), *vb = (const uint4 *)(pb + head);
    for (uint32_t v0 = 0; v0 < nvec && found == 0xFFFFFFFFu; v0 += 256) {
        uint4 x[4], y[4]; bool d[4];
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const uint32_t v = v0 + q * 64 + lane;
            x[q] = y[q] = make_uint4(0, 0, 0, 0);
            if (v < nvec) { x[q] = va[v]; y[q] = vb[v]; }
        }
#pragma unroll
        for (int q = 0; q < 4; q++) d[q] = ((x[q].x ^ y[q].x) | (x[q].y ^ y[q].y) | (x[q].z ^ y[q].z) | (x[q].w ^ y[q].w)) != 0;
        if (__ballot(d[0] | d[1] | d[2] | d[3]) == 0) continue;
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const uint64_t m = __ballot(d[q]);
            if (m && found == 0xFFFFFFFFu) {
                const uint32_t l = (uint32_t)__builtin_ctzll(m);
                const uint32_t byte = d[q] ? first_diff_byte(x[q], y[q]) : 0u;
                found = head + ((v0 + q * 64 + l) << 4) + (uint32_t)__shfl((int)byte, (int)l);
            }
        }
    }
    const uint32_t t0 = head + (nvec << 4);                          // the tail (<= 15 bytes)
    if (found == 0xFFFFFFFFu && t0 < n) {
        const uint32_t i = t0 + lane;
        const uint64_t m = __ballot(i < n && pa[i] != pb[i]);
        if (m) found = t0 + (uint32_t)__builtin_ctzll(m);
    }
    if (found != 0xFFFFFFFFu && lane == 0) atomicMin(&first[p.entry], (unsigned long long)(p.base + s + found));
}

void launch_diff(const DiffPiece *pieces, uint32_t npieces, uint32_t ntiles, const uint8_t *a, const uint8_t *b, unsigned long long *first, hipStream_t st) {
    if (npieces && ntiles) hipLaunchKernelGGL(k_diff, dim3((ntiles + 3) / 4), dim3(256), 0, st, pieces, npieces, ntiles, a, b, first);
}

}
