// k_pick.hip -- pna_gpu_extract_select_host's device destinations: copy n pieces (PickPiece, pna_dev.h) -- bytes [src_off, src_off + len) of the
// launch's source buffer, where the decoders left an entry -- byte-exactly to the caller's dst[0 .. len).  The decoders round their stores up to 16 bytes
// and need slack behind the last entry, which a caller's exactly-sized tensor does not have: they keep writing into the driver's window buffers and this
// kernel carries each selected entry over.
//
// Memory-bound: one read and one write per byte.  Work distribution as k_diff's: a piece is cut into tiles of PICK_TILE bytes, one wave per tile, four
// tiles per workgroup; tile -> piece by binary search over the pieces' first-tile numbers (prefix sums made by the driver), so one piece of several GiB
// and 10^5 pieces of a few KiB both fill the chip.  Whole waves exit; there is no barrier.
//
// The caller chooses the destinations and inner entries of a solid stream start at any byte, so source and destination are misaligned against each other
// as a rule.  A tile's body is therefore written with aligned 16-byte stores, four per lane in flight (4 KiB per wave and step), and its source is read
// as ALIGNED 16-byte loads: a destination group takes its bytes from the one or two source groups that hold them, joined by v_alignbyte_b32 (the byte
// shift is the same for the whole tile).  Only the at most 15 bytes in front of the first and behind the last aligned destination group go bytewise.
// Loads: a 16-byte source group is read only if it holds a byte of the tile, i.e. nothing outside [src_off, src_off + len) rounded out to 16; the bytes
// of such a group beyond the piece are read and dropped.  Stores: nothing outside dst[0 .. len).
#include <hip/hip_runtime.h>
#include "pna_dev.h"

namespace pna {

static_assert(PICK_TILE % 4096 == 0, "a tile is a whole number of 4 KiB steps");

// the destination pointers come out of the piece list: said to be global memory, so that the stores are global_store and not flat_store instructions
typedef uint32_t v4u __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) v4u g_v4u;
typedef __attribute__((address_space(1))) uint8_t g_u8;

// dwords k .. k + 3 of the byte string w[0] w[1] ... shifted down by b bytes (b = 0 .. 3)
#define PICK_JOIN(k) make_uint4(__builtin_amdgcn_alignbyte(w[(k) + 1], w[(k)], b), __builtin_amdgcn_alignbyte(w[(k) + 2], w[(k) + 1], b), \
                                __builtin_amdgcn_alignbyte(w[(k) + 3], w[(k) + 2], b), __builtin_amdgcn_alignbyte(w[(k) + 4], w[(k) + 3], b))

__global__ __launch_bounds__(256)
void k_pick(const PickPiece *__restrict__ pieces, uint32_t npieces, uint32_t ntiles, const uint8_t *__restrict__ src) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t tile = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));     // wave-uniform: the search runs on the scalar unit
    if (tile >= ntiles) return;                                      // (whole waves leave: no barrier below)
    uint32_t lo = 0, hi = npieces - 1;                               // the last piece whose first tile is <= tile
    while (lo < hi) { const uint32_t mid = (lo + hi + 1) >> 1; if (pieces[mid].tile0 <= tile) lo = mid; else hi = mid - 1; }
    const PickPiece p = pieces[lo];
    const uint64_t s = (uint64_t)(tile - p.tile0) * PICK_TILE;       // the tile's offset in its piece
    if (s >= p.len) return;
    const uint32_t n = (uint32_t)min((uint64_t)PICK_TILE, p.len - s);
    const uint8_t *ps = src + p.src_off + s;
    g_u8 *pd = (g_u8 *)(p.dst + s);
    const uint32_t head = min(n, (uint32_t)((16 - ((uintptr_t)pd & 15)) & 15));      // bytes in front of the first aligned destination group
    if (lane < head) pd[lane] = ps[lane];
    const uint32_t nvec = (n - head) >> 4;
    const uint32_t sh = (uint32_t)((uintptr_t)(ps + head) & 15);     // where a destination group's first byte lies in its source group
    const uint4 *va = (const uint4 *)(ps + head - sh);               // the aligned source group that holds it
    g_v4u *vd = (g_v4u *)(pd + head);
    const uint32_t b = sh & 3;
    for (uint32_t v0 = 0; v0 < nvec; v0 += 256) {
        uint4 x[4], y[4];
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const uint32_t v = v0 + q * 64 + lane;
            x[q] = y[q] = make_uint4(0, 0, 0, 0);
            if (v < nvec) { x[q] = va[v]; if (sh) y[q] = va[v + 1]; }      // (sh != 0: the group's last 16 - sh .. 15 bytes lie in the next source group, which holds bytes of the tile)
        }
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const uint32_t v = v0 + q * 64 + lane;
            const uint32_t w[8] = {x[q].x, x[q].y, x[q].z, x[q].w, y[q].x, y[q].y, y[q].z, y[q].w};
            uint4 o;
            switch (sh >> 2) {                                       // (wave-uniform)
                case 0: o = PICK_JOIN(0); break;
                case 1: o = PICK_JOIN(1); break;
                case 2: o = PICK_JOIN(2); break;
                default: o = PICK_JOIN(3); break;
            }
            if (v < nvec) vd[v] = v4u{o.x, o.y, o.z, o.w};
        }
    }
    const uint32_t t0 = head + (nvec << 4);                          // the tail (<= 15 bytes)
    if (t0 + lane < n) pd[t0 + lane] = ps[t0 + lane];
}
#undef PICK_JOIN

void launch_pick(const PickPiece *pieces, uint32_t npieces, uint32_t ntiles, const uint8_t *src, hipStream_t st) {
    if (npieces && ntiles) hipLaunchKernelGGL(k_pick, dim3((ntiles + 3) / 4), dim3(256), 0, st, pieces, npieces, ntiles, src);
}

}
