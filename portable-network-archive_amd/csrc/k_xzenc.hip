// k_xzenc.hip -- Compression::XZ on the write side (XzEncoder::new(writer, level), lib/src/entry/write.rs:257-263): per entry one .xz stream of one block
// per 1 MiB segment, one LZMA2 chunk per LZ block (include/pna_gpu.h has the format rules).  The algorithm itself is xz_enc_core.h (shared with the CPU
// test build); this file is how it is spread over the chip, behind the LZ stage and in front of the cipher / framing stages, as k_deflate.hip is:
//   k_xzcrc      CRC64 of every segment's INPUT bytes: a workgroup per piece of 256 KiB (as many per segment as the batch's longest segment has), a thread
//                per KiB, k_xzcheck's share arithmetic (xz_core.h) over the source buffer; the shares are xor-ed into the segment's accumulator.
//   k_lzma2enc   the chunk coder: one wave per LZ block, one wave per workgroup; the probability model (7 992 x 2 bytes) is the workgroup's dynamic LDS, as
//                in k_lzma2, so a CU holds ten chunks.  The coder is a serial chain over wave-uniform values -- decision, model index, probability (one LDS
//                round trip), bound, low / range, probability update --; the segment's bytes and the block's sequences reach it through windows that all
//                64 lanes load (256 bytes / 64 sequences at a time).  Output: the block's slot of the scratch (1 << blk_log bytes: the coder stops once
//                its output reaches the chunk's input size, xz_enc_core.h), lane 0's byte stores.  BlkInfo::lit_body = the LZMA form's size, 0: stored.
//   k_xzplan     a thread per segment: chunk sizes and offsets (BlkInfo::out_size / out_off / plan), the block's unpadded size.
//   k_xzsize     a thread per segment: its bytes in the entry's stream -- the stream header in front of an entry's first block, the Index (sized over the
//                entry's blocks) and the footer behind its last -- into seg_size; the scan over them gives seg_off, as in the deflate path.
//   k_xzwrite    a workgroup per LZ block: the chunk header and the chunk from the scratch (or, stored, from the source); a segment's first block also
//                writes the stream and block headers, its last the end marker, the padding and the finished CRC64.
//   k_xzfinal    a thread per entry: the Index with its CRC32 and the stream footer; an empty entry's 32-byte stream.
// Bounds: k_lzma2enc reads its segment's bytes and its block's sequences (count clamped to the slot's capacity) and writes its scratch slot only;
// k_xzwrite / k_xzfinal write inside [seg_off[s], seg_off[s] + seg_size[s]) of their segments only.
#include <hip/hip_runtime.h>
#include "pna_dev.h"
#include "xz_enc_core.h"

namespace pna {

typedef uint32_t v4u __attribute__((ext_vector_type(4)));
static __device__ __forceinline__ v4u xe_ld16u(const uint8_t *p) { v4u v; __builtin_memcpy(&v, p, 16); return v; }   // 16 bytes at any byte address
constexpr uint32_t XE_PIECE = 256u << 10, XE_SUB = 1024;

__global__ __launch_bounds__(256)
void k_xzcrc(const uint8_t *__restrict__ src, const SegDesc *__restrict__ segs, uint32_t nseg, uint32_t pieces_per_seg, unsigned long long *__restrict__ acc) {
    __shared__ uint64_t tab[256];
    __shared__ uint64_t part[4];
    const uint32_t sidx = blockIdx.x / pieces_per_seg, piece = blockIdx.x % pieces_per_seg;
    if (sidx >= nseg) return;
    const SegDesc sd = segs[sidx];
    if ((uint64_t)piece * XE_PIECE >= sd.len) return;                    // (the whole workgroup leaves: no barrier passed yet)
    const uint32_t t = threadIdx.x;
    tab[t] = xz_crc_tab_entry(t, XZ_POLY64);
    __syncthreads();
    const uint32_t at = piece * XE_PIECE + t * XE_SUB;                   // this thread's KiB of the segment
    uint64_t share = 0;
    if (at < sd.len) {
        const uint32_t len = min(XE_SUB, sd.len - at);
        const uint64_t raw = xz_crc_raw(src + sd.src_off + at, len, tab, 0);
        share = xz_crc_share(raw, (uint64_t)sd.len - at - len, XZ_CHECK_CRC64);
    }
    for (int d = 32; d >= 1; d >>= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)share, d), hi = (uint32_t)__shfl_xor((int)(uint32_t)(share >> 32), d);
        share ^= ((uint64_t)hi << 32) | lo;
    }
    if ((t & 63) == 0) part[t >> 6] = share;
    __syncthreads();
    if (t == 0) atomicXor(&acc[sidx], (unsigned long long)(part[0] ^ part[1] ^ part[2] ^ part[3]));
}

__global__ __launch_bounds__(64)
void k_lzma2enc(const uint8_t *__restrict__ src, const SegDesc *__restrict__ segs, const uint32_t *__restrict__ blk_seg, uint32_t nblk,
                const uint64_t *__restrict__ seqs, BlkInfo *__restrict__ blk, uint8_t *__restrict__ scratch) {
    extern __shared__ __attribute__((aligned(16))) uint16_t xze_probs[];
    const uint32_t g = blockIdx.x, lane = threadIdx.x;
    if (g >= nblk) return;
    const SegDesc sd = segs[blk_seg[g]];
    const uint32_t bsz = 1u << sd.blk_log, c0 = (g - sd.blk_base) << sd.blk_log;
    if (c0 >= sd.len || sd.blk_log > 16) return;                          // (cannot be: the plan's blocks lie inside their segments, at most 64 KiB each)
    const uint32_t clen = min(bsz, sd.len - c0), cap = seq_cap_of(sd.blk_log);
    const uint32_t nseq = min((uint32_t)__builtin_amdgcn_readfirstlane((int)blk[g].nseq), cap);
    const uint32_t size = xze_chunk(src + sd.src_off, sd.len, c0, clen, seqs + (size_t)g * cap, nseq, xze_probs, scratch + ((size_t)g << sd.blk_log), bsz, lane);
    if (lane == 0) blk[g].lit_body = size;
}

__global__ void k_xzplan(const SegDesc *__restrict__ segs, uint32_t nseg, BlkInfo *__restrict__ blk, uint64_t *__restrict__ unpadded) {
    const uint32_t sidx = blockIdx.x * blockDim.x + threadIdx.x;
    if (sidx >= nseg) return;
    const SegDesc sd = segs[sidx];
    if (sd.len == 0) { unpadded[sidx] = 0; return; }
    const uint32_t nb = seg_nblk(sd), bsz = 1u << sd.blk_log;
    uint64_t off = ((sd.first & 1) ? (uint64_t)XZE_STREAM_HEADER : 0) + XZE_BLOCK_HEADER, chunks = 0;
    for (uint32_t b = 0; b < nb; b++) {
        const uint32_t g = sd.blk_base + b, clen = min(bsz, sd.len - b * bsz);
        const uint32_t lz = blk[g].lit_body, sz = xze_chunk_bytes(lz, clen);
        blk[g].plan = lz ? 1u : 0u; blk[g].out_size = sz; blk[g].out_off = off + chunks;
        chunks += sz;
    }
    unpadded[sidx] = xze_block_unpadded(chunks);
}

// the Index of the entry whose last segment is `last`: counted (o == null) or written; its size
static __device__ uint64_t xe_index(const SegDesc *__restrict__ segs, const uint64_t *__restrict__ unpadded, uint32_t first, uint32_t last, uint8_t *o) {
    XzeIndex ix; xze_idx_begin(ix, o, (uint64_t)last - first + 1);
    for (uint32_t s = first; s <= last; s++) xze_idx_record(ix, unpadded[s], segs[s].len);
    return xze_idx_end(ix);
}
__global__ void k_xzsize(const SegDesc *__restrict__ segs, uint32_t nseg, const uint64_t *__restrict__ unpadded, uint64_t *__restrict__ seg_size) {
    const uint32_t sidx = blockIdx.x * blockDim.x + threadIdx.x;
    if (sidx >= nseg) return;
    const SegDesc sd = segs[sidx];
    if (sd.len == 0) { seg_size[sidx] = 32; return; }                    // an empty entry: header, an Index without records, footer
    uint64_t sz = ((sd.first & 1) ? (uint64_t)XZE_STREAM_HEADER : 0) + ((unpadded[sidx] + 3) & ~3ull);
    if (sd.first & 2) {
        uint32_t first = sidx;
        while (first > 0 && !(segs[first].first & 1)) first--;           // (an entry's segments lie behind each other)
        sz += xe_index(segs, unpadded, first, sidx, nullptr) + XZE_STREAM_FOOTER;
    }
    seg_size[sidx] = sz;
}

__global__ __launch_bounds__(256)
void k_xzwrite(const uint8_t *__restrict__ src, const SegDesc *__restrict__ segs, const uint32_t *__restrict__ blk_seg, const BlkInfo *__restrict__ blk,
               const uint64_t *__restrict__ seg_off, const uint8_t *__restrict__ scratch, const uint64_t *__restrict__ unpadded,
               const unsigned long long *__restrict__ acc, uint8_t *__restrict__ dst) {
    const uint32_t tid = threadIdx.x, g = blockIdx.x, T = blockDim.x;
    const uint32_t sidx = blk_seg[g];
    const SegDesc sd = segs[sidx];
    const BlkInfo bi = blk[g];
    const uint32_t b = g - sd.blk_base, nb = seg_nblk(sd), bsz = 1u << sd.blk_log;
    const uint32_t c0 = b * bsz, clen = min(bsz, sd.len - c0);
    uint8_t *seg_out = dst + seg_off[sidx], *out = seg_out + bi.out_off;
    const uint32_t lz = (bi.plan & 1) ? bi.lit_body : 0u, hl = lz ? 6u : 3u;
    if (tid == 0) {
        uint8_t h[6];
        xze_chunk_header(h, b == 0, lz, clen);
        for (uint32_t i = 0; i < hl; i++) out[i] = h[i];
    }
    // (the three small jobs go to threads 0, 64 and 128 -- three waves -- where the workgroup has them, to thread 0 in its wave-per-block form)
    if (b == 0 && tid == 64 % T) {                                       // the stream header (an entry's first block) and the block header
        uint8_t h[12];
        uint8_t *o = seg_out;
        if (sd.first & 1) { xze_stream_header(h); for (int i = 0; i < 12; i++) o[i] = h[i]; o += XZE_STREAM_HEADER; }
        xze_block_header(h);
        for (int i = 0; i < 12; i++) o[i] = h[i];
    }
    if (b + 1 == nb && tid == 128 % T) {                                 // the end marker, the padding, the check
        uint8_t *blk_out = seg_out + ((sd.first & 1) ? XZE_STREAM_HEADER : 0);
        uint64_t at = unpadded[sidx] - 9;
        blk_out[at++] = 0;
        while (at & 3) blk_out[at++] = 0;
        const uint64_t crc = xz_crc_finish(acc[sidx], sd.len, XZ_CHECK_CRC64);
        for (int k = 0; k < 8; k++) blk_out[at + k] = (uint8_t)(crc >> (8 * k));
    }
    // n bytes from p to o: the destination's unaligned head and tail byte by byte, its aligned middle as 16-byte stores of unaligned 16-byte loads
    const uint8_t *p = lz ? scratch + ((size_t)g << sd.blk_log) : src + sd.src_off + c0;
    uint8_t *o = out + hl;
    const uint32_t n = lz ? lz : clen;
    const uint32_t head = (uint32_t)((16u - ((uintptr_t)o & 15u)) & 15u), h = head < n ? head : n, mid = (n - h) >> 4;
    if (tid < h) o[tid] = p[tid];
    for (uint32_t i = tid; i < mid; i += T) *(v4u *)(o + h + 16 * i) = xe_ld16u(p + h + 16 * i);
    for (uint32_t i = h + 16 * mid + tid; i < n; i += T) o[i] = p[i];
}

__global__ void k_xzfinal(const SegDesc *__restrict__ segs, const uint32_t *__restrict__ entry_seg, uint32_t nentry, const uint64_t *__restrict__ seg_off,
                          const uint64_t *__restrict__ seg_size, const uint64_t *__restrict__ unpadded, uint8_t *__restrict__ dst) {
    const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= nentry) return;
    const uint32_t s0 = entry_seg[e], s1 = entry_seg[e + 1];
    if (s1 <= s0) return;
    if (segs[s0].len == 0) {
        uint8_t *o = dst + seg_off[s0];
        xze_stream_header(o);
        XzeIndex ix; xze_idx_begin(ix, o + XZE_STREAM_HEADER, 0);
        const uint64_t isz = xze_idx_end(ix);
        xze_stream_footer(o + XZE_STREAM_HEADER + isz, isz);
        return;
    }
    uint8_t *end = dst + seg_off[s1 - 1] + seg_size[s1 - 1];             // segment offsets need not be contiguous (in-HBM framing)
    const uint64_t isz = xe_index(segs, unpadded, s0, s1 - 1, nullptr);
    xe_index(segs, unpadded, s0, s1 - 1, end - XZE_STREAM_FOOTER - isz);
    xze_stream_footer(end - XZE_STREAM_FOOTER, isz);
}

void k_scan_launch_big(const uint64_t *in, uint64_t *out, uint32_t n, hipStream_t st);

// max_seg: the longest segment's bytes (the CRC kernel's grid holds that segment's pieces per segment, not a whole MiB's: one for small entries).
// work: 2 * nseg 64-bit words -- the blocks' unpadded sizes, then the CRC64 accumulators.  ev: three events (after the CRC kernel, after the coder, after the sizes) or null
void launch_xzenc_stage(const uint8_t *src, const SegDesc *segs, uint32_t nseg, uint32_t max_seg, const uint32_t *blk_seg, uint32_t nblk, const uint64_t *seqs, BlkInfo *blk,
                        uint8_t *scratch, uint64_t *work, uint64_t *seg_size, uint64_t *seg_off, hipStream_t st, hipEvent_t *ev) {
    uint64_t *unpadded = work; unsigned long long *acc = (unsigned long long *)(work + nseg);
    (void)hipMemsetAsync(acc, 0, (size_t)nseg * 8, st);
    const uint32_t longest = max_seg < SEG_SIZE ? max_seg : SEG_SIZE, pieces_per_seg = longest ? (longest + XE_PIECE - 1) / XE_PIECE : 1u;
    hipLaunchKernelGGL(k_xzcrc, dim3(nseg * pieces_per_seg), dim3(256), 0, st, src, segs, nseg, pieces_per_seg, acc);
    if (ev) (void)hipEventRecord(ev[0], st);
    if (nblk) hipLaunchKernelGGL(k_lzma2enc, dim3(nblk), dim3(64), (size_t)XZE_PROBS * 2, st, src, segs, blk_seg, nblk, seqs, blk, scratch);
    if (ev) (void)hipEventRecord(ev[1], st);
    hipLaunchKernelGGL(k_xzplan, dim3((nseg + 255) / 256), dim3(256), 0, st, segs, nseg, blk, unpadded);
    hipLaunchKernelGGL(k_xzsize, dim3((nseg + 255) / 256), dim3(256), 0, st, segs, nseg, unpadded, seg_size);
    k_scan_launch_big(seg_size, seg_off, nseg, st);
    if (ev) (void)hipEventRecord(ev[2], st);
}

void launch_xzenc_write(const uint8_t *src, const SegDesc *segs, const uint32_t *blk_seg, uint32_t nblk, const BlkInfo *blk, const uint64_t *seg_off,
                        const uint64_t *seg_size, const uint8_t *scratch, const uint64_t *work, uint32_t nseg, const uint32_t *entry_seg, uint32_t nentry,
                        uint8_t *dst, hipStream_t st, bool small_blocks) {
    const uint64_t *unpadded = work; const unsigned long long *acc = (const unsigned long long *)(work + nseg);
    if (nblk) hipLaunchKernelGGL(k_xzwrite, dim3(nblk), dim3(small_blocks ? 64 : 256), 0, st, src, segs, blk_seg, blk, seg_off, scratch, unpadded, acc, dst);
    hipLaunchKernelGGL(k_xzfinal, dim3((nentry + 255) / 256), dim3(256), 0, st, segs, entry_seg, nentry, seg_off, seg_size, unpadded, dst);
}

} // namespace pna
