// k_camellia.hip -- Camellia-256 in the cipher stage, on gfx950: CTR (Ctr128BE), CBC encryption (PKCS#7) and CBC decryption over payloads where they
// stand in HBM.  The Camellia arm of the reference's CipherWriter / DecryptReader (Encryption::CAMELLIA, lib/src/cipher.rs:16-77; the writers and
// readers named in k_cipher.hip's header take the block cipher as a type parameter).  GCM STREAM over Camellia is k_cam_ctr under per-segment keys plus
// k_cipher.hip's GHASH kernels, which take H and E(K, J0) from the host and do not care which cipher made them.
//
// The block function is camellia_core.h's table form (cam_block): 24 rounds of 8 look-ups in four 256 x 32-bit tables, the 34 subkeys a kernel argument
// of 272 bytes (scalar registers).  Integer / table work, no MFMA.  The unit scheme, the byte-wise handling of partial blocks and the launch geometry are
// those of the AES kernels, so the host plans one unit list for either cipher.
//
// Table layout of k_cam_ctr: the layout k_aes_ctr measured best for random byte-indexed look-ups -- the four tables replicated over the 32 LDS banks
// (entry x of table t for bank b is word (t * 256 + x) * 32 + b, lane l reads bank l & 31 only: a wave's look-ups are conflict-free by construction),
// 128 KiB of the CU's 160 KiB, one workgroup of 1024 per CU, workgroups striding over the units so that the image is built once per workgroup.  Measured
// on the payloads of 10 000 x 1 MiB zstd 3 (3.43 GiB in 20 000 units; profiles/camellia_rate.txt): 8.12 ms, k_aes_ctr 7.77 ms on the same bytes -- 192
// look-ups per block against AES's 224; where the rest of the time goes (instruction issue, by k_aes_ctr's account of itself) was not examined.  No other
// layout was tried for Camellia; the CBC kernels, bound by their serial chain or by one workgroup per entry, keep four shared 1 KiB tables.
#include <hip/hip_runtime.h>
#include "pna_dev.h"
#include "camellia_core.h"

namespace pna {

struct __attribute__((packed, aligned(1))) CU4u { uint32_t x, y, z, w; };   // 16 bytes at any byte address

struct CamSharedTab {                     // four shared tables: T_i[x] at sT[i * 256 + x]
    const uint32_t *sT;
    __device__ __forceinline__ uint32_t operator()(uint32_t i, uint32_t x) const { return sT[(i << 8) + x]; }
};
struct CamBankTab {                       // bank-replicated: `my` points at this lane's bank of entry 0 of table 0
    const uint8_t *my;
    __device__ __forceinline__ uint32_t operator()(uint32_t i, uint32_t x) const { return *(const uint32_t *)(my + (i << 15) + (x << 7)); }
};

// ------------------------------------------------------------------ CTR (Ctr128BE), in place; encrypt == decrypt
// Unit u covers buf[off .. off + len) = stream bytes [pos, pos + len) of the stream whose IV is ivs[iv_idx]; keys != null: the unit's own schedule
// keys[iv_idx] (GCM STREAM: every segment names its stream's key).  Nothing outside a unit's bytes is written.
constexpr uint32_t CAM_CTR_THREADS = 1024;
constexpr uint32_t CAM_CTR_LDS = 4 * 256 * 32 * 4;                    // 128 KiB

__global__ __launch_bounds__(CAM_CTR_THREADS)
void k_cam_ctr(const CipherUnit *__restrict__ units, uint32_t nunits, const uint8_t *__restrict__ ivs, const CamTabs *__restrict__ tabs,
               uint8_t *__restrict__ buf, const CamKey key0, const CamKey *__restrict__ keys) {
    extern __shared__ __attribute__((aligned(16))) uint32_t sR[];
    const uint32_t tid = threadIdx.x;
    {   // thread t owns table entry (t >> 8, t & 255): one global read, 32 bank copies
        const uint32_t v = tabs->T[tid >> 8][tid & 0xFF];
        uint32_t *row = sR + (tid << 5);
#pragma unroll
        for (int b = 0; b < 32; b += 4) *(uint4 *)(row + b) = make_uint4(v, v, v, v);
    }
    const CamBankTab tab{(const uint8_t *)sR + ((tid & 31) << 2)};
    __syncthreads();
    for (uint32_t ui = blockIdx.x; ui < nunits; ui += gridDim.x) {
        const CipherUnit u = units[ui];
        CamKey key = key0;
        if (keys) key = keys[u.iv_idx];                               // (wave-uniform load)
        const uint8_t *ivp = ivs + (size_t)u.iv_idx * 16;
        uint64_t iv_hi = 0, iv_lo = 0;                                // the IV as a 128-bit big-endian number
        for (int b = 0; b < 8; b++) { iv_hi = (iv_hi << 8) | ivp[b]; iv_lo = (iv_lo << 8) | ivp[8 + b]; }
        const uint64_t b0 = u.pos >> 4;                               // first keystream block of the unit
        const uint64_t end = u.pos + u.len;
        const uint32_t nblk = (uint32_t)(((end + 15) >> 4) - b0);
        const int64_t base = (int64_t)u.off - (int64_t)(u.pos & 15);  // buf offset of keystream block b0's byte 0
        for (uint32_t j = tid; j < nblk; j += CAM_CTR_THREADS) {
            const uint64_t lo = iv_lo + b0 + j, hi = iv_hi + (lo < iv_lo ? 1u : 0u);
            uint32_t w0 = (uint32_t)(hi >> 32), w1 = (uint32_t)hi, w2 = (uint32_t)(lo >> 32), w3 = (uint32_t)lo;
            cam_block(tab, key, w0, w1, w2, w3);
            const uint32_t s0 = __builtin_bswap32(w0), s1 = __builtin_bswap32(w1), s2 = __builtin_bswap32(w2), s3 = __builtin_bswap32(w3);   // as the bytes lie in memory
            const int64_t a = base + (int64_t)j * 16;
            const uint64_t sp = (b0 + j) << 4;                        // stream position of this block
            if (sp >= u.pos && sp + 16 <= end) {
                CU4u *q = (CU4u *)(buf + a);
                CU4u v = *q;
                v.x ^= s0; v.y ^= s1; v.z ^= s2; v.w ^= s3;
                *q = v;
            } else {                                                  // first / last block of the unit: only the bytes inside it
                const uint32_t ks[4] = {s0, s1, s2, s3};
                for (uint32_t b = 0; b < 16; b++) {
                    const uint64_t p = sp + b;
                    if (p >= u.pos && p < end) buf[a + b] ^= (uint8_t)(ks[b >> 2] >> (8 * (b & 3)));
                }
            }
        }
    }
}

// ------------------------------------------------------------------ CBC encryption with PKCS#7 padding, in place, one lane per entry
// Entry e: plaintext buf[off .. off + len) becomes (len / 16 + 1) * 16 bytes of ciphertext at the same offset (the layout leaves room for the padding
// block).  The chain is serial; block b + 1 is requested before block b goes through the rounds.
__global__ __launch_bounds__(64)
void k_cam_cbc_enc(const CipherUnit *__restrict__ units, uint32_t n, const uint8_t *__restrict__ ivs, const CamTabs *__restrict__ tabs,
                   uint8_t *__restrict__ buf, const CamKey key) {
    __shared__ uint32_t sT[1024];
    for (uint32_t i = threadIdx.x; i < 1024; i += 64) sT[i] = (&tabs->T[0][0])[i];
    __syncthreads();
    const CamSharedTab tab{sT};
    const uint32_t e = blockIdx.x * 64 + threadIdx.x;
    if (e >= n) return;
    const CipherUnit u = units[e];
    const CU4u iv = *(const CU4u *)(ivs + (size_t)u.iv_idx * 16);
    uint32_t c0 = __builtin_bswap32(iv.x), c1 = __builtin_bswap32(iv.y), c2 = __builtin_bswap32(iv.z), c3 = __builtin_bswap32(iv.w);
    const uint32_t nb = u.len / 16 + 1;
    uint8_t *p = buf + u.off;
    CU4u nx = {0, 0, 0, 0};
    if (nb > 1) nx = *(const CU4u *)p;
    for (uint32_t b = 0; b < nb; b++) {
        uint32_t x0, x1, x2, x3;                                      // the plaintext block as it lies in memory (little-endian words)
        if (b + 1 < nb) {
            x0 = nx.x; x1 = nx.y; x2 = nx.z; x3 = nx.w;
            if (b + 2 < nb) nx = *(const CU4u *)(p + 16 * (size_t)(b + 1));
        } else {
            const uint32_t have = u.len - 16 * b, padv = 16 - have;
            uint32_t w[4] = {0, 0, 0, 0};
            for (uint32_t k2 = 0; k2 < 16; k2++) { const uint32_t byte = k2 < have ? p[16 * (size_t)b + k2] : padv; w[k2 >> 2] |= byte << (8 * (k2 & 3)); }
            x0 = w[0]; x1 = w[1]; x2 = w[2]; x3 = w[3];
        }
        c0 ^= __builtin_bswap32(x0); c1 ^= __builtin_bswap32(x1); c2 ^= __builtin_bswap32(x2); c3 ^= __builtin_bswap32(x3);
        cam_block(tab, key, c0, c1, c2, c3);
        CU4u o; o.x = __builtin_bswap32(c0); o.y = __builtin_bswap32(c1); o.z = __builtin_bswap32(c2); o.w = __builtin_bswap32(c3);
        *(CU4u *)(p + 16 * (size_t)b) = o;
    }
}

// ------------------------------------------------------------------ CBC decryption, block-parallel: P_j = D(C_j) ^ C_(j-1), C_(-1) = IV
// One workgroup per unit, 256 blocks per step, in place: a step loads its ciphertext (and the block in front of it) before anything is written, the last
// ciphertext block of a step is carried to the next one through LDS.  The PKCS#7 padding is checked at the unit's end and the plaintext length reported
// (0xFFFFFFFF: bad length or padding) -- the outputs of k_aes_cbc_dec.  `key`: the decrypt-order schedule (cam_dec_key).
__global__ __launch_bounds__(256)
void k_cam_cbc_dec(const CipherUnit *__restrict__ units, const uint8_t *__restrict__ ivs, const CamTabs *__restrict__ tabs,
                   uint8_t *__restrict__ buf, const CamKey key, uint32_t *__restrict__ plain_len) {
    __shared__ uint32_t sT[1024];
    __shared__ uint32_t carry[4];
    const uint32_t tid = threadIdx.x;
    for (uint32_t i = tid; i < 1024; i += 256) sT[i] = (&tabs->T[0][0])[i];
    const CamSharedTab tab{sT};
    const CipherUnit u = units[blockIdx.x];
    if (tid == 0) { const CU4u iv = *(const CU4u *)(ivs + (size_t)u.iv_idx * 16); carry[0] = iv.x; carry[1] = iv.y; carry[2] = iv.z; carry[3] = iv.w; }
    __syncthreads();
    if (u.len == 0 || (u.len & 15)) { if (tid == 0) plain_len[blockIdx.x] = 0xFFFFFFFFu; return; }
    const uint32_t nb = u.len >> 4;
    uint8_t *p = buf + u.off;
    for (uint32_t base = 0; base < nb; base += 256) {
        const uint32_t j = base + tid;
        CU4u cj = {0, 0, 0, 0}, pv = {0, 0, 0, 0};
        if (j < nb) {
            cj = *(const CU4u *)(p + 16 * (size_t)j);
            if (tid) pv = *(const CU4u *)(p + 16 * (size_t)(j - 1)); else { pv.x = carry[0]; pv.y = carry[1]; pv.z = carry[2]; pv.w = carry[3]; }
        }
        __syncthreads();                                             // everyone holds its ciphertext: the step may overwrite it now
        if (j < nb) {
            uint32_t w0 = __builtin_bswap32(cj.x), w1 = __builtin_bswap32(cj.y), w2 = __builtin_bswap32(cj.z), w3 = __builtin_bswap32(cj.w);
            cam_block(tab, key, w0, w1, w2, w3);
            CU4u o; o.x = __builtin_bswap32(w0) ^ pv.x; o.y = __builtin_bswap32(w1) ^ pv.y; o.z = __builtin_bswap32(w2) ^ pv.z; o.w = __builtin_bswap32(w3) ^ pv.w;
            *(CU4u *)(p + 16 * (size_t)j) = o;
            if (tid == 255) { carry[0] = cj.x; carry[1] = cj.y; carry[2] = cj.z; carry[3] = cj.w; }
            if (j + 1 == nb) {                                       // PKCS#7: the last byte names the padding length, all padding bytes repeat it
                const uint32_t pad = o.w >> 24;
                bool ok = pad >= 1 && pad <= 16;
                const uint32_t w[4] = {o.x, o.y, o.z, o.w};
                for (uint32_t k = 0; ok && k < pad; k++) { const uint32_t bi = 15 - k; ok = ((w[bi >> 2] >> (8 * (bi & 3))) & 0xFF) == pad; }
                plain_len[blockIdx.x] = ok ? u.len - pad : 0xFFFFFFFFu;
            }
        }
        __syncthreads();                                             // the carry is in place before the next step's lane 0 reads it
    }
}

void launch_cam_ctr(const CipherUnit *units, uint32_t n, const uint8_t *ivs, const CamTabs *tabs, uint8_t *buf, const CamKey &key, const CamKey *keys, hipStream_t st) {
    static const hipError_t attr_set = hipFuncSetAttribute((const void *)k_cam_ctr, hipFuncAttributeMaxDynamicSharedMemorySize, (int)CAM_CTR_LDS);   // once, thread-safe
    (void)attr_set;
    // one workgroup per CU at a time (128 KiB of LDS); a few per CU in the grid even out the ragged units
    if (n) hipLaunchKernelGGL(k_cam_ctr, dim3(n < 1024 ? n : 1024), dim3(CAM_CTR_THREADS), CAM_CTR_LDS, st, units, n, ivs, tabs, buf, key, keys);
}
void launch_cam_cbc_enc(const CipherUnit *units, uint32_t n, const uint8_t *ivs, const CamTabs *tabs, uint8_t *buf, const CamKey &key, hipStream_t st) {
    if (n) hipLaunchKernelGGL(k_cam_cbc_enc, dim3((n + 63) / 64), dim3(64), 0, st, units, n, ivs, tabs, buf, key);
}
void launch_cam_cbc_dec(const CipherUnit *units, uint32_t n, const uint8_t *ivs, const CamTabs *tabs, uint8_t *buf, const CamKey &dkey, uint32_t *plain_len, hipStream_t st) {
    if (n) hipLaunchKernelGGL(k_cam_cbc_dec, dim3(n), dim3(256), 0, st, units, ivs, tabs, buf, dkey, plain_len);
}

} // namespace pna
