// k_cipher.hip -- the cipher stage between the compressor and the chunk sink, on gfx950: AES-256 and Camellia-256 in CTR (Ctr128BE) and CBC
// (PKCS#7) mode over payloads that already sit at their archive offsets in HBM, and the GHASH / tag kernel of GCM STREAM.
//
// Replaces CipherWriter::{CtrAes, CbcAes, CtrCamellia, CbcCamellia} (lib/src/entry/write.rs:189-248 encryption_writer; lib/src/cipher/stream/write.rs:52-58
// apply_keystream; lib/src/cipher/block/write.rs:44-57,67-107; Encryption::CAMELLIA, lib/src/cipher.rs:16-77) in the stack compress -> cipher -> sink
// (get_writer, lib/src/entry/write.rs:268-274) and, on the read side, DecryptReader::CtrAes / CbcAes and their Camellia arms (lib/src/entry/read.rs:77-88).
// The reference's writers and readers take the block cipher as a type parameter; so do the three mode bodies here (ctr_body, cbc_enc_body, cbc_dec_body),
// written once over a block-cipher policy -- AesCipher over aes_core.h, CamCipher over camellia_core.h -- and instantiated as six kernels.  GCM STREAM is
// the CTR kernel under per-segment keys plus k_gcm_tag, which takes H and E(K, J0) from the host and does not care which cipher made them.
//
// Integer/table work, no MFMA.  One 16-byte block per lane and step; the round tables live in LDS (CTR: every table replicated per bank, CBC: four
// shared ones), the key schedule (AES: 15 round keys, 240 bytes; Camellia: 34 subkeys, 272 bytes) arrives as a kernel argument (scalar registers).
// CTR: block j of a stream is E(IV + j) with the IV read as one 128-bit big-endian counter; every block is independent, so a stream is cut into units
// of <= 256 KiB (any byte position: the unit carries its stream offset) and each unit is one workgroup's work.  CBC encryption chains its blocks, so
// there the parallelism is across entries only: one lane per entry.  The host plans one unit list for either cipher.
//
// Table layout of the CTR kernels: the four tables replicated over the 32 LDS banks -- entry x of table t for bank b is word (t * 256 + x) * 32 + b,
// and lane l only ever reads bank l & 31.  A wave's 64 look-ups are then conflict-free by construction (the two halves of a wave go through the LDS in
// different cycles), where four shared 1 KiB tables serialise random look-ups ~3.6-fold (k_aes_ctr, measured on 10 000 x 1 MiB: 11.1 ms shared tables ->
// 8.0 ms one replicated table + rotations -> 7.6 ms four replicated tables, workgroups striding over the units so that the 128 KiB table image -- of
// the CU's 160 KiB -- is built once per workgroup).  What is left is instruction issue: 882 VALU + 224 LDS instructions per AES block and lane.
// k_cam_ctr took that layout over (measured on the payloads of 10 000 x 1 MiB zstd 3, 3.43 GiB in 20 000 units; profiles/camellia_rate.txt: 8.12 ms,
// k_aes_ctr 7.77 ms on the same bytes -- 192 look-ups per block against AES's 224; where the rest of the time goes was not examined).  No other layout
// was tried for Camellia; the CBC kernels, bound by their serial chain or by one workgroup per entry, keep four shared 1 KiB tables and were not measured.
#include <hip/hip_runtime.h>
#include "pna_dev.h"
#include "camellia_core.h"

namespace pna {

struct __attribute__((packed, aligned(1))) U4u { uint32_t x, y, z, w; };   // 16 bytes at any byte address (unaligned dwordx4 access)

// shared tables: entry x of table i at sT[i * 256 + x].  Two spellings of that address, each the one its cipher's kernels were written and measured
// with -- the compiler folds AES's table offset into the LDS instruction and adds Camellia's to the index; making them one is tuning, not done here
struct AesSharedTab {
    const uint32_t *sT;
    __device__ __forceinline__ uint32_t operator()(uint32_t i, uint32_t x) const { return (sT + (i << 8))[x]; }
};
struct CamSharedTab {
    const uint32_t *sT;
    __device__ __forceinline__ uint32_t operator()(uint32_t i, uint32_t x) const { return sT[(i << 8) + x]; }
};
struct BankTab {                          // bank-replicated: `my` points at this lane's bank of entry 0 of table 0
    const uint8_t *my;
    __device__ __forceinline__ uint32_t operator()(uint32_t i, uint32_t x) const { return *(const uint32_t *)(my + (i << 15) + (x << 7)); }
};

// What a mode body needs of a block cipher: the key schedule and the table images as the host uploads them (Tabs: the four tables of the forward
// direction, 1 024 words; DecTabs: DEC_WORDS words for decryption), the accessor of shared tables, the block calls over a table accessor, and `word`, which turns a 32-bit word as it
// lies in memory into a word of the cipher's state and back (AES: the same word; Camellia: big-endian words, a byte swap).
struct AesCipher {
    using Key = AesKey; using Tabs = AesTabs; using DecTabs = AesDecTabs; using Shared = AesSharedTab;
    static constexpr uint32_t DEC_WORDS = 1280;                       // Td and the inverse S-box
    static __device__ __forceinline__ uint32_t word(uint32_t v) { return v; }
    template <class Tab> static __device__ __forceinline__ void enc(const Tab &t, const Key &k, uint32_t &a, uint32_t &b, uint32_t &c, uint32_t &d) { aes_block(t, k, a, b, c, d); }
    template <class Tab> static __device__ __forceinline__ void dec(const Tab &t, const Key &k, uint32_t &a, uint32_t &b, uint32_t &c, uint32_t &d) { aes_block_inv(t, k, a, b, c, d); }
};
struct CamCipher {                                                    // one network, one table set: the decrypt-order schedule (cam_dec_key) decrypts
    using Key = CamKey; using Tabs = CamTabs; using DecTabs = CamTabs; using Shared = CamSharedTab;
    static constexpr uint32_t DEC_WORDS = 1024;
    static __device__ __forceinline__ uint32_t word(uint32_t v) { return __builtin_bswap32(v); }
    template <class Tab> static __device__ __forceinline__ void enc(const Tab &t, const Key &k, uint32_t &a, uint32_t &b, uint32_t &c, uint32_t &d) { cam_block(t, k, a, b, c, d); }
    template <class Tab> static __device__ __forceinline__ void dec(const Tab &t, const Key &k, uint32_t &a, uint32_t &b, uint32_t &c, uint32_t &d) { cam_block(t, k, a, b, c, d); }
};

// ------------------------------------------------------------------ CTR (Ctr128BE), in place; encrypt == decrypt
// Unit u covers buf[off .. off + len) = stream bytes [pos, pos + len) of the stream whose IV is ivs[iv_idx]; keys != null: the unit's own schedule
// keys[iv_idx] (GCM STREAM: every segment names its stream's key).  Nothing outside a unit's bytes is written.
constexpr uint32_t CTR_THREADS = 1024;
constexpr uint32_t CTR_LDS = 4 * 256 * 32 * 4;                        // four bank-replicated tables: 128 KiB

template <class C>
__device__ __forceinline__ void ctr_body(uint32_t *sR, const CipherUnit *__restrict__ units, uint32_t nunits, const uint8_t *__restrict__ ivs, const typename C::Tabs *__restrict__ tabs,
                                         uint8_t *__restrict__ buf, const typename C::Key key0, const typename C::Key *__restrict__ keys) {
    const uint32_t tid = threadIdx.x;
    {   // thread t owns table entry (t >> 8, t & 255): one global read, 32 bank copies
        const uint32_t v = ((const uint32_t *)tabs)[tid];
        uint32_t *row = sR + (tid << 5);
#pragma unroll
        for (int b = 0; b < 32; b += 4) *(uint4 *)(row + b) = make_uint4(v, v, v, v);
    }
    const BankTab tab{(const uint8_t *)sR + ((tid & 31) << 2)};
    __syncthreads();
    // the table image is built once per workgroup; the workgroups stride over the units
    for (uint32_t ui = blockIdx.x; ui < nunits; ui += gridDim.x) {
        const CipherUnit u = units[ui];
        typename C::Key key = key0;
        if (keys) key = keys[u.iv_idx];                               // (wave-uniform load)
        const uint8_t *ivp = ivs + (size_t)u.iv_idx * 16;
        uint64_t iv_hi = 0, iv_lo = 0;                                // the IV as a 128-bit big-endian number: hi = bytes 0..7, lo = bytes 8..15
        for (int b = 0; b < 8; b++) { iv_hi = (iv_hi << 8) | ivp[b]; iv_lo = (iv_lo << 8) | ivp[8 + b]; }
        const uint64_t b0 = u.pos >> 4;                               // first keystream block of the unit
        const uint64_t end = u.pos + u.len;
        const uint32_t nblk = (uint32_t)(((end + 15) >> 4) - b0);
        const int64_t base = (int64_t)u.off - (int64_t)(u.pos & 15);  // buf offset of keystream block b0's byte 0
        for (uint32_t j = tid; j < nblk; j += CTR_THREADS) {
            const uint64_t lo = iv_lo + b0 + j, hi = iv_hi + (lo < iv_lo ? 1u : 0u);
            // the counter block's memory words are the byte-swapped halves of hi and lo
            uint32_t w0 = C::word(__builtin_bswap32((uint32_t)(hi >> 32))), w1 = C::word(__builtin_bswap32((uint32_t)hi));
            uint32_t w2 = C::word(__builtin_bswap32((uint32_t)(lo >> 32))), w3 = C::word(__builtin_bswap32((uint32_t)lo));
            C::enc(tab, key, w0, w1, w2, w3);
            const uint32_t s0 = C::word(w0), s1 = C::word(w1), s2 = C::word(w2), s3 = C::word(w3);   // as the bytes lie in memory
            const int64_t a = base + (int64_t)j * 16;
            const uint64_t sp = (b0 + j) << 4;                        // stream position of this block
            if (sp >= u.pos && sp + 16 <= end) {
                U4u *q = (U4u *)(buf + a);
                U4u v = *q;
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
// block).  The chain is serial, the loads are not: block b + 1 is requested before block b goes through the rounds.
template <class C>
__device__ __forceinline__ void cbc_enc_body(uint32_t *sT, const CipherUnit *__restrict__ units, uint32_t n, const uint8_t *__restrict__ ivs, const typename C::Tabs *__restrict__ tabs,
                                             uint8_t *__restrict__ buf, const typename C::Key key) {
    for (uint32_t i = threadIdx.x; i < 1024; i += 64) sT[i] = ((const uint32_t *)tabs)[i];
    __syncthreads();
    const typename C::Shared tab{sT};
    const uint32_t e = blockIdx.x * 64 + threadIdx.x;
    if (e >= n) return;
    const CipherUnit u = units[e];
    const U4u iv = *(const U4u *)(ivs + (size_t)u.iv_idx * 16);
    uint32_t c0 = C::word(iv.x), c1 = C::word(iv.y), c2 = C::word(iv.z), c3 = C::word(iv.w);
    const uint32_t nb = u.len / 16 + 1;
    uint8_t *p = buf + u.off;
    U4u nx = {0, 0, 0, 0};
    if (nb > 1) nx = *(const U4u *)p;
    for (uint32_t b = 0; b < nb; b++) {
        uint32_t x0, x1, x2, x3;                                      // the plaintext block as it lies in memory (little-endian words)
        if (b + 1 < nb) {
            x0 = nx.x; x1 = nx.y; x2 = nx.z; x3 = nx.w;
            if (b + 2 < nb) nx = *(const U4u *)(p + 16 * (size_t)(b + 1));
        } else {
            const uint32_t have = u.len - 16 * b, padv = 16 - have;
            uint32_t w[4] = {0, 0, 0, 0};
            for (uint32_t k2 = 0; k2 < 16; k2++) { const uint32_t byte = k2 < have ? p[16 * (size_t)b + k2] : padv; w[k2 >> 2] |= byte << (8 * (k2 & 3)); }
            x0 = w[0]; x1 = w[1]; x2 = w[2]; x3 = w[3];
        }
        c0 ^= C::word(x0); c1 ^= C::word(x1); c2 ^= C::word(x2); c3 ^= C::word(x3);
        C::enc(tab, key, c0, c1, c2, c3);
        U4u o; o.x = C::word(c0); o.y = C::word(c1); o.z = C::word(c2); o.w = C::word(c3);
        *(U4u *)(p + 16 * (size_t)b) = o;
    }
}

// ------------------------------------------------------------------ CBC decryption (read side: DecryptCbcAes256Reader, lib/src/cipher/block/read.rs)
// P_j = D(C_j) ^ C_(j-1), C_(-1) = IV: every block is independent once its predecessor's ciphertext is at hand.  One workgroup per unit, 256 blocks
// per step, in place: a step loads its ciphertext (and the block in front of it) before anything is written, the last ciphertext block of a step is
// carried to the next one through LDS.  The PKCS#7 padding is checked at the unit's end and the plaintext length reported (0xFFFFFFFF: bad length or
// padding -- wrong key or damage).  `key`: the schedule that decrypts (aes256_dec_key: the equivalent inverse cipher, FIPS-197 5.3.5; cam_dec_key).
template <class C>
__device__ __forceinline__ void cbc_dec_body(uint32_t *sT, uint32_t *carry, const CipherUnit *__restrict__ units, const uint8_t *__restrict__ ivs, const typename C::DecTabs *__restrict__ tabs,
                                             uint8_t *__restrict__ buf, const typename C::Key key, uint32_t *__restrict__ plain_len) {
    const uint32_t tid = threadIdx.x;
    for (uint32_t i = tid; i < C::DEC_WORDS; i += 256) sT[i] = ((const uint32_t *)tabs)[i];
    const typename C::Shared tab{sT};
    const CipherUnit u = units[blockIdx.x];
    if (tid == 0) { const U4u iv = *(const U4u *)(ivs + (size_t)u.iv_idx * 16); carry[0] = iv.x; carry[1] = iv.y; carry[2] = iv.z; carry[3] = iv.w; }
    __syncthreads();
    if (u.len == 0 || (u.len & 15)) { if (tid == 0) plain_len[blockIdx.x] = 0xFFFFFFFFu; return; }
    const uint32_t nb = u.len >> 4;
    uint8_t *p = buf + u.off;
    for (uint32_t base = 0; base < nb; base += 256) {
        const uint32_t j = base + tid;
        U4u cj = {0, 0, 0, 0}, pv = {0, 0, 0, 0};
        if (j < nb) {
            cj = *(const U4u *)(p + 16 * (size_t)j);
            if (tid) pv = *(const U4u *)(p + 16 * (size_t)(j - 1)); else { pv.x = carry[0]; pv.y = carry[1]; pv.z = carry[2]; pv.w = carry[3]; }
        }
        __syncthreads();                                             // everyone holds its ciphertext: the step may overwrite it now
        if (j < nb) {
            uint32_t w0 = C::word(cj.x), w1 = C::word(cj.y), w2 = C::word(cj.z), w3 = C::word(cj.w);
            C::dec(tab, key, w0, w1, w2, w3);
            U4u o; o.x = C::word(w0) ^ pv.x; o.y = C::word(w1) ^ pv.y; o.z = C::word(w2) ^ pv.z; o.w = C::word(w3) ^ pv.w;
            *(U4u *)(p + 16 * (size_t)j) = o;
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

// ------------------------------------------------------------------ the six kernels: a mode body per cipher; the kernel owns the LDS (sR: the
// bank-replicated image, CTR_LDS bytes of dynamic LDS; sT: shared tables; carry: CBC decryption's block between two steps) and takes the key by value
extern __shared__ __attribute__((aligned(16))) uint32_t sR[];
__global__ __launch_bounds__(CTR_THREADS)
void k_aes_ctr(const CipherUnit *__restrict__ units, uint32_t nunits, const uint8_t *__restrict__ ivs, const AesTabs *__restrict__ tabs,
               uint8_t *__restrict__ buf, const AesKey key0, const AesKey *__restrict__ keys) { ctr_body<AesCipher>(sR, units, nunits, ivs, tabs, buf, key0, keys); }
__global__ __launch_bounds__(CTR_THREADS)
void k_cam_ctr(const CipherUnit *__restrict__ units, uint32_t nunits, const uint8_t *__restrict__ ivs, const CamTabs *__restrict__ tabs,
               uint8_t *__restrict__ buf, const CamKey key0, const CamKey *__restrict__ keys) { ctr_body<CamCipher>(sR, units, nunits, ivs, tabs, buf, key0, keys); }
__global__ __launch_bounds__(64)
void k_aes_cbc_enc(const CipherUnit *__restrict__ units, uint32_t n, const uint8_t *__restrict__ ivs, const AesTabs *__restrict__ tabs,
                   uint8_t *__restrict__ buf, const AesKey key) { __shared__ uint32_t sT[1024]; cbc_enc_body<AesCipher>(sT, units, n, ivs, tabs, buf, key); }
__global__ __launch_bounds__(64)
void k_cam_cbc_enc(const CipherUnit *__restrict__ units, uint32_t n, const uint8_t *__restrict__ ivs, const CamTabs *__restrict__ tabs,
                   uint8_t *__restrict__ buf, const CamKey key) { __shared__ uint32_t sT[1024]; cbc_enc_body<CamCipher>(sT, units, n, ivs, tabs, buf, key); }
__global__ __launch_bounds__(256)
void k_aes_cbc_dec(const CipherUnit *__restrict__ units, const uint8_t *__restrict__ ivs, const AesDecTabs *__restrict__ tabs,
                   uint8_t *__restrict__ buf, const AesKey key, uint32_t *__restrict__ plain_len) {
    __shared__ uint32_t sT[AesCipher::DEC_WORDS], carry[4];
    cbc_dec_body<AesCipher>(sT, carry, units, ivs, tabs, buf, key, plain_len);
}
__global__ __launch_bounds__(256)
void k_cam_cbc_dec(const CipherUnit *__restrict__ units, const uint8_t *__restrict__ ivs, const CamTabs *__restrict__ tabs,
                   uint8_t *__restrict__ buf, const CamKey key, uint32_t *__restrict__ plain_len) {
    __shared__ uint32_t sT[CamCipher::DEC_WORDS], carry[4];
    cbc_dec_body<CamCipher>(sT, carry, units, ivs, tabs, buf, key, plain_len);
}

// ... and their launchers.  CTR: one workgroup per CU at a time (128 KiB of LDS); a few per CU in the grid even out the ragged units
void launch_aes_ctr(const CipherUnit *units, uint32_t n, const uint8_t *ivs, const AesTabs *tabs, uint8_t *buf, const AesKey &key, const AesKey *keys, hipStream_t st) {
    static const hipError_t attr_set = hipFuncSetAttribute((const void *)k_aes_ctr, hipFuncAttributeMaxDynamicSharedMemorySize, (int)CTR_LDS);   // once, thread-safe
    (void)attr_set;
    if (n) hipLaunchKernelGGL(k_aes_ctr, dim3(n < 1024 ? n : 1024), dim3(CTR_THREADS), CTR_LDS, st, units, n, ivs, tabs, buf, key, keys);
}
void launch_cam_ctr(const CipherUnit *units, uint32_t n, const uint8_t *ivs, const CamTabs *tabs, uint8_t *buf, const CamKey &key, const CamKey *keys, hipStream_t st) {
    static const hipError_t attr_set = hipFuncSetAttribute((const void *)k_cam_ctr, hipFuncAttributeMaxDynamicSharedMemorySize, (int)CTR_LDS);
    (void)attr_set;
    if (n) hipLaunchKernelGGL(k_cam_ctr, dim3(n < 1024 ? n : 1024), dim3(CTR_THREADS), CTR_LDS, st, units, n, ivs, tabs, buf, key, keys);
}
void launch_aes_cbc_enc(const CipherUnit *units, uint32_t n, const uint8_t *ivs, const AesTabs *tabs, uint8_t *buf, const AesKey &key, hipStream_t st) {
    if (n) hipLaunchKernelGGL(k_aes_cbc_enc, dim3((n + 63) / 64), dim3(64), 0, st, units, n, ivs, tabs, buf, key);
}
void launch_cam_cbc_enc(const CipherUnit *units, uint32_t n, const uint8_t *ivs, const CamTabs *tabs, uint8_t *buf, const CamKey &key, hipStream_t st) {
    if (n) hipLaunchKernelGGL(k_cam_cbc_enc, dim3((n + 63) / 64), dim3(64), 0, st, units, n, ivs, tabs, buf, key);
}
void launch_aes_cbc_dec(const CipherUnit *units, uint32_t n, const uint8_t *ivs, const AesDecTabs *tabs, uint8_t *buf, const AesKey &dkey, uint32_t *plain_len, hipStream_t st) {
    if (n) hipLaunchKernelGGL(k_aes_cbc_dec, dim3(n), dim3(256), 0, st, units, ivs, tabs, buf, dkey, plain_len);
}
void launch_cam_cbc_dec(const CipherUnit *units, uint32_t n, const uint8_t *ivs, const CamTabs *tabs, uint8_t *buf, const CamKey &dkey, uint32_t *plain_len, hipStream_t st) {
    if (n) hipLaunchKernelGGL(k_cam_cbc_dec, dim3(n), dim3(256), 0, st, units, ivs, tabs, buf, dkey, plain_len);
}


// ------------------------------------------------------------------ GHASH + tag of AES-GCM (NIST SP 800-38D), one workgroup per segment
// Cipher mode 2 of the reference ("GCM STREAM": GcmEncryptWriter::flush_segment, lib/src/cipher/gcm.rs:45-60 -- AES-256-GCM, 96-bit
// nonce, no associated data, detached 16-byte tag behind the segment).  The CTR part runs in k_aes_ctr (counter block nonce || 2 ...);
// this kernel computes  tag = GHASH_H(ciphertext) ^ E(K, nonce || 1)  over the ciphertext where it stands.
//
// GHASH = sum_i Y_i * H^(N - i) over the blocks Y_0 .. Y_(N-1) = [zero blocks in front (free), ciphertext blocks, length block],
// N a multiple of the 256 lanes.  Lane j runs Horner over Y_j, Y_(j+256), ... with the multiplier H^256 (4-bit table method, the
// table of the 16 nibble multiples of H^256 shared in LDS), then a log-step tree folds the lanes with H, H^2, H^4 .. H^128 (bitwise
// multiplies) and a last multiply by H finishes the sum.  128-bit values are four big-endian words (word 0 = bytes 0..3); "times x"
// is a right shift of that number with 0xE1 << 120 folded in when a bit drops out.
constexpr uint32_t GH_THREADS = 256;
struct G128 { uint32_t a, b, c, d; };
__device__ __forceinline__ G128 gx(const G128 &p, const G128 &q) { return G128{p.a ^ q.a, p.b ^ q.b, p.c ^ q.c, p.d ^ q.d}; }
__device__ __forceinline__ G128 g_mulx(const G128 &v) {
    const uint32_t carry = (0u - (v.d & 1u)) & 0xE1000000u;
    return G128{(v.a >> 1) ^ carry, (v.b >> 1) | (v.a << 31), (v.c >> 1) | (v.b << 31), (v.d >> 1) | (v.c << 31)};
}
__device__ G128 g_mul_bitwise(const G128 &x, G128 v) {                 // x * v, 128 conditional adds
    G128 z{0, 0, 0, 0};
    const uint32_t xw[4] = {x.a, x.b, x.c, x.d};
    for (int w = 0; w < 4; w++)
        for (int b = 31; b >= 0; b--) {
            const uint32_t m = 0u - ((xw[w] >> b) & 1u);
            z.a ^= v.a & m; z.b ^= v.b & m; z.c ^= v.c & m; z.d ^= v.d & m;
            v = g_mulx(v);
        }
    return z;
}
__device__ __forceinline__ uint32_t be32(uint32_t v) { return __builtin_bswap32(v); }

// PER (read side only): one verdict word per segment (bad[segment] = 1 when its tag does not match, 0 otherwise) instead of the shared counter
template <bool PER = false>
__global__ __launch_bounds__(GH_THREADS)
void k_gcm_tag(const GcmEntry *__restrict__ ents, uint8_t *__restrict__ buf, const uint8_t *__restrict__ expect, uint32_t *__restrict__ bad) {
    __shared__ G128 sM[16];                  // nibble multiples of H^256: sM[8] = H^256, sM[4] = H^256 x, sM[2], sM[1], the rest by addition
    __shared__ uint32_t sR[16];              // what the four bits dropped by a 4-bit shift fold back into the top 16 bits
    __shared__ G128 sHp[9];                  // H^(2^k), k = 0..8
    __shared__ G128 sAcc[GH_THREADS];
    const uint32_t tid = threadIdx.x;
    const GcmEntry e = ents[blockIdx.x];
    if (tid == 0) {
        G128 h{e.h[0], e.h[1], e.h[2], e.h[3]};
        sHp[0] = h;
        for (int k = 1; k <= 8; k++) { h = g_mul_bitwise(h, h); sHp[k] = h; }
        G128 m = h;                                                    // H^256
        sM[0] = G128{0, 0, 0, 0};
        sM[8] = m; m = g_mulx(m); sM[4] = m; m = g_mulx(m); sM[2] = m; m = g_mulx(m); sM[1] = m;
        for (int i = 2; i <= 8; i <<= 1) for (int j = 1; j < i; j++) sM[i + j] = gx(sM[i], sM[j]);
    }
    if (tid < 16) {
        uint32_t r = 0;
        for (int p = 0; p < 4; p++) if ((tid >> p) & 1) r ^= 0xE100u >> (3 - p);
        sR[tid] = r << 16;
    }
    __syncthreads();
    const uint32_t m = (e.len + 15) / 16;                              // ciphertext blocks; block m is the length block
    const uint32_t N = (m + 1 + GH_THREADS - 1) / GH_THREADS * GH_THREADS;
    const uint32_t pad = N - (m + 1);                                  // zero blocks in front
    const uint8_t *ct = buf + e.off;
    G128 acc{0, 0, 0, 0};
    for (uint32_t i = tid; i < N; i += GH_THREADS) {
        // acc = acc * H^256 (table method: 32 nibbles of acc, last nibble first), then + Y_i
        {
            const uint32_t xw[4] = {acc.a, acc.b, acc.c, acc.d};
            G128 z{0, 0, 0, 0};
#pragma unroll
            for (int n = 0; n < 32; n++) {                             // nibble n: n = 0 is the low nibble of byte 15
                const uint32_t nib = (xw[3 - (n >> 3)] >> (4 * (n & 7))) & 0xF;
                if (n) {
                    const uint32_t rem = z.d & 0xF;
                    z.d = (z.d >> 4) | (z.c << 28); z.c = (z.c >> 4) | (z.b << 28); z.b = (z.b >> 4) | (z.a << 28); z.a = (z.a >> 4) ^ sR[rem];
                }
                const G128 t = sM[nib];
                z.a ^= t.a; z.b ^= t.b; z.c ^= t.c; z.d ^= t.d;
            }
            acc = z;
        }
        if (i >= pad) {
            const uint32_t bi = i - pad;
            if (bi < m) {
                const uint64_t o = (uint64_t)bi * 16;
                if (o + 16 <= e.len) { const U4u v = *(const U4u *)(ct + o); acc.a ^= be32(v.x); acc.b ^= be32(v.y); acc.c ^= be32(v.z); acc.d ^= be32(v.w); }
                else {
                    uint32_t w[4] = {0, 0, 0, 0};
                    for (uint32_t k = 0; o + k < e.len; k++) w[k >> 2] |= (uint32_t)ct[o + k] << (24 - 8 * (k & 3));
                    acc.a ^= w[0]; acc.b ^= w[1]; acc.c ^= w[2]; acc.d ^= w[3];
                }
            } else {                                                   // len(A) = 0 || len(C) in bits
                const uint64_t bits = (uint64_t)e.len * 8;
                acc.c ^= (uint32_t)(bits >> 32); acc.d ^= (uint32_t)bits;
            }
        }
    }
    // fold the lanes: P = sum_j acc_j * H^(255 - j)
    sAcc[tid] = acc;
    __syncthreads();
    for (uint32_t k = 0; k < 8; k++) {
        const uint32_t st = 1u << k;
        if ((tid & (2 * st - 1)) == 0) sAcc[tid] = gx(g_mul_bitwise(sAcc[tid], sHp[k]), sAcc[tid + st]);
        __syncthreads();
    }
    if (tid == 0) {
        const G128 s = g_mul_bitwise(sAcc[0], sHp[0]);
        U4u t; t.x = be32(s.a ^ e.ej0[0]); t.y = be32(s.b ^ e.ej0[1]); t.z = be32(s.c ^ e.ej0[2]); t.w = be32(s.d ^ e.ej0[3]);
        if (expect) {                                                  // read side: the tag is compared, nothing is written
            const U4u x = *(const U4u *)(expect + 16 * (size_t)blockIdx.x);
            const bool mism = ((t.x ^ x.x) | (t.y ^ x.y) | (t.z ^ x.z) | (t.w ^ x.w)) != 0;
            if (PER) bad[blockIdx.x] = mism ? 1u : 0u;
            else if (mism) atomicAdd(bad, 1u);
        } else *(U4u *)(buf + e.off + e.len) = t;
    }
}

void launch_gcm_tag(const GcmEntry *ents, uint32_t n, uint8_t *buf, hipStream_t st) {
    if (n) hipLaunchKernelGGL(k_gcm_tag<false>, dim3(n), dim3(GH_THREADS), 0, st, ents, buf, (const uint8_t *)nullptr, (uint32_t *)nullptr);
}
void launch_gcm_verify(const GcmEntry *ents, uint32_t n, const uint8_t *buf, const uint8_t *expect, uint32_t *bad, hipStream_t st) {
    if (n) hipLaunchKernelGGL(k_gcm_tag<false>, dim3(n), dim3(GH_THREADS), 0, st, ents, const_cast<uint8_t *>(buf), expect, bad);
}
// `pna verify`: every segment's tag checked, one verdict word per segment in verdict[0 .. n)
void launch_gcm_verdict(const GcmEntry *ents, uint32_t n, const uint8_t *buf, const uint8_t *expect, uint32_t *verdict, hipStream_t st) {
    if (n) hipLaunchKernelGGL(k_gcm_tag<true>, dim3(n), dim3(GH_THREADS), 0, st, ents, const_cast<uint8_t *>(buf), expect, verdict);
}

} // namespace pna
