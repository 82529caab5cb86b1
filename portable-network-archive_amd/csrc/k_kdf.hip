// k_kdf.hip -- pna_gpu_kdf_batch's kernels: the block fill of Argon2 (RFC 9106; d / i / id, version 0x13) and the PBKDF2-HMAC-SHA256 chain, for a
// batch of independent jobs (one password, one salt and parameter set per job).  H0, the two seed blocks per Argon2 lane, the final H', HMAC's pad states
// and U_1 are host work (kdf_core.h, pna_kdf.cpp): BLAKE2b over a few hundred bytes per job against a fill of m x t blocks.
//
// k_argon2_fill.  One Argon2 lane of one job is filled by a GROUP of 32 wave lanes, so a wave carries two groups; a 1 KiB block is 128 words of 64 bits
// and every wave lane holds four of them.  The block just computed stays in registers: it is the next step's `prev`.  A step:
//     J1 | J2          word 0 of prev (one cross-lane read from the group's first lane), or a word of the address block (LDS) in the data-independent slices
//     ref              kdf_argon_ref (kdf_core.h) -> one 1 KiB read, four 8-byte loads per wave lane
//     R = prev ^ ref   keep = R (^ the block's old value from pass 1 on: a second 1 KiB read)
//     P on the rows    wave lane (row, j) of the group holds v[j], v[4 + j], v[8 + j], v[12 + j] of its row of 16 words: the column step of the BLAKE2b round
//                      is one kdf_quarter per wave lane, the diagonal step the same after b, c, d moved by 1, 2, 3 lanes inside the quad (DPP quad_perm)
//     transpose        through the group's 1 KiB of LDS: written by rows, read by columns (column c, words 2 c and 2 c + 1 of every row)
//     P on the columns as on the rows; transposed back
//     next = R' ^ keep one 1 KiB write; it stays in registers as prev
// A group's LDS is touched by its own wave only, so a wave-level fence orders the transpose; nothing waits for another wave.
// Jobs with one Argon2 lane: workgroups of one wave, two jobs each (<false>).  Jobs with p > 1 lanes: one workgroup per job, p groups (<true>; one launch per
// value of p, so every wave lane of a workgroup runs the same loops), and a workgroup barrier at the end of every slice -- a reference into another lane
// reads only slices that are complete (kdf_argon_ref), and those were written by waves of this workgroup before the barrier.
//
// k_pbkdf2_sha256.  One wave lane per job: U_1 .. U_c and the running XOR in registers, two SHA-256 compressions per round from the precomputed pad states.
#include <hip/hip_runtime.h>
#include "kdf_core.h"

namespace pna {

// x of the quad's lane (j + K) & 3, for lane j
template <int K>
static __device__ __forceinline__ uint64_t quad_rot(uint64_t x) {
    constexpr int ctrl = K == 1 ? 0x39 : K == 2 ? 0x4E : 0x93;      // quad_perm [1,2,3,0] / [2,3,0,1] / [3,0,1,2]
    const int lo = __builtin_amdgcn_mov_dpp((int)(uint32_t)x, ctrl, 0xF, 0xF, true);
    const int hi = __builtin_amdgcn_mov_dpp((int)(uint32_t)(x >> 32), ctrl, 0xF, 0xF, true);
    return (uint64_t)(uint32_t)lo | ((uint64_t)(uint32_t)hi << 32);
}
// P over 16 words held by a quad, lane j: v[j], v[4 + j], v[8 + j], v[12 + j]
static __device__ __forceinline__ void quad_perm16(uint64_t r[4]) {
    kdf_quarter(r[0], r[1], r[2], r[3]);
    r[1] = quad_rot<1>(r[1]); r[2] = quad_rot<2>(r[2]); r[3] = quad_rot<3>(r[3]);
    kdf_quarter(r[0], r[1], r[2], r[3]);
    r[1] = quad_rot<3>(r[1]); r[2] = quad_rot<2>(r[2]); r[3] = quad_rot<1>(r[3]);
}
// the group's LDS accesses of one wave, ordered: what was written before is read after
static __device__ __forceinline__ void group_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}
// r, in the row layout (wave lane t of the group, slot s: word 16 (t >> 2) + (t & 3) + 4 s), through P on rows and columns; pad: the group's 128 words of LDS
static __device__ __forceinline__ void group_p(uint64_t r[4], uint64_t *pad, uint32_t t) {
    const uint32_t q = t >> 2, j = t & 3;
    quad_perm16(r);
    group_sync();                                                // (the pad's last readers are done)
#pragma unroll
    for (int s = 0; s < 4; s++) pad[16 * q + j + 4 * s] = r[s];
    group_sync();
#pragma unroll
    for (int s = 0; s < 4; s++) { const uint32_t i = j + 4 * s; r[s] = pad[16 * (i >> 1) + 2 * q + (i & 1)]; }      // column q: v[i] = word 2 q + (i & 1) of row i / 2
    quad_perm16(r);
    group_sync();
#pragma unroll
    for (int s = 0; s < 4; s++) { const uint32_t i = j + 4 * s; pad[16 * (i >> 1) + 2 * q + (i & 1)] = r[s]; }
    group_sync();
#pragma unroll
    for (int s = 0; s < 4; s++) r[s] = pad[16 * q + j + 4 * s];
}

template <bool MULTI>
__global__ __launch_bounds__(MULTI ? 512 : 64)
void k_argon2_fill(const KdfArgonJob *__restrict__ jobs, uint32_t njobs, uint64_t *mem, const uint64_t *__restrict__ seeds, uint64_t *__restrict__ fin) {
    __shared__ uint64_t lds[MULTI ? 16 : 2][2][128];            // per group: the transpose pad, the address block
    const uint32_t t = threadIdx.x & 31, grp = threadIdx.x >> 5;
    const uint32_t job = MULTI ? blockIdx.x : blockIdx.x * 2 + grp, lane = MULTI ? grp : 0;
    if (job >= njobs) return;                                    // (<false> only: the odd job's other half wave; no workgroup barrier there)
    const KdfArgonJob jb = jobs[job];
    const KdfArgonGeom g = jb.g;
    if (MULTI && lane >= g.lanes) return;                        // (never: the launch has 32 g.lanes threads per workgroup)
    uint64_t *pad = lds[grp][0], *addr = lds[grp][1];
    uint64_t *base = mem + jb.mem_off * 128;
    uint32_t w[4];                                               // the words this wave lane holds of every block
#pragma unroll
    for (int s = 0; s < 4; s++) w[s] = 16 * (t >> 2) + (t & 3) + 4 * s;
    uint64_t prev[4];
    {   // the seed blocks go to columns 0 and 1; the second is the first step's prev
        const uint64_t *sd = seeds + (size_t)(jb.lane0 + lane) * 256;
        uint64_t *b0 = base + (size_t)lane * g.lane_len * 128;
#pragma unroll
        for (int s = 0; s < 4; s++) { b0[w[s]] = sd[w[s]]; prev[s] = sd[128 + w[s]]; b0[128 + w[s]] = prev[s]; }
    }
    if (MULTI) __syncthreads();
    for (uint32_t pass = 0; pass < g.t_cost; pass++)
        for (uint32_t slice = 0; slice < 4; slice++) {
            const bool indep = kdf_argon_indep(g, pass, slice);
            for (uint32_t i = kdf_argon_first(pass, slice); i < g.seg; i++) {
                if (indep && ((i & 127) == 0 || (i == 2 && pass == 0 && slice == 0))) {      // the next 128 columns' address block: G(0, G(0, input))
                    uint64_t r[4], k[4];
#pragma unroll
                    for (int s = 0; s < 4; s++) { r[s] = w[s] < 7 ? kdf_argon_addr_input(g, pass, slice, lane, i / 128 + 1, (int)w[s]) : 0; k[s] = r[s]; }
                    group_p(r, pad, t);
#pragma unroll
                    for (int s = 0; s < 4; s++) { r[s] ^= k[s]; k[s] = r[s]; }
                    group_p(r, pad, t);
                    group_sync();
#pragma unroll
                    for (int s = 0; s < 4; s++) addr[w[s]] = r[s] ^ k[s];
                    group_sync();
                }
                uint64_t rnd;
                if (indep) rnd = addr[i & 127];
                else {
                    const int src = (int)(threadIdx.x & 32);     // the group's first wave lane holds word 0
                    rnd = (uint64_t)(uint32_t)__shfl((int)(uint32_t)prev[0], src, 64) | ((uint64_t)(uint32_t)__shfl((int)(uint32_t)(prev[0] >> 32), src, 64) << 32);
                }
                uint32_t rl, rc;
                kdf_argon_ref(g, pass, slice, lane, i, rnd, rl, rc);
                const uint64_t *ref = base + ((size_t)rl * g.lane_len + rc) * 128;
                uint64_t *cur = base + ((size_t)lane * g.lane_len + slice * g.seg + i) * 128;
                uint64_t r[4], keep[4];
#pragma unroll
                for (int s = 0; s < 4; s++) { r[s] = prev[s] ^ ref[w[s]]; keep[s] = r[s]; }
                if (pass) {
#pragma unroll
                    for (int s = 0; s < 4; s++) keep[s] ^= cur[w[s]];
                }
                group_p(r, pad, t);
#pragma unroll
                for (int s = 0; s < 4; s++) { prev[s] = r[s] ^ keep[s]; cur[w[s]] = prev[s]; }
            }
            if (MULTI) __syncthreads();                          // the slice is complete in every lane before any lane refers to it
        }
    uint64_t *out = fin + (size_t)(jb.lane0 + lane) * 128;      // the lane's last block: the host XORs the lanes and runs H'
#pragma unroll
    for (int s = 0; s < 4; s++) out[w[s]] = prev[s];
}

__global__ __launch_bounds__(64)
void k_pbkdf2_sha256(const KdfPbkdf2Job *__restrict__ jobs, uint32_t njobs, uint32_t *__restrict__ out) {
    const uint32_t j = blockIdx.x * 64 + threadIdx.x;
    if (j >= njobs) return;
    const KdfPbkdf2Job jb = jobs[j];
    uint32_t tw[8];
    kdf_pbkdf2_chain(jb.s.istate, jb.s.ostate, jb.s.u1, jb.rounds, tw);
#pragma unroll
    for (int i = 0; i < 8; i++) out[8 * j + i] = tw[i];
}

// jobs: njobs of ONE lane count p (1 .. 16), in device memory
void launch_argon2_fill(const KdfArgonJob *jobs, uint32_t njobs, uint32_t p, uint64_t *mem, const uint64_t *seeds, uint64_t *fin, hipStream_t st) {
    if (!njobs) return;
    if (p == 1) hipLaunchKernelGGL(k_argon2_fill<false>, dim3((njobs + 1) / 2), dim3(64), 0, st, jobs, njobs, mem, seeds, fin);
    else hipLaunchKernelGGL(k_argon2_fill<true>, dim3(njobs), dim3(32 * p), 0, st, jobs, njobs, mem, seeds, fin);
}
void launch_pbkdf2_sha256(const KdfPbkdf2Job *jobs, uint32_t njobs, uint32_t *out, hipStream_t st) {
    if (njobs) hipLaunchKernelGGL(k_pbkdf2_sha256, dim3((njobs + 63) / 64), dim3(64), 0, st, jobs, njobs, out);
}

}
