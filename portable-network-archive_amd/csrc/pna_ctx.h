// pna_host.cpp -- host side of libpna_gpu.so: context, workspace, batch planning and the C ABI of
// include/pna_gpu.h.  Mirrors the construction/finish protocol of the reference's CompressionWriter
// (lib/src/compress.rs:21-76, lib/src/entry/write.rs:251-265) and the per-entry fan-out of
// cli/src/command/core.rs:496-537.  No CPU compression path exists here: everything goes through the HIP kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include <algorithm>
#include <thread>
#include <mutex>
#include <condition_variable>
#include <atomic>
#include <chrono>
#include <new>
#include <functional>
#include <memory>
#include <sys/random.h>
#include "pna_dev.h"
#include "camellia_core.h"
#include "../../include/pna_gpu.h"
#include "../../include/pna_archive.h"

struct XzScan; struct XzBlock;     // xz_core.h
struct KdfArgonJob; struct KdfPbkdf2Job;     // kdf_core.h
namespace pna {
void launch_lz(const LzLaunch &L);                    // k_lz.hip: every form but Small (pna_dev.h LzLaunch)
void launch_lz_small(const LzLaunch &L, bool w3);     // k_lz_split.hip: the short segments behind a one-kernel launch; w3: words of three bytes
uint32_t lz_gtab_log();
void launch_deflate_stage1(const uint8_t *src, const SegDesc *segs, uint32_t nseg, const uint32_t *blk_seg, uint32_t nblk,
                           const uint64_t *seqs, const uint8_t *lits, BlkInfo *blk, const uint4 *ctab, DeflTables *tabs, uint8_t *outc,
                           uint64_t *seg_size, uint64_t *seg_off, hipStream_t st, hipEvent_t *ev, uint32_t dbg, bool stored_only, bool wave_per_seg);
void launch_deflate_write(const uint8_t *src, const SegDesc *segs, const uint32_t *blk_seg, uint32_t nblk, const BlkInfo *blk,
                          const uint64_t *seg_off, const uint64_t *seg_size, const uint8_t *outc, const uint32_t *entry_seg, uint32_t nentry,
                          uint8_t *dst, hipStream_t st, bool stored_only, bool small_blocks);
// (k_deflate.hip) one window of a zlib stream compressed in windows: k_dwrite, then k_dfold (header / trailer by the window's place, the Adler-32 carry).
// A weak reference: the sanitizer build of the host code (tests/san) links its own stand-ins for the launch layer and has none for it -- write_stage
// refuses a deflate window when it is absent; the library always defines it.
__attribute__((weak)) void launch_deflate_write_run(const uint8_t *src, const SegDesc *segs, const uint32_t *blk_seg, uint32_t nblk, const BlkInfo *blk,
                                                    const uint64_t *seg_off, const uint64_t *seg_size, const uint8_t *outc, const uint32_t *entry_seg,
                                                    uint8_t *dst, hipStream_t st, bool stored_only, bool small_blocks, uint32_t *adler_carry, uint32_t run);
void launch_entropy_chunk(const SegDesc *segs, uint32_t s0, uint32_t ns, const uint32_t *blk_seg, uint32_t g0, uint32_t nb,
                          const uint64_t *seqs, const uint8_t *lits, BlkInfo *blk, SegTables *tabs, uint8_t *litc, uint8_t *seqc, uint32_t *seqw,
                          uint32_t flags, uint32_t blk_log, uint32_t *hist, hipStream_t st, hipEvent_t *ev, hipStream_t side, hipEvent_t fork, hipEvent_t join, bool single_block, const uint32_t *seq_hist);
void launch_default_tables(hipStream_t st);   // k_entropy.hip: the predefined sequence tables, once per device
void launch_plan(const SegDesc *segs, uint32_t nseg, BlkInfo *blk, const SegTables *tabs, uint64_t *seg_size, uint64_t *seg_off,
                 uint32_t flags, hipStream_t st);
void launch_write(const uint8_t *src, const SegDesc *segs, uint32_t nseg, const uint32_t *blk_seg, uint32_t nblk, const BlkInfo *blk,
                  const SegTables *tabs, const uint64_t *seg_off, const uint8_t *lits, const uint8_t *litc,
                  const uint8_t *seqc, uint8_t *dst, bool any_empty, hipStream_t st, bool small_blocks);
void lz_read_stamps(unsigned long long *out);
void launch_frame(const FrameDesc *fd, uint32_t nentry, const uint8_t *blob, const CrcTabs *ct, uint8_t *dst, uint64_t cap16,
                  uint32_t fend_crc, const char ty[4], bool with_fend, hipStream_t st, uint32_t max_payload);
void launch_place(const void *pd, uint32_t n, const uint8_t *src, uint8_t *dst, hipStream_t st);
void launch_gather(const void *pd, uint32_t n, const uint8_t *src, uint8_t *dst, hipStream_t st);
// Compression::No (k_store.hip; weak like launch_diff: the sanitizer build has no stand-ins for them, and without them PNA_ALGO_STORE stays unsupported on the
// archive entry points).  pieces: StorePiece x n; with_crc: the fused form, states[i] = the raw CRC register of piece i; chunks: StoreChunk x n
__attribute__((weak)) void launch_store(const void *pieces, uint32_t n, const uint8_t *src, uint8_t *dst, const CrcTabs *ct, uint32_t *states, bool with_crc, hipStream_t st);
// (sd_ch != 0: the inner records of a stored solid stream -- StoreChunk::crc_off counts in the stream, whose position p stands at sd_base + p + sd_ovh * (p / sd_ch) of dst)
__attribute__((weak)) void launch_store_fold(const void *chunks, uint32_t n, const uint32_t *states, const void *pieces, const char ty[4], uint32_t fend_crc, uint8_t *dst, hipStream_t st,
                                             uint64_t sd_base = 0, uint64_t sd_ch = 0, uint64_t sd_ovh = 0);
void launch_link_copy(const uint8_t *src, uint8_t *dst, size_t n, uint32_t wgs, hipStream_t st);
void launch_link_gather(const void *segs, uint32_t nseg, uint32_t wgs, hipStream_t st);   // k_frame.hip: {src, dst, len} x nseg, page-locked sources
void launch_layout(FrameDesc *fd, uint8_t *blob, const uint32_t *entry_seg, const uint64_t *seg_off, uint32_t nentry, uint32_t nseg, uint64_t out_base,
                   uint64_t *segdst, uint64_t *ent_off, uint64_t *total, hipStream_t st);
void launch_frame_pieces(const FrameDesc *fd, uint32_t n, const CrcTabs *ct, const uint8_t *buf, uint64_t cap16, const char ty[4], uint32_t *states, hipStream_t st);
struct CrcPatchH { int64_t off; uint32_t crc, mask; };   // = CrcPatch of k_frame.hip
void launch_crc_patch(const void *patches, uint32_t n, uint8_t *dst, hipStream_t st);
void launch_frame_verify(const FrameDesc *fd, uint32_t n, const CrcTabs *ct, const uint8_t *buf, uint64_t cap16, const char ty[4], uint32_t *verify, hipStream_t st, uint32_t max_payload);
// `pna verify`'s kernels (weak: the sanitizer build has no stand-ins for them, pna_gpu_verify_archive_host refuses to run there)
__attribute__((weak)) void launch_frame_verdict(const FrameDesc *fd, uint32_t n, const CrcTabs *ct, const uint8_t *buf, uint64_t cap16, const char ty[4], uint32_t *verdict, hipStream_t st, uint32_t max_payload);
__attribute__((weak)) void launch_verdict(const VerdictEnt *ve, uint32_t n, const uint32_t *crc_v, const uint32_t *gcm_v, const uint32_t *cbc_plen, uint32_t *out, hipStream_t st);
// `pna diff`'s kernel (k_diff.hip; weak like the verdict kernels: pna_gpu_diff_archive_host refuses to run without it)
__attribute__((weak)) void launch_diff(const DiffPiece *pieces, uint32_t npieces, uint32_t ntiles, const uint8_t *a, const uint8_t *b, unsigned long long *first, hipStream_t st);
// pna_gpu_extract_select_host's kernel (k_pick.hip; weak like launch_diff: the entry point refuses to run without it)
__attribute__((weak)) void launch_pick(const PickPiece *pieces, uint32_t npieces, uint32_t ntiles, const uint8_t *src, hipStream_t st);
// Compression::XZ, decode only (k_xz.hip; weak like launch_diff: without them xz stays "not decoded on the device").  streams: XzStreamInH x n (pna_decode.cpp);
// launch_xzscan with blocks == null counts, otherwise writes the block descriptors and the check kernel's piece list
__attribute__((weak)) void launch_xzscan(const void *streams, uint32_t n, const uint8_t *src, XzScan *out, XzBlock *blocks, void *pieces, hipStream_t st);
__attribute__((weak)) void launch_lzma2(XzBlock *blocks, uint32_t nblk, const uint8_t *src, uint8_t *dst, uint32_t lclp, hipStream_t st);
__attribute__((weak)) void launch_xzcheck(const void *pieces, uint32_t npieces, const XzBlock *blocks, uint32_t nblk, const uint8_t *src, const uint8_t *dst, uint64_t *acc,
                                          uint32_t *stream_status, hipStream_t st);
// Compression::XZ on the write side (k_xzenc.hip; weak like the decoder's: the sanitizer build has no stand-ins for them, and without them PNA_ALGO_XZ stays unsupported
// on the compress entry points).  max_seg: the longest segment's bytes; work: 2 * nseg 64-bit words (the blocks' unpadded sizes, the CRC64 accumulators)
__attribute__((weak)) void launch_xzenc_stage(const uint8_t *src, const SegDesc *segs, uint32_t nseg, uint32_t max_seg, const uint32_t *blk_seg, uint32_t nblk, const uint64_t *seqs, BlkInfo *blk,
                                              uint8_t *scratch, uint64_t *work, uint64_t *seg_size, uint64_t *seg_off, hipStream_t st, hipEvent_t *ev);
__attribute__((weak)) void launch_xzenc_write(const uint8_t *src, const SegDesc *segs, const uint32_t *blk_seg, uint32_t nblk, const BlkInfo *blk, const uint64_t *seg_off,
                                              const uint64_t *seg_size, const uint8_t *scratch, const uint64_t *work, uint32_t nseg, const uint32_t *entry_seg, uint32_t nentry,
                                              uint8_t *dst, hipStream_t st, bool small_blocks);
// pna_gpu_kdf_batch's kernels (k_kdf.hip; weak like launch_diff: the entry point refuses to run without them).  jobs: of ONE Argon2 lane count p
__attribute__((weak)) void launch_argon2_fill(const KdfArgonJob *jobs, uint32_t njobs, uint32_t p, uint64_t *mem, const uint64_t *seeds, uint64_t *fin, hipStream_t st);
__attribute__((weak)) void launch_pbkdf2_sha256(const KdfPbkdf2Job *jobs, uint32_t njobs, uint32_t *out, hipStream_t st);
// pna_kdf.cpp: pna_gpu_kdf_batch without the argument checks; add: the counters of pna_gpu_debug_kdf_stats go on from where they stand (weak: the sanitizer build of the host code does not hold it; the drivers derive on the host there)
__attribute__((weak)) int kdf_batch(pna_gpu_ctx *c, const void *password, size_t password_len, size_t n, const pna_kdf_job *jobs, uint8_t *keys, int *status, hipStream_t st, bool add);
inline bool xz_kernels_present() { return launch_xzscan && launch_lzma2 && launch_xzcheck; }
// pna_decode.cpp: which stream of an xz decode call failed and why (the call's error text is "entry <index>: <reason>"), for a caller that knows its streams by name
struct XzFail { size_t index = ~(size_t)0; std::string reason; };
void launch_zdec(ZFrame *frames, uint32_t n, const uint8_t *src, uint8_t *dst, uint8_t *lit_scratch, uint32_t dbg, hipStream_t st);
void launch_zxxh(ZFrame *frames, uint32_t n, const uint8_t *src, const uint8_t *dst, hipStream_t st);
void launch_zscan(const ZEntry *ents, uint32_t n, const uint8_t *src, ZFrame *frames, ZFrameX *fx, hipStream_t st);
void launch_zcount(const ZEntry *ents, uint32_t n, const uint8_t *src, uint32_t *counts, hipStream_t st);
void launch_zlist(const uint8_t *src, uint64_t base, uint64_t len, uint64_t ip0, void *items, uint32_t cap, uint64_t *hdr, hipStream_t st);   // items: {off, len, fcs} x cap (24 B each)
// (k_zdec.hip) the decoded size of one zstd payload from its frame and block headers: out = {size or bound, exact, malformed, frames, last frame's share}.  A weak reference like
// launch_deflate_write_run: the sanitizer build has no stand-in for it, pna_gpu_open_size_device refuses zstd there.
__attribute__((weak)) void launch_zsize(const uint8_t *src, uint64_t base, uint64_t len, unsigned long long *out, hipStream_t st);
void launch_zparse(ZFrame *frames, ZFrameX *fx, uint32_t n, const uint8_t *src, ZBlock *blocks, ZTables *tabs, uint32_t *huf_list, uint32_t *seq_list,
                   void *work, hipStream_t st);
void launch_zparse_big_a(ZFrame *frames, ZFrameX *fx, const uint32_t *big_list, uint32_t nbig, const uint8_t *src, ZBlock *blocks, uint32_t *one_list, void *work, hipStream_t st);
void launch_zparse_big_b(ZFrame *frames, ZFrameX *fx, uint32_t nblocks, const uint8_t *src, ZBlock *blocks, ZTables *tabs, uint32_t *huf_list, uint32_t *seq_list,
                         void *work, const uint32_t *one_list, hipStream_t st);
void launch_zstreams(uint32_t n_huf, uint32_t n_seq, const uint32_t *huf_list, const uint32_t *seq_list, const void *work, ZBlock *blocks,
                     const ZFrame *frames, const ZTables *tabs, const uint8_t *src, uint8_t *lit_scratch, uint64_t *seqs, hipStream_t st);
// pna_decode.cpp: the measurement behind pna_gpu_open_size_device (zstd: also its frames and the last frame's share of the size)
struct OpenSize { uint64_t size = 0; int exact = 0; uint64_t frames = 0, last = 0; };
int open_size(pna_gpu_ctx *c, int algo, const void *d_src, uint64_t src_off, uint64_t src_len, OpenSize *out, hipStream_t st);
// pna_decode.cpp: what one decode call decodes -- n streams of one codec, all in d_src, decoded into d_dst -- and the one way to the codecs' decoders.  decode_batch is internal: it
// checks no pointer, the caller has set the device (hipSetDevice) and names the stream (the exports do all three before they call it).
struct DecodeBatch {
    size_t n; const void *d_src; const uint64_t *src_off, *src_len; void *d_dst; const uint64_t *dst_off, *raw_len;   // raw_len: the size, or with `open` the room
    bool open = false; uint64_t *raw_out = nullptr;   // open: the sizes are recorded nowhere; raw_out: the sizes found
    uint32_t *ent_status = nullptr; hipStream_t st;   // ent_status, verdict mode: one status per stream (ZFrame::status) instead of a failing call
    const OpenSize *plan = nullptr;                   // zstd, n = 1, open: the stream's measurement -- frames of 1 MiB but the last, which gets plan->last bytes (the rest of the room only if the stream is not of that shape)
};
int decode_batch(pna_gpu_ctx *c, int algo, const DecodeBatch &b, XzFail *why = nullptr);
struct ISChunkH { uint64_t start_bit, end_bit, lit_base, out_base, rec_base, end_found, mtot; uint32_t nlit, nrec, status, adler; };   // = ISChunk of k_inflate.hip
static_assert(sizeof(ISChunkH) == 72, "ISChunk layout");
void launch_ispec(const uint8_t *src, uint64_t src_off, uint64_t src_len, uint32_t cbytes, uint32_t nchunks, uint64_t *start, hipStream_t st);
void launch_inflate_chunks(ZFrame *frames, ZFrameX *fx, uint32_t frame, void *chunks, uint32_t nchunks, uint32_t emit, const uint8_t *src, ZBlock *blocks,
                           uint8_t *lit_scratch, uint64_t *seqs, hipStream_t st);
void launch_inflate(ZFrame *frames, ZFrameX *fx, uint32_t n, const uint8_t *src, ZBlock *blocks, uint8_t *lit_scratch, uint64_t *seqs, const uint32_t *mode, hipStream_t st);
void launch_icount(const uint8_t *src, const uint64_t *off, const uint64_t *len, uint32_t n, uint32_t *count, uint32_t G, hipStream_t st);
void launch_vinflate(ZFrame *frames, ZFrameX *fx, uint32_t n, const void *pieces, uint32_t npieces, uint64_t *pb, uint32_t *mode, uint32_t *cntg, uint32_t G, const uint8_t *src,
                     ZBlock *blocks, uint8_t *lit_scratch, uint64_t *seqs, hipStream_t st);
void launch_iadler(ZFrame *frames, const ZFrameX *fx, const ZBlock *blocks, uint32_t n, const uint32_t *cbase, uint32_t npieces, const uint8_t *dst,
                   void *part, hipStream_t st);
void launch_zexec_groups(ZFrame *frames, const ZFrameX *fx, uint32_t n, ZBlock *blocks, const void *pieces, uint32_t npieces, const uint8_t *src, const uint8_t *lit_scratch,
                         const uint64_t *seqs, uint8_t *dst, hipStream_t st);
struct ZxFrame { uint64_t dst_off, dst_len; uint32_t blk_base, nblk, status, unresolved; };      // k_zexec_par.hip
int launch_zexec_par(ZxFrame *zf, const ZxFrame &h, const ZBlock *blocks, const uint8_t *src, const uint8_t *lit_scratch, uint64_t *seqs, uint32_t *rep_scratch,
                     uint32_t *words, uint8_t *dst, uint32_t *status_out, uint32_t *rounds_out, hipStream_t st,
                     uint32_t nwin, const uint32_t *win_blk, const uint64_t *win_off);
void launch_zexec(ZFrame *frames, const ZFrameX *fx, uint32_t n, ZBlock *blocks, const uint8_t *src, const uint8_t *lit_scratch,
                  const uint64_t *seqs, uint8_t *dst, hipStream_t st);
std::string pna_sanitize_name(const char *name, size_t n);
// the chunk stream of an archive (pna_archive.cpp): the signature, big-endian words, one chunk at a time
extern const uint8_t PNA_SIGNATURE[8];
void put_be32(uint8_t *p, uint32_t v);
uint32_t rd_be32(const uint8_t *p);
struct PnaChunk { size_t off; uint32_t len; const uint8_t *type, *data; };      // off: where the chunk starts; its CRC follows the body
enum { CHUNK_OK = 0, CHUNK_SHORT_HEADER, CHUNK_SHORT_BODY };
int  next_chunk(const uint8_t *buf, size_t len, size_t &pos, PnaChunk &out);
bool chunk_crc_ok(const PnaChunk &ch);
bool b64_decode_nopad(const std::string &s, std::vector<uint8_t> &out);
void frame_inner_entry_empty(std::vector<uint8_t> &o, const char *name);
void frame_solid_head(std::vector<uint8_t> &o, int compression);
void frame_solid_head_enc(std::vector<uint8_t> &o, int compression, int encryption, int cipher_mode, const char *phsf, const uint8_t *prefix, size_t prefix_len);
void frame_solid_tail(std::vector<uint8_t> &o);
void frame_nonfile_record(std::vector<uint8_t> &o, int kind, const char *name, const void *extra, size_t extra_len, const void *facets, size_t facets_len,
                          const void *target, size_t target_len, uint32_t max_chunk);
void frame_archive_head(std::vector<uint8_t> &o, uint32_t archive_number);
void frame_archive_tail(std::vector<uint8_t> &o);
void frame_entry_prefix(std::vector<uint8_t> &o, const char *name, int compression, uint64_t raw_size, uint32_t payload_len);
size_t frame_entry_prefix_bound(const char *name);
size_t frame_entry_prefix_into(uint8_t *out, const char *name, int compression, uint64_t raw_size);
uint32_t frame_fend_crc();
void frame_entry_prefix_enc(std::vector<uint8_t> &o, const char *name, int compression, uint64_t raw_size, int encryption, int cipher_mode,
                            const char *phsf, const uint8_t *prefix, size_t prefix_len);
std::vector<uint8_t> frame_fhed_bytes(const char *name, int compression, int encryption, int cipher_mode);
void sha256_bytes(const void *a, size_t an, const void *b, size_t bn, uint8_t out[32]);
void hkdf_sha256_32(const void *ikm, size_t ikm_len, const void *salt, size_t salt_len, const void *info, size_t info_len, uint8_t okm[32]);
void launch_gcm_tag(const GcmEntry *ents, uint32_t n, uint8_t *buf, hipStream_t st);
void launch_gcm_verify(const GcmEntry *ents, uint32_t n, const uint8_t *buf, const uint8_t *expect, uint32_t *bad, hipStream_t st);
__attribute__((weak)) void launch_gcm_verdict(const GcmEntry *ents, uint32_t n, const uint8_t *buf, const uint8_t *expect, uint32_t *verdict, hipStream_t st);
void launch_aes_cbc_dec(const CipherUnit *units, uint32_t n, const uint8_t *ivs, const AesDecTabs *tabs, uint8_t *buf, const AesKey &dkey, uint32_t *plain_len, hipStream_t st);
size_t frame_entry_prefix_enc_bound(const char *name, const char *phsf);
void launch_aes_ctr(const CipherUnit *units, uint32_t n, const uint8_t *ivs, const AesTabs *tabs, uint8_t *buf, const AesKey &key, const AesKey *keys, hipStream_t st);
void launch_aes_cbc_enc(const CipherUnit *units, uint32_t n, const uint8_t *ivs, const AesTabs *tabs, uint8_t *buf, const AesKey &key, hipStream_t st);
// Camellia-256 in the cipher stage (k_cipher.hip; weak like the xz launchers: the sanitizer build has no stand-ins for them and still links -- Camellia
// then stays PNA_E_UNSUPPORTED whatever option "camellia" says).  Only pna_cipher.cpp calls the six cipher launchers.
__attribute__((weak)) void launch_cam_ctr(const CipherUnit *units, uint32_t n, const uint8_t *ivs, const CamTabs *tabs, uint8_t *buf, const CamKey &key, const CamKey *keys, hipStream_t st);
__attribute__((weak)) void launch_cam_cbc_enc(const CipherUnit *units, uint32_t n, const uint8_t *ivs, const CamTabs *tabs, uint8_t *buf, const CamKey &key, hipStream_t st);
__attribute__((weak)) void launch_cam_cbc_dec(const CipherUnit *units, uint32_t n, const uint8_t *ivs, const CamTabs *tabs, uint8_t *buf, const CamKey &dkey, uint32_t *plain_len, hipStream_t st);
void launch_corpus(int kind, uint64_t first_file, uint64_t n_files, uint64_t file_len, uint64_t stride,
                   const uint8_t *vocab, const uint64_t *cum, const uint32_t *phrases, uint8_t *dst, hipStream_t st);
}
using namespace pna;

struct DevBuf {
    void *p = nullptr; size_t cap = 0;
    int ensure(size_t n) {
        if (n <= cap) return 0;
        if (p) (void)hipFree(p);
        p = nullptr; cap = 0;
        size_t want = n + (n >> 3) + 4096;
        if (hipMalloc(&p, want) != hipSuccess) { p = nullptr; if (hipMalloc(&p, n) != hipSuccess) { p = nullptr; return -1; } want = n; }
        cap = want; return 0;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
};

struct PinBuf {                                  // page-locked host staging: async copies that really are asynchronous
    void *p = nullptr; size_t cap = 0;
    int ensure(size_t n) {
        if (n <= cap) return 0;
        if (p) (void)hipHostFree(p);
        p = nullptr; cap = 0;
        size_t want = n + (n >> 2) + 4096;
        if (hipHostMalloc(&p, want, hipHostMallocDefault) != hipSuccess) { p = nullptr; return -1; }
        cap = want; return 0;
    }
    int ensure_exact(size_t n) {                 // no headroom: a buffer whose size is a documented bound
        if (n <= cap) return 0;
        release();
        if (hipHostMalloc(&p, n, hipHostMallocDefault) != hipSuccess) { p = nullptr; return -1; }
        cap = n; return 0;
    }
    void release() { if (p) (void)hipHostFree(p); p = nullptr; cap = 0; }
};

// Tuning knobs of a context (pna_gpu_set_option; include/pna_gpu.h lists them).  Each starts from the environment variable of the same
// purpose, read ONCE in pna_gpu_init -- no entry point consults the environment afterwards.
struct Tuning {
    long lz_split = 1;               // PNA_LZ_SPLIT: 0 one-kernel LZ stage, 1 split form for long runs (default), 2 split form with the wave-per-region parse kernel
    long lz_split_blocks = 131072;   // PNA_LZ_SPLIT_BLOCKS: blocks per run of the split form (the words workspace holds one run: 3 bytes per input byte -- 16 GiB of input, 48 GiB of words at most; round 5:
                                     // until then 32 768 = 4 GiB per run, and the 10 GiB headline paid three kernel tails per stage -- one run: 74.7 -> 73.5 ms; a workspace that cannot be had is halved, as before)
    long lz_split_min = 0;           // PNA_LZ_SPLIT_MIN: shortest run (segments) that takes the split form (0: every run; shorter ones take the one-kernel form)
    long lz_pbuf_fail = 0;           // PNA_LZ_PBUF_FAIL: testing -- behave as if the words workspace could not be allocated
    long max_chunk_size = 0;         // PNA_MAX_CHUNK_SIZE: FlattenWriter::max_chunk_size of the archive entry points without such a parameter (0 = the reference's default, u32::MAX)
    long sub_mib = 256;              // PNA_SUB_MIB: largest sub-batch (input bytes) of the bounded host pipeline (1 .. 16 384; the small end is for tests)
    long stage_threads = 0;          // PNA_STAGE_THREADS: host threads that stage entries into page-locked memory (0: min(8, cores / 2))
    long extract_win_mib = 1024;     // PNA_EXTRACT_WIN_MIB: archive bytes per window of the extract driver
    long diff_slot_mib = 256;        // PNA_DIFF_SLOT_MIB: pna_gpu_diff_archive_host carries the files' bytes to the device through two page-locked slots of this many MiB (and two device slots)
    long solid_win_mib = 256;        // PNA_SOLID_WIN_MIB: pna_gpu_create_solid_archive_host takes the serialised inner entries through in windows of this many MiB (page-locked memory: ~4 windows)
    long batch_piece_mib = 256;      // PNA_BATCH_PIECE_MIB: pna_gpu_compress_batch takes a large batch through in pieces of this size (0: one piece)
    long inflate_serial = 0;         // PNA_INFLATE_SERIAL: deflate decoding on the wave-per-stream walk only
    long zdec_serial = 0;            // PNA_ZDEC_SERIAL: zstd decoding with one workgroup per frame only
    long zdec_dbg = 0;               // PNA_ZDEC_DBG: the one-workgroup kernel's diagnostics (1 skip execution, 2 skip sequences, 4 skip Huffman streams, 8 small re-base distances)
    long blk_log = 0;                // PNA_BLK_LOG: block size of every batch = 1 << blk_log (13..17); 0 = by batch size (latency mode)
    long unit_log = 0;               // PNA_LZ_UNIT_LOG: LZ units of 1 << unit_log bytes (>= the block size, <= 20); 0 = by batch size
    long latency_max_mib = 128;      // PNA_LATENCY_MAX_MIB: batches of at most this many MiB of input run in latency mode (0: never)
    long tail_units = 1;             // PNA_TAIL_UNITS: the segments behind a run's last full round of the CUs go through the match kernel in units of one block
    long lazy2 = 2;                  // PNA_LAZY2: how far the lazy level sets look ahead beyond the next position: 2 = two more positions (default), 1 = one more, 0 = none (the high sets: one)
    long single_frame = 0;           // PNA_SINGLE_FRAME: 1: a zstd entry is ONE frame whatever its size (header once, last-block bit once; SURVEY 8 a14's fallback for a reader that would
                                     // not take concatenated frames -- zstd's own Decoder, which the reference uses, does); 0 (default): one frame per 1 MiB segment
    long stream_gather_wgs = 48;     // PNA_STREAM_GATHER_WGS: workgroups of the kernel that copies a batch's page-locked slabs to the device (0: one hipMemcpyAsync per slab, ~30 us each)
    long stream_overlap_mib = 24;    // PNA_STREAM_OVERLAP_MIB: while a batch runs on the device the next one is taken (and copied in beside it) only once the queue holds this much
    long stream_batch_mib = 256;     // PNA_STREAM_BATCH_MIB: input bytes one batch of the streaming facade takes at most (the queue's rest is the next batch, which is copied in meanwhile)
    long zexec_par_min_mib = 8;      // PNA_ZEXEC_PAR_MIN_MIB: zstd frames whose content takes this many MiB and more are executed in parallel by pointer jumping (0: never)
    long zdec_fallback_max_mib = 0;  // PNA_ZDEC_FALLBACK_MAX_MIB: zstd frames of more content than this that the parallel paths cannot take are REFUSED (PNA_E_UNSUPPORTED) instead of decoded by one workgroup at ~11 MiB/s (0: no limit) -- a host may prefer its CPU decoder
    long zexec_win_mib = 1024;       // PNA_ZEXEC_WIN_MIB: output bytes of one window of the parallel executor (its words count 31 bits from the window's start: at most 1 024; tests take a few MiB)
    long small_geometry = 1;         // PNA_SMALL_GEOMETRY: 1 (default): segments of at most 4 096 bytes run the small geometry of the match finder (pna_dev.h SMALL_SEG: one wave per segment, sub-tiles of 256 positions); 0: the large one like every segment (they then find no match: one tile)
    long mtile = 0;                  // PNA_MTILE: 0 (default): the match kernel k_lzm looks up all 4 096 positions of a tile before it inserts any; 256 / 512 / 1024 / 2048: look-ups and inserts alternate per sub-tile of that many positions, so that a position sees the tile's earlier sub-tiles (oracle: mtile).  Segments above 16 KiB of every set with the table in LDS -- zstd 1 .. 9, deflate --, always in the split form and in whole segments (no LZ units); zstd 10 .. 22 ignore it
    long tab3 = 1;                   // PNA_TAB3: 1 (default): the zstd sets on the 32 / 16 KiB geometries keep their table PACKED (three 21-bit entries per 64-bit LDS word: 49 062 / 55 206 slots, lz_common.h); 0: 32-bit entries (32 704 / 36 800)
    long strong2 = 1;                // PNA_STRONG2: 1 (default): zstd levels 4 .. 22 on their standard geometries adopt over eight positions as well and count up to 15 back bytes (levels 6 - 9: 2.864 -> 2.880); 0: the default set's three rounds
    long seq_hist = 1;               // PNA_SEQ_HIST: 1 (default): large zstd batches behind the split LZ stage -- the parse kernel counts every block's sequence codes, k_stats walks the literals only (2.6 -> 1.1 ms per 10 000 segments, + 0.5 in the parse kernel); 0: k_stats reads the sequences once more
    long far1 = 1;                   // PNA_FAR1: 1 (default): the zstd light / default sets (packed table, 32 KiB window) verify at most 63 far candidates per wave of 256 positions -- one compacted round of k_lzm -- and drop the rest (FLAG_FAR1: - 0.16 % of ratio, - 6 % of the match kernel); 0: every far candidate, in as many rounds as it takes
    long win32k = 1;                 // PNA_WIN32K: 1 (default): the zstd default set on the 32 KiB-window geometry of the match finder (32 704 table slots), the high set on the 16 KiB one (36 800); 0: both on 64 KiB / 24 512; 2: both on 16 KiB
    long lit_beside_seq = 1;         // PNA_LIT_BESIDE_SEQ: large zstd batches: the literal coder on a second stream next to the sequence coder
    long strong_gtab = 1;            // PNA_STRONG_GTAB: zstd levels 10 .. 22 with the match kernel's hash tables in global memory (2^19 slots per segment); 0: the LDS table
    long dev_layout = 1;             // PNA_DEV_LAYOUT: archive layout of plain one-chunk entries on the device (k_layout); 0: on the host, after a wait for the sizes
    long trace = 0;                  // PNA_TRACE: phase times of the host pipelines on stderr
    long d2h_wgs = 6;                // PNA_D2H_WGS: workgroups of the kernel that carries a sub-batch's archive bytes to the host (0: the copy engine / runtime's choice)
    long xz_encode = 0;              // PNA_XZ_ENCODE: 1: pna_gpu_compress_batch[_device] and the non-solid archive entry points take PNA_ALGO_XZ (k_xzenc.hip: multi-block streams with per-chunk state resets -- their bytes differ from the reference's encoder and their ratio is lower, so a host chooses them knowingly); 0 (default): PNA_E_UNSUPPORTED, as before
    long camellia = 0;               // PNA_CAMELLIA: 1: Encryption::CAMELLIA (Camellia-256 in CTR, CBC and GCM STREAM; k_cipher.hip) is written by the entry points that take a cipher and read by extract / verify / diff / extract-select; 0 (default): PNA_E_UNSUPPORTED / PNA_VERIFY_UNSUPPORTED, as before
    long kdf_device = 0;             // PNA_KDF_DEVICE: 0 (default): the read-side drivers derive every key on the host, one PHSF string after the other; N >= 1: a window's not yet derived PHSF strings go through pna_gpu_kdf_batch (k_kdf.hip) when there are at least N of them
    long kdf_mem_mib = 0;            // PNA_KDF_MEM_MIB: the cap of pna_gpu_kdf_batch's Argon2 block memory; 0 (default): a quarter of the device's free memory at the first batch, at most 32 GiB
    long store_unfused = -1;         // PNA_STORE_UNFUSED: stored payloads without a cipher -- 0: the fused k_store + k_store_fold (one read of the payload); 1: k_store's copy-only form and k_frame (two reads; a chunk is CRC'd by ONE workgroup); -1 (default): per sub-batch by its longest data chunk -- fused above 1 MiB and up to 4 KiB, unfused between, as measured in profiles/store_rate.txt; the bytes are the same
    long hist_by_block = -1;         // PNA_HIST_BY_BLOCK: zstd entropy stage in its per-block form (1: k_hist, k_seqa, k_seqb) or its per-segment form (0: k_stats, k_seq); -1: by batch size
};
struct TuningName { const char *name, *env; long Tuning::*field; long lo, hi; };

// The LZ stage's parameter set of one call: what its level and the options choose (lz_level_set), the source of every launch's flag word (lz_launch_flags)
struct LzSet {
    uint32_t bits = 0;                 // of call_flags, what the launch word takes over: the level set and the diagnostics the LZ kernels know (INIT_TO_LAUNCH)
    bool lazy2 = false, lazy3 = false; // lazy deferral over two / three positions (FLAG_LAZY2, FLAG_LAZY3)
    bool gtab = false;                 // the max set: the match kernel's table in global memory -- always the split form, words of four bytes
    bool w32 = false, w16 = false;     // the match finder's LDS geometry: the 32 KiB window, of these the 16 KiB one (FLAG_W32 / FLAG_W16)
    bool tab3 = false, far1 = false;   // ... its table packed (FLAG_TAB3), far candidates in one compacted round (FLAG_FAR1)
    bool strong2 = false;              // the high / max sets' fourth adoption round and 15 back bytes (FLAG_STRONG2)
    uint32_t max_off = 0, max_len = 0; // the longest look-back and match of the codec and the set
};
struct pna_gpu_stream;
struct pna_gpu_ctx {
    Tuning tun;
    // the plan of a sub-batch -- segment descriptors, LZ units (latency mode: pieces of segments, one workgroup each), block -> segment, entry -> first
    // segment -- is staged in ONE page-locked blob and travels in one copy; the per-segment histograms of k_hist lie behind the BlkInfo array (one memset)
    DevBuf plan; PinBuf h_plan;
    DevBuf d_tail; PinBuf h_tail; size_t tail_used = 0;     // unit descriptors of the segments behind a run's last full round of workgroups (lz_stage)
    SegDesc *d_segs = nullptr, *d_units = nullptr; uint32_t *d_blk_seg = nullptr, *d_entry_seg = nullptr, *d_hist = nullptr;
    uint32_t last_blk_log = PNA_BLK_LOG, last_units = 0;
    int device = 0;
    uint32_t flags = 0;
    uint32_t call_flags = 0;                        // flags of the current call: the level picks the parse (level_flags)
    LzSet lz;                                       // ... and the LZ stage's parameter set (lz_level_set, pna_lz.cpp)
    uint32_t n_cus = 256;                           // compute units of the device (hipDeviceProp_t::multiProcessorCount): a full round of one-workgroup-per-CU kernels
    bool call_xz = false;                           // the current call writes xz: LZ blocks of at most 64 KiB (one LZMA2 chunk each), matches of at most 273 bytes
    bool call_stored = false;                       // deflate level 0: stored blocks only (Compression::none())
    bool lzp_hist_all = false;                      // the current sub-batch: the parse kernel has added EVERY segment's sequence codes to the segments' counters (lz_run)
    std::vector<hipEvent_t> lzm_ev; size_t lzm_used = 0;   // event pairs around the match kernel launches of the current sub-batch (timed calls)
    std::vector<uint8_t> lzm_nl;                            // launches inside each pair (2 where a run's last segments go in units)
    hipStream_t stream = nullptr;
    hipEvent_t ev[8] = {};
    DevBuf blk, tabs, seqs, lits, litc, seqc, seqw, seg_size, seg_off, stage_in, stage_out, ctab, pbuf;
    DevBuf z_list;                                  // foreign multi-frame payloads: the frame list (k_zlist)
    DevBuf z_big, z_one;                            // large zstd frames: their numbers, their blocks (k_zparse_a -> k_zparse<true>)
    DevBuf z_spec;                                  // large foreign zlib streams: chunk starts + chunk descriptors (k_ispec, k_inflate's chunk mode)
    DevBuf z_words, z_rep, z_zxf;                   // the parallel executor of large zstd frames (k_zexec_par.hip): a word per output byte, histories per block
    uint32_t zexec_par_rounds = 0;                  // pointer-jumping rounds of the latest large frame (diagnostics)
    std::vector<uint64_t> pl_off, pl_len, pl_cap, pl_eoff;   // the host pipeline's per-entry plan (staging offsets, lengths, capacity terms), kept between calls
    uint32_t inflate_spec_streams = 0;              // streams of the latest inflate call that went through the speculative chunk decoder (diagnostics)
    DevBuf c_vocab, c_cum, c_phr;
    DevBuf gtab;                                    // hash tables of the strong level set's match kernel (global memory)
    DevBuf fr_desc, fr_blob, fr_segdst, fr_entoff, crc_tabs;
    PinBuf h_entoff;
    DevBuf x_arc, x_pk, x_raw[2], x_desc, x_place, x_flag, x_tags, x_plen, aes_dtabs;
    DevBuf v_crc, v_seg, v_ent, v_out;   // pna verify: chunk and segment verdicts, the records' VerdictEnt, their status words
    // pna diff: the files' bytes travel through two page-locked slots (df_pin) into two device slots (df_dev) on a stream of their own; df_ev_cp[s]: slot s is on the
    // device, df_ev_k[s]: the k_diff launches that read it are done; the piece lists, first[] of the window's records; event pairs around the k_diff launches
    PinBuf df_pin[2]; DevBuf df_dev[2], df_pieces, df_first;
    hipStream_t df_cp = nullptr; hipEvent_t df_ev_cp[2] = {}, df_ev_k[2] = {}; std::vector<hipEvent_t> df_tev; size_t df_tused = 0;
    uint64_t df_streams = 0, df_bytes = 0; double df_ms = 0;   // the latest diff call: streams handed to the decoders, bytes compared by k_diff, its HIP-event time
    // pna_gpu_extract_select_host: k_pick's piece list, event pairs around its launches, and the latest call's counters -- bytes of H2D archive copies, streams
    // taken through the decode stage, key derivations, bytes k_pick moved, its HIP-event time
    DevBuf xs_pieces; std::vector<hipEvent_t> xs_tev; size_t xs_tused = 0;
    uint64_t xs_uploaded = 0, xs_streams = 0, xs_kdf = 0, xs_picked = 0; double xs_ms = 0;
    // pna_gpu_kdf_batch (pna_kdf.cpp): Argon2's block memory (one allocation, at most kdf_cap bytes), the jobs, seed blocks and results of a round; the latest batch's counts
    DevBuf kdf_mem, kdf_jobs, kdf_seeds, kdf_fin; size_t kdf_cap = 0; hipEvent_t kdf_ev[2] = {};
    uint64_t kdf_dev_jobs = 0, kdf_host_jobs = 0, kdf_rounds = 0; double kdf_ms = 0;
    hipStream_t x_cp = nullptr; hipEvent_t x_ev[2] = {}, x_done = nullptr;   // extract driver: D2H of window k on x_cp next to window k+1's work
    bool aes_dec_ready = false;        // read side (pna_gpu_extract_archive_host): archive image, packed payloads, decoded entries
    DevBuf xz_in, xz_scan, xz_blocks, xz_pieces, xz_acc;       // xz decode: stream descriptors, scan results, block descriptors, check pieces, accumulators + stream statuses
    DevBuf z_vp, z_pb, z_mode;                                 // lane-per-piece inflate: piece list, piece boundaries, per-stream mode
    DevBuf ci_spread, ci_spread_desc;                          // GCM entries of several segments: their compact payloads, the pieces to move
    DevBuf aes_tabs, ci_units, ci_ivs, ci_keys, ci_gcm;        // cipher stage: round tables, unit descriptors, IVs; GCM: per-segment round keys (SegKeys), segment descriptors
    bool aes_ready = false;
    DevBuf cam_tabs, ci_ckeys; bool cam_ready = false;         // ... for Camellia (option camellia): its four tables, GCM's per-segment schedules (SegKeys)
    hipEvent_t ev_ci[2] = {};
    DevBuf solid_plain, solid_desc, solid_blob, solid_place;   // serialised inner entries of a solid archive
    // Compression::No (store_subbatch): the pieces, the framing bytes' places, the chunks and the pieces' CRC registers; the event pair around k_store; the
    // latest call's counters (pna_gpu_debug_store_stats); option store_unfused: plain payloads take the copy-only form + k_frame
    DevBuf st_pieces, st_lits, st_chunks, st_states; hipEvent_t st_ev[2] = {};
    uint64_t st_fused = 0, st_copy_only = 0, st_folded = 0; double st_ms = 0;
    DevBuf solid_adler;                                        // deflate solid from host memory: the stream's Adler-32 carried from window to window
    DevBuf solid_carry;                                        // GCM solid from host memory: the tail of a window's output not yet cut into a segment
    DevBuf z_ents, z_frames, z_lit;                            // decoder descriptors, literal scratch
    DevBuf z_fx, z_blocks, z_tabs, z_seqs, z_hlist, z_slist, z_work, z_fb, z_cbase, z_apart;   // lane-parallel decoder workspace
    PinBuf h_desc, h_blob, h_segdst, h_segoff;
    // pipelined host path (pna_gpu_create_archive_host): two slots of staging
    PinBuf hp_in[4], hp_out[2];
    // page-locked buffers handed to the host (pna_gpu_host_alloc): entries that live in one go to the device straight from there (no staging copy)
    std::mutex lent_mu; std::vector<std::pair<const uint8_t *, size_t>> lent;
    DevBuf dp_in[4], dp_out[2];
    hipStream_t cp_in = nullptr, cp_out = nullptr;
    uint64_t call_total = 0;                          // input bytes of the whole call that run_subbatch's sub-batch belongs to (0: the sub-batch is the call): decides the block size
    hipStream_t aux = nullptr;                        // zstd's literal coder next to the sequence coder (option lit_beside_seq)
    hipEvent_t ev_lz[2] = {}, ev_en[4] = {}, ev_join = nullptr, ev_fork = nullptr;   // around the LZ stage, the entropy stage's parts; aux's fork and join
    hipEvent_t ev_in[4] = {}, ev_out[2] = {};
    bool crc_ready = false;
    bool corpus_ready = false;
    std::string err;
    pna_gpu_timing timing = {};
    pna_gpu_decode_forms forms = {};                // which forms of the decoders the latest decode call ran (pna_gpu_last_decode_forms)
    uint32_t last_nblk = 0;
    uint32_t plan_log = PNA_BLK_LOG;                // block size the current call's sub-batches are planned with (plan_call)
    size_t max_blocks = (size_t)1 << 17;            // blocks per sub-batch: what ~96 GiB of per-block workspace hold at that block size (16 GiB of input at 128 KiB)
    // group commit of the streaming facade (pna_gpu_stream_finish from many host threads -> one device batch)
    std::mutex comb_mu, run_mu;            // comb_mu: queue + leader flag; run_mu: the device batch itself and ctx->err
    std::condition_variable comb_cv, gate_cv;   // gate_cv: the ONE leader waiting for its slot / the device / a larger queue (every push signals it: not the hundreds of writers on comb_cv)
    std::vector<pna_gpu_stream *> comb_queue;
    bool comb_leader = false;
    uint64_t comb_batches = 0, comb_entries = 0, comb_max = 0, comb_seq = 0;
    uint32_t comb_linger_us = 0xFFFFFFFFu; // PNA_STREAM_LINGER_US: the leader waits this long for more finishes before it submits (unset: adaptive)
    size_t comb_last = 0;                  // entries of the previous batch
    size_t comb_peak = 0;                  // the cohort the linger waits for: the largest recent batch (max(batch, peak - 1): a straggler's batch of one does not shrink it)
    // page-locked memory of the streaming facade: write() copies straight into 1 MiB slabs of a pool (no staging copy before the H2D
    // copy), the compressed streams come back into one of two page-locked output slots and the owners drain them from there
    std::mutex pool_mu;
    std::vector<void *> pool_arenas; std::vector<uint8_t *> pool_free; size_t pool_bytes = 0, pool_cap = 4096ull << 20;
    // Round 4: the batches of the facade form a PIPELINE of three stages over three slots -- (1) the H2D copies of batch k + 1 from the writers' slabs, (2) the
    // device batch k, (3) the D2H copy of batch k - 1's streams -- each on a stream of its own; a leader holds `comb_leader` only while it takes its batch
    // and copies it in, `run_mu` only for the device batch.  A batch takes at most stream_batch_mib of input (what fills the chip), the rest of the queue
    // is the next leader's.
    static constexpr int S_SLOTS = 3;
    PinBuf s_out[S_SLOTS];
    DevBuf st_in[S_SLOTS], st_out[S_SLOTS];
    PinBuf s_segs[S_SLOTS];                 // the copy-in kernel's segment list of the slot's batch
    hipStream_t s_h2d = nullptr, s_d2h = nullptr;
    hipEvent_t s_ev[S_SLOTS] = {nullptr, nullptr, nullptr};
    uint64_t slot_pending[S_SLOTS] = {0, 0, 0};     // streams of the slot's last batch that have not been drained yet (under comb_mu)
    bool device_busy = false;              // a batch of the facade holds the device (under comb_mu).  While it does, a new leader keeps collecting until the queue holds
                                           // stream_overlap_mib -- enough to be worth copying in beside the running batch --; few writers therefore still form ONE batch per
                                           // device turn (the fixed ~0.7 ms of a batch is shared by all of them), many writers fill the pipeline
    uint32_t staged_waiting = 0;           // batches copied in and waiting for the device (under comb_mu): a new leader takes its batch only when there is none --
                                           // while the device is busy the queue keeps growing, so few writers still share batches (4 writers: batches of 2 - 3, not 1)
    std::mutex err_mu;                     // ctx->err from the pipeline's copy stages (the device batch sets it under run_mu as every entry point does)
};

inline int fail(pna_gpu_ctx *c, int code, const char *what, hipError_t e = hipSuccess) {
    if (c) { c->err = what; if (e != hipSuccess) { c->err += ": "; c->err += hipGetErrorString(e); } }
    return code;
}
#define HIPCHK(c, call) do { hipError_t e__ = (call); if (e__ != hipSuccess) return fail((c), PNA_E_HIP, #call, e__); } while (0)

// ---- what the translation units of the host code share (defined in pna_host.cpp unless noted)
constexpr uint64_t CTR_UNIT = 256u << 10;                    // bytes of one CTR work unit (one workgroup)
struct PlaceDescH { uint64_t src_off, dst_off; uint32_t len, pad; };   // = PlaceDesc of k_frame.hip (k_place / k_gather)
// The entries of a call that are not files (pna_gpu_entry_kinds: directories, symbolic links, hard links): their finished records (frame_nonfile_record),
// built once per call.  Entry e's record is blob[off[e] .. off[e + 1]); a file's is empty, so `len(e) != 0` is "entry e is not a file".
struct EntryRecords { std::vector<uint8_t> blob; std::vector<uint64_t> off; size_t count = 0;
                      uint64_t len(size_t e) const { return off[e + 1] - off[e]; } const uint8_t *at(size_t e) const { return blob.data() + off[e]; } };
struct FrameJob { const char *const *names; int solid; const pna_gpu_cipher *cipher = nullptr; const uint8_t *ivs = nullptr; const pna_gpu_entry_meta *meta = nullptr;
                  uint32_t max_chunk = 0; bool want_offsets = true;      // FDAT chunks of at most this many bytes (FlattenWriter::max_chunk_size; 0 = the reference's default u32::MAX)
                  // a solid stream compressed in windows (pna_gpu_create_solid_archive_host): the sub-batch is one window of a stream of stream_len bytes and
                  // is planned as the whole stream; deflate: DRUN_* flags of the window's place in the stream, the stream's Adler-32 carry in device memory
                  uint64_t stream_len = 0; uint32_t run = 0; uint32_t *adler_carry = nullptr;
                  // ... with a cipher: where the window stands in the cipher stream, updated by layout_solid (SolidCipherRun)
                  struct SolidCipherRun *crun = nullptr;
                  // ... stored (PNA_ALGO_STORE): where the window stands in the stream and the CRC register of the SDAT chunk that is open across the window edge,
                  // updated by store_solid_window (SolidStoreRun); max_chunk then also cuts the stream into SDAT chunks
                  struct SolidStoreRun *srun = nullptr;
                  // the tree entry points: the call's non-file records (NULL: every entry is a file).  Such an entry has no segments, no cipher unit, no IV drawn
                  const EntryRecords *recs = nullptr; };
// The cipher state of a solid stream compressed in windows.  CTR: `pos`, the stream offset of the window's first compressed byte (the keystream
// continues).  GCM STREAM: segments are cut from the whole compressed stream -- `seg`, the counter of the next segment; `carry` (carry_len bytes,
// 1 .. G once the stream has begun, in device memory) the tail of the output before that is not yet known to be a non-final segment, placed in
// front of the window's output; `final_win`: nothing follows the window, its last segment carries the final flag.  layout_solid advances
// pos, seg and carry_len past the window.
// The state of a STORED solid stream that travels in windows: `pos`, the stream position of the window's first byte; `state` / `started`: the raw CRC register of
// the SDAT chunk that began in an earlier window and has not ended yet (chained with CRC(A || B) = x^(8|B|) CRC(A) + CRC(B), as the inner chunks are).
struct SolidStoreRun { uint64_t pos = 0; uint32_t state = 0; bool started = false; };
struct SolidCipherRun { uint64_t pos = 0, seg = 0, carry_len = 0; uint8_t *carry = nullptr; bool final_win = false; };
// A block cipher's key schedule as a value (pna_cipher.cpp): which cipher (a PNA_ENC_* id) and its schedule.  cipher_ctr / cipher_cbc_enc / cipher_cbc_dec
// turn the id into a kernel, block() into the host's block function; nobody else asks which cipher it is.
struct BlockKey {
    int enc = PNA_ENC_AES;
    union { AesKey aes; CamKey cam = {}; };                        // (zeroed through its larger member)
    void expand(int encryption, const uint8_t key32[32]);          // the encryption schedule of a 256-bit key
    BlockKey dec() const;                                          // ... its counterpart for decryption (CBC)
    void block(const uint8_t in[16], uint8_t out[16]) const;       // one block on the host
};
// GCM STREAM: the schedule of every segment's stream by segment index, as the CTR kernels read them (keys[unit.iv_idx]) -- one array per cipher, a
// segment's slot in the other one unused.  A window of the read side may mix AES and Camellia streams: sort_units puts the AES segments' units first,
// and cipher_ctr runs each cipher's kernel over its part.  (A list that is not sorted holds one cipher only.)
struct SegKeys {
    std::vector<AesKey> aes; std::vector<CamKey> cam; std::vector<uint8_t> is_cam; size_t aes_units = 0;
    void push(uint32_t segment, const BlockKey &k);
    void sort_units(std::vector<CipherUnit> &units);
    int upload(pna_gpu_ctx *c, hipStream_t st) const;              // to c->ci_keys / c->ci_ckeys
};
struct GcmMaterial { uint8_t header[75]; BlockKey key; uint32_t h[4]; };     // a stream's header, the schedule of its stream key and the hash subkey
struct GcmCallKeys { uint8_t kc[32], phsf_hash[32]; };
// GCM STREAM segment size of a cipher job (0: the reference's DEFAULT_SEGMENT_SIZE, 1 MiB)
inline uint32_t gcm_seg_size(const pna_gpu_cipher *ci) { return ci->gcm_segment_size ? ci->gcm_segment_size : (1u << 20); }

void set_call_level(pna_gpu_ctx *c, int algo, int level);
// The plan of a sub-batch (plan_subbatch, pna_host.cpp): its geometry, its forms, and the host's copy of the tables it uploaded
struct SubPlan {
    uint32_t blk_log = PNA_BLK_LOG, unit_log = 20, nseg = 0, nblk = 0, nunits = 0;
    uint64_t max_len = 0;                    // the longest entry (a window of a solid stream: the whole stream)
    bool latency = false, unit_mode = false, single_block = false, hist_on = false, seq_hist = false, any_empty = false;
    uint32_t small_fl = 0;                   // launch flags of the short segments' geometry (k_lzms)
    bool wave_blk = false;                   // many small entries: deflate's stage 1 runs a wave per segment, the write kernels a wave per block
    uint32_t frame_max_payload = 0;          // an upper bound of every payload when the entries are small and plain (k_frame's wave-per-entry form; 0: none)
    const SegDesc *segs = nullptr; const uint32_t *entry_first_seg = nullptr;
};
// pna_lz.cpp -- the host side of the LZ stage: the level's parameter set (algo: zstd or deflate; xz: zstd's with LZMA's match cap), and the stage over one sub-batch
LzSet lz_level_set(const pna_gpu_ctx *c, int algo, int level, bool xz);
int lz_run(pna_gpu_ctx *c, int algo, const uint8_t *d_src, const SubPlan &p, hipStream_t st, bool timed);
// what the compress entry points take: zstd, deflate and -- with option xz_encode, on the batch and the non-solid archive entry points -- xz; `archive`: the
// non-solid archive entry points, which write stored entries too (run_subbatch's codec-free branch)
inline bool encode_algo_ok(const pna_gpu_ctx *c, int algo, bool archive = false) {
    if (algo == PNA_ALGO_STORE) return archive && launch_store && launch_store_fold;
    return algo == PNA_ALGO_ZSTD || algo == PNA_ALGO_DEFLATE || (algo == PNA_ALGO_XZ && c && c->tun.xz_encode != 0 && launch_xzenc_stage && launch_xzenc_write);
}
inline size_t plan_blocks(const pna_gpu_ctx *c, uint64_t len) {
    return (size_t)((len + ((uint64_t)1 << c->plan_log) - 1) >> c->plan_log);
}
// Block size of a batch whose entries are all small: the per-block arrays have the block size as their stride, so a batch of 4 KiB entries on 128 KiB
// blocks would spend 32 times the memory (and a sub-batch per 131 072 entries) that 8 KiB blocks need.  Entries of up to 64 KiB: the power of two that
// holds the largest (>= 8 KiB); anything larger: 128 KiB.  (Latency mode, for small batches of large entries, chooses on top of this in plan_geometry.)
// The input bytes of the whole call for the duration of a scope (pna_gpu_ctx::call_total: run_subbatch picks the block size by the call, not by its sub-batches)
// A scope opened while another is open on the context (an entry point that cuts its call into parts or pieces and runs each through another entry point: the
// multi-context create, the host form of compress_batch) leaves the outer total in place -- every part then picks the block size of the WHOLE call, so the
// bytes do not depend on how the call was cut.
struct CallTotalScope {
    pna_gpu_ctx *c; bool own;
    template <class L> CallTotalScope(pna_gpu_ctx *ctx, const L *len, size_t n) : c(ctx), own(ctx->call_total == 0) {
        if (own) { uint64_t t = 0; for (size_t i = 0; i < n; i++) t += len[i]; c->call_total = t; } }
    CallTotalScope(pna_gpu_ctx *ctx, uint64_t total) : c(ctx), own(ctx->call_total == 0) { if (own) c->call_total = total; }
    ~CallTotalScope() { if (own) c->call_total = 0; }
    CallTotalScope(const CallTotalScope &) = delete; CallTotalScope &operator=(const CallTotalScope &) = delete;
};
inline uint32_t blk_log_for_longest(const pna_gpu_ctx *c, uint64_t mx) {
    const uint32_t cap = c->call_xz ? std::min<uint32_t>(16u, PNA_BLK_LOG) : (uint32_t)PNA_BLK_LOG;     // (xz: an LZ block is one LZMA2 chunk, 64 KiB at most)
    if (c->tun.blk_log) return std::min<uint32_t>((uint32_t)c->tun.blk_log, cap);
    if (mx > 65536) return cap;
    uint32_t lg = BLK_LOG_MIN;
    while (((uint64_t)1 << lg) < mx) lg++;
    return lg;
}
// The per-entry host loops of a sub-batch of 10^5 .. 10^6 small entries (plan, bounds, record prefixes) run on several threads over CONTIGUOUS index
// ranges: fn(t, a, b) for thread t and its range [a, b) of [0, n); the caller's thread takes the first range.
inline unsigned host_loop_threads(size_t n) {
    const unsigned hw = std::max(1u, std::thread::hardware_concurrency());
    return (unsigned)std::min<size_t>(std::min<unsigned>(16u, hw), std::max<size_t>(1, n / 16384));
}
// The helper threads are a process-wide POOL (round 5): a sub-batch of 10^6 entries runs half a dozen of these loops, and starting + joining fifteen threads for each
// was ~0.5 ms a time -- more than the loops themselves.  One job at a time (a second caller -- another context's thread -- starts threads of its own, as before).
struct HostPool {
    std::mutex mu, busy; std::condition_variable cv, done_cv;
    std::vector<std::thread> th;
    std::function<void(unsigned)> job; unsigned want = 0, gen = 0, left = 0; bool stop = false;
    void worker(unsigned t) {
        unsigned seen = 0;
        for (;;) {
            std::function<void(unsigned)> j;
            {
                std::unique_lock<std::mutex> lk(mu);
                cv.wait(lk, [&] { return stop || (gen != seen && t < want); });
                if (stop) return;
                seen = gen; j = job;
            }
            j(t);
            { std::lock_guard<std::mutex> lk(mu); if (--left == 0) done_cv.notify_all(); }
        }
    }
    // runs fn(1 .. nt - 1) on the pool's threads and fn(0) on the caller's; false: the pool is taken (the caller falls back)
    bool run(unsigned nt, const std::function<void(unsigned)> &fn) {
        if (!busy.try_lock()) return false;
        {
            std::lock_guard<std::mutex> lk(mu);
            while (th.size() + 1 < nt) { const unsigned t = (unsigned)th.size() + 1; th.emplace_back([this, t]() { worker(t); }); }
            job = fn; want = nt; left = nt - 1; gen++;
        }
        cv.notify_all();
        fn(0);
        { std::unique_lock<std::mutex> lk(mu); done_cv.wait(lk, [&] { return left == 0; }); want = 0; }
        busy.unlock();
        return true;
    }
    ~HostPool() { { std::lock_guard<std::mutex> lk(mu); stop = true; } cv.notify_all(); for (auto &x : th) x.join(); }
};
inline HostPool &host_pool() { static HostPool p; return p; }
template <class F>
inline void par_ranges(size_t n, unsigned nt, F &&fn) {
    if (nt <= 1) { fn(0u, (size_t)0, n); return; }
    auto part = [&fn, n, nt](unsigned t) { if (t == 0) fn(0u, (size_t)0, n / nt); else fn(t, n * t / nt, n * (t + 1) / nt); };
    if (host_pool().run(nt, part)) return;
    std::vector<std::thread> th;
    for (unsigned t = 1; t < nt; t++) th.emplace_back([&part, t]() { part(t); });
    part(0);
    for (auto &x : th) x.join();
}
// per call: the block size the sub-batches are cut with and how many blocks fit the workspace budget
inline void plan_call_longest(pna_gpu_ctx *c, uint64_t longest) {           // plan_call for a caller that knows the longest entry already
    c->plan_log = blk_log_for_longest(c, longest);
    const uint64_t per_block = (uint64_t)seq_cap_of(c->plan_log) * 16 + ((uint64_t)3 << c->plan_log) + 64;
    c->max_blocks = (size_t)std::max<uint64_t>(1024, (96ull << 30) / per_block);
}
template <class L>
inline void plan_call(pna_gpu_ctx *c, const L *src_len, size_t n) {
    uint64_t mx = 0;
    if (!c->tun.blk_log) for (size_t e = 0; e < n; e++) mx = std::max<uint64_t>(mx, src_len[e]);     // (a forced block size needs no longest entry)
    plan_call_longest(c, mx);
}


int  ensure_crc(pna_gpu_ctx *c);
uint32_t crc_gf2_mulmod(uint32_t a, uint32_t b);       // a * b mod P of the CRC-32 (reflected bit order), x^e mod P: what chains the raw registers of a chunk's pieces
uint32_t crc_gf2_xpow(uint64_t e);
// The cipher stage's dispatch (pna_cipher.cpp), in place over `buf`: units and ivs are device arrays, `key` a by-value kernel argument; each readies its
// cipher's tables on first use.  cipher_ctr: stream_keys != null -- GCM STREAM, every unit under the schedule of its segment (uploaded before).
// cipher_mark: records event `i` of the pair around the stage (ms_cipher) -- event 0 by the three functions themselves, once their tables are on the
// device, event 1 by the caller.
int  cipher_ctr(pna_gpu_ctx *c, const CipherUnit *units, uint32_t n, const uint8_t *ivs, uint8_t *buf, const BlockKey &key, const SegKeys *stream_keys, hipStream_t st);
int  cipher_cbc_enc(pna_gpu_ctx *c, const CipherUnit *units, uint32_t n, const uint8_t *ivs, uint8_t *buf, const BlockKey &key, hipStream_t st);
int  cipher_cbc_dec(pna_gpu_ctx *c, const CipherUnit *units, uint32_t n, const uint8_t *ivs, uint8_t *buf, const BlockKey &dkey, uint32_t *plain_len, hipStream_t st);
int  cipher_mark(pna_gpu_ctx *c, int i, hipStream_t st);
// Encryption::CAMELLIA is taken: option camellia is on and the library holds the Camellia launchers
bool camellia_on(const pna_gpu_ctx *c);
int  check_cipher(pna_gpu_ctx *c, const pna_gpu_cipher *ci);
int  resolve_ivs(pna_gpu_ctx *c, const pna_gpu_cipher *cipher, size_t n, std::vector<uint8_t> &own, const uint8_t **ivs);
GcmCallKeys gcm_call_keys(const uint8_t key[32], const char *phsf, size_t phsf_len);
void gcm_stream_key(const uint8_t master[32], const uint8_t header[43], const char htype[4], const std::vector<uint8_t> &hbody, const uint8_t phsf_hash[32], int encryption, GcmMaterial &m);
void gcm_segment(const GcmMaterial &m, uint32_t counter, bool fin, GcmEntry &ge, uint8_t iv[16]);
void gcm_entry_material(const pna_gpu_cipher *ci, const GcmCallKeys &keys, const uint8_t salt_prefix[39], uint32_t seg_size, const char *name, int compression,
                        GcmMaterial &m);
void gcm_solid_material(const pna_gpu_cipher *ci, const uint8_t salt_prefix[39], int compression, GcmMaterial &m);
void solid_archive_head(std::vector<uint8_t> &head, int compression, const pna_gpu_cipher *ci, const uint8_t *ivs);
uint64_t chunk_limit(uint32_t max_chunk);
size_t meta_len(const pna_gpu_entry_meta *m, size_t e);
bool meta_blob_ok(const uint8_t *p, size_t n);
int  check_meta(pna_gpu_ctx *c, const pna_gpu_entry_meta *meta, size_t n);
// the checks of pna_gpu_entry_kinds_check, then every non-file's record into `out` (kinds == NULL or kinds->kind == NULL: `out` stays empty -- all files)
int  build_entry_records(pna_gpu_ctx *c, size_t n, const char *const *names, const uint64_t *src_len, const pna_gpu_entry_kinds *kinds,
                         const pna_gpu_entry_meta *meta, uint32_t max_chunk, EntryRecords &out);
// FHED | fSIZ | rest  ->  FHED | extra | fSIZ | facets | rest: entry e's metadata chunks where NormalEntry::write_chunks_to puts them
void splice_meta(std::vector<uint8_t> &pre, const pna_gpu_entry_meta *m, size_t e);
// pna_gpu_create_solid_archive_enc_device and its tree form (meta, max_chunk, kinds: NULL / 0 for the former)
int  create_solid_device_impl(pna_gpu_ctx *c, int algo, int level, size_t n, const char *const *names, const void *d_src, const uint64_t *src_off, const uint64_t *src_len,
                              const pna_gpu_cipher *cipher, const pna_gpu_entry_meta *meta, uint32_t max_chunk, const pna_gpu_entry_kinds *kinds,
                              void *d_dst, size_t dst_cap, uint64_t *archive_len, void *hip_stream);
int  run_subbatch(pna_gpu_ctx *c, int algo, const uint8_t *d_src, const uint64_t *src_off, const uint64_t *src_len,
                  size_t e0, size_t e1, uint8_t *d_dst, size_t dst_cap, uint64_t out_base, uint64_t *dst_off,
                  hipStream_t st, bool timed, const FrameJob *fj = nullptr);

// ---- the staging and copy layer of the host pipelines (pna_pipeline.cpp, pna_stream.cpp, the diff driver): thread count, parallel memcpy, copy streams,
// sink calls and slot reservation, each written once.
// Host threads that copy entries to or from page-locked memory: option stage_threads, or min(8, cores / 2)
inline unsigned staging_threads(const pna_gpu_ctx *c) {
    if (c && c->tun.stage_threads > 0) return (unsigned)c->tun.stage_threads;
    return std::min(8u, std::max(1u, std::thread::hardware_concurrency() / 2));
}
// n copies, job(i) = {dst, src, len}, on up to `threads` threads: on the calling thread when there is one job, one thread or less than `serial_below` bytes;
// otherwise the list is cut into CONTIGUOUS ranges balanced by bytes (adjacent small entries stay on one thread, a range ends behind the job that fills its
// share).  The threads are the call's own, not host_pool()'s: the stager thread copies while run_subbatch's per-entry loops hold the pool on the main thread,
// and a loop that finds the pool taken starts threads of its own (~0.5 ms a loop, DESIGN §5 "Many small entries").
struct CopyJob { uint8_t *dst; const uint8_t *src; uint64_t len; };
template <class J>
inline void parallel_copy(size_t n, unsigned threads, uint64_t serial_below, J &&job) {
    auto run = [&job](size_t a, size_t b) { for (size_t i = a; i < b; i++) { const CopyJob j = job(i); if (j.len) memcpy(j.dst, j.src, j.len); } };
    uint64_t total = 0;
    if (threads > 1 && n > 1) for (size_t i = 0; i < n; i++) total += job(i).len;
    if (threads <= 1 || n <= 1 || total < serial_below) { run(0, n); return; }
    std::vector<std::thread> th;
    const uint64_t per = (total + threads - 1) / threads;
    size_t e = 0;
    for (unsigned t = 0; t < threads && e < n; t++) {
        const size_t b = e; uint64_t acc = 0;
        while (e < n && (acc < per || t + 1 == threads)) acc += job(e++).len;
        th.emplace_back([&run, b, e]() { run(b, e); });
    }
    for (auto &x : th) x.join();
}
// the copy streams and slot events of the pipelined host paths, created on first use (the device is set)
inline int ensure_copy_lanes(pna_gpu_ctx *c) {
    if (c->cp_in) return PNA_OK;
    HIPCHK(c, hipStreamCreate(&c->cp_in)); HIPCHK(c, hipStreamCreate(&c->cp_out));
    for (auto &e : c->ev_in) HIPCHK(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
    for (auto &e : c->ev_out) HIPCHK(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
    return PNA_OK;
}
// a piece of the archive to the caller's sink (an empty piece is not handed on)
inline int sink_put(pna_gpu_ctx *c, pna_sink_fn sink, void *user, const void *p, size_t n) {
    return !n || sink(user, p, n) == 0 ? PNA_OK : fail(c, PNA_E_SINK, "sink failed");
}
// A pipeline's staging memory: every buffer (or array of slots) with its size, stated once; done() is the one PNA_E_NOMEM exit.
struct Reserve {
    pna_gpu_ctx *c; bool bad = false;
    template <class B> Reserve &add(B &buf, size_t bytes) { bad = bad || buf.ensure(bytes); return *this; }
    template <class B> Reserve &add(B *slots, size_t count, size_t bytes) { for (size_t s = 0; s < count; s++) add(slots[s], bytes); return *this; }
    int done() const { return bad ? fail(c, PNA_E_NOMEM, "staging allocation failed") : PNA_OK; }
};
