/*
 * include/pna_gpu.h -- C ABI of libpna_gpu.so, the MI355X-native replacement for the per-entry compression
 * path of ChanTsune/Portable-Network-Archive (reference paths relative to /root/reference).
 *
 * The reference has no FFI for this path; the seam is the crate-private Rust type
 *     enum CompressionWriter<W: Write> { No, Deflate(ZlibEncoder<W>), ZStd(ZstdEncoder<W>), Xz(..) }
 *     lib/src/compress.rs:21-76, constructed only by compression_writer() lib/src/entry/write.rs:251-265.
 * Each entry point below names the reference interface it replaces; INTEGRATION.md shows the Rust `extern "C"`
 * stub a maintainer would add behind the Compression::{ZStandard,Deflate} arms.
 *
 * Conventions: every function returns 0 (PNA_OK) or a negative PNA_E_* code; no global state; a ctx may be used
 * from one thread at a time (the reference creates one encoder per rayon task, cli/src/command/core.rs:505-517;
 * here one ctx owns one GPU and batches those tasks).  Pointers are host pointers unless the name says `_device`.
 * There is NO CPU fallback: without a usable HIP device pna_gpu_init fails with PNA_E_NODEVICE.
 */
#ifndef PNA_GPU_H
#define PNA_GPU_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PNA_OK            0
#define PNA_E_NODEVICE   (-1)   /* no HIP device / HIP runtime error at init                        */
#define PNA_E_INVAL      (-2)   /* bad argument (io::ErrorKind::InvalidInput in the reference)       */
#define PNA_E_NOMEM      (-3)   /* device or host allocation failed                                  */
#define PNA_E_DSTSIZE    (-4)   /* destination capacity smaller than pna_gpu_bound()                 */
#define PNA_E_HIP        (-5)   /* a HIP call or kernel failed; pna_gpu_last_error() has the text    */
#define PNA_E_SINK       (-6)   /* the sink callback (== W::write) returned non-zero                 */
#define PNA_E_UNSUPPORTED (-7)  /* algorithm not offered by this build                               */

/* == Compression::to_byte(), lib/src/entry/options.rs:241-247 */
#define PNA_ALGO_STORE    0
#define PNA_ALGO_DEFLATE  1
#define PNA_ALGO_ZSTD     2
#define PNA_ALGO_XZ       4     /* == Compression::XZ.to_byte(); decoded everywhere; WRITTEN only with option "xz_encode" = 1, by pna_gpu_compress_batch[_device] and the
                                 * non-solid archive entry points (below: "XZ ON THE WRITE SIDE"); without the option every compress entry point answers PNA_E_UNSUPPORTED */

/* encoder feature bits (pna_gpu_init flags, low byte); default = all of them */
#define PNA_F_HUF   1u
#define PNA_F_FSE   2u
#define PNA_F_LAZY  4u
#define PNA_F_REP   8u
#define PNA_F_FAR   0x10u       /* zstd: look-back over the whole 1 MiB segment (candidates beyond the LDS window verified in HBM / L2) */
#define PNA_F_ADOPT 0x20u       /* backward adoption: a match found late is moved back to its true start */
#define PNA_F_INS2  0x40u       /* only even positions enter the hash table (with PNA_F_ADOPT) */
#define PNA_F_STRONG 0x80u      /* third adoption round (up to 7 positions back) + two-step lazy deferral: the set of the high levels */
#define PNA_F_LZ_WAVEPARSE 0x4000u  /* testing: the split LZ stage with the wave-per-region parse kernel as its second half */
#define PNA_F_LZ_FUSED 0x8000u     /* the LZ stage as ONE kernel (match + parse in k_lz) instead of the default split form (match kernel ->
                                     * one word per input byte in a workspace of up to 16 GiB -> parse kernel): same bytes, ~20 % slower,
                                     * no workspace; the library falls back to it by itself when the workspace cannot be allocated */
#define PNA_F_DEFAULT 0x80000000u   /* let the library choose */

typedef struct pna_gpu_ctx pna_gpu_ctx;
/* == W::write of the reference's sink: non-zero return aborts with PNA_E_SINK */
typedef int (*pna_sink_fn)(void *user, const void *buf, size_t len);

/* One context per (process, GPU).  Replaces the per-entry encoder construction
 * ZstdEncoder::new(writer, level) / ZlibEncoder::new(writer, level) (lib/src/entry/write.rs:257-262). */
int  pna_gpu_init(pna_gpu_ctx **out, int device_id, uint32_t flags);
void pna_gpu_shutdown(pna_gpu_ctx *ctx);
const char *pna_gpu_last_error(const pna_gpu_ctx *ctx);
/* Tuning knobs of a context.  Each starts from an environment variable that pna_gpu_init reads ONCE (named in brackets); no entry point
 * consults the environment afterwards.  PNA_E_INVAL for unknown names and values out of range.
 *   "blk_log" [PNA_BLK_LOG]               block size of every batch = 1 << value (13..17); 0 = chosen by batch size (default)
 *   "unit_log" [PNA_LZ_UNIT_LOG]          LZ-stage units of 1 << value bytes (block size..20); 0 = chosen by batch size (default)
 *   "latency_max_mib" [PNA_LATENCY_MAX_MIB]  batches of at most this many MiB of input run in LATENCY MODE (default 128; 0 = never): smaller
 *                                         blocks inside the same frames and one LZ workgroup per unit instead of per segment, so that a handful
 *                                         of entries -- the CompressionWriter seam under the reference's thread pool -- fills the chip.  Same
 *                                         format, same decoders; ratio -0.1 .. -0.3 % (block headers).  pna_gpu_last_timing reports what was chosen.
 *                                         zstd calls beyond the mode still take smaller blocks by their input (32 KiB up to 384 MiB, 64 KiB up to 1 GiB, 128 KiB
 *                                         beyond: a batch's time below ~1 GiB is its blocks' chains); 0 = never AND 128 KiB blocks whatever the batch.
 *   "hist_by_block" [PNA_HIST_BY_BLOCK]   zstd entropy stage with statistics per block and three-lane state chains (1) or per segment and the one-kernel
 *                                         sequence coder (0); -1 (default): the first up to 40 960 blocks per sub-batch.  Same bytes either way.
 *   "lz_split" [PNA_LZ_SPLIT]             0 one-kernel LZ stage, 1 split form for long runs (default), 2 split form with the wave-per-region parse
 *   "lz_split_blocks" [PNA_LZ_SPLIT_BLOCKS]  blocks per run of the split form (default 131 072 = 16 GiB of input, 48 GiB of workspace; halved while the workspace cannot be had)
 *   "lz_split_min" [PNA_LZ_SPLIT_MIN]     shortest run, in segments, that takes the split form (default 0: every run)
 *   "lz_pbuf_fail" [PNA_LZ_PBUF_FAIL]     testing: behave as if the split form's workspace could not be allocated
 *   "win32k" [PNA_WIN32K]                 LDS geometry of the zstd match finder: 1 (default) the light and default level sets (zstd 2, 3) on a 32 KiB window, the high set (4 .. 9) on
 *                                         a 16 KiB window; 0: both on 64 KiB; 2: both on 16 KiB.  Other bytes, same format
 *   "tab3" [PNA_TAB3]                     the hash table of the zstd light / default / high sets: 1 (default) PACKED, three 21-bit entries (even position + 2-bit tag) per
 *                                         64-bit LDS word -- 49 062 slots next to the 32 KiB window, 55 206 next to the 16 KiB one; 0: one 32-bit entry per slot
 *                                         (32 704 / 36 800: round 3's table).  Other bytes (ratio 2.847 against 2.759 on text at the default level), same format
 *   "seq_hist" [PNA_SEQ_HIST]             1 (default): large zstd batches -- the parse kernel of the split LZ stage counts every block's sequence codes, the statistics kernel walks the literals only; 0: it
 *                                         reads the sequences once more.  Same bytes
 *   "far1" [PNA_FAR1]                     1 (default): the zstd light / default sets (levels 2, 3: packed table, 32 KiB window) verify at most 63 candidates beyond the match kernel's LDS window
 *                                         per wave of 256 positions -- one compacted round of far candidates -- and drop the rest (round 5: - 0.16 % of ratio, - 8.5 % of the match kernel);
 *                                         0: every far candidate, in as many rounds as it takes.  Other bytes, same format
 *   "strong2" [PNA_STRONG2]               1 (default): zstd levels 4 .. 22 (the high and max sets) on their standard geometries run a fourth backward-adoption round over eight positions and count up to
 *                                         15 back bytes (round 5: the high set 2.860 -> 2.883 on text, 10 - 22 2.977 -> 3.002); 0: the default level's three rounds.  Other bytes, same format
 *   "small_geometry" [PNA_SMALL_GEOMETRY] 1 (default): segments of at most 16 KiB -- small entries, the tail of longer ones -- are matched by one wave each with look-ups and inserts
 *                                         alternating per 256 positions (k_lzms) instead of by a workgroup per 4 096: such a segment's first tile finds nothing in the large
 *                                         geometry (4 KiB text entries: ratio 1.77 -> 2.04, libzstd -3: 2.05).  0: the large geometry for every segment.  Other bytes, same format
 *   "mtile" [PNA_MTILE]                   0 (default): the match kernel of the large geometry (k_lzm, segments above 16 KiB) looks up all 4 096 positions of a tile before it inserts
 *                                         any of them, so a position sees nothing less than a tile back.  256, 512, 1024 or 2048: look-ups and inserts alternate per sub-tile of that
 *                                         many positions inside the tile, and a position finds the matches a few hundred bytes back that real text, sources and binaries are made of
 *                                         (oracle: mtile; README has the measured cost and gain).  Any other value is PNA_E_INVAL.  Covers every set whose table lies in LDS -- zstd
 *                                         1 .. 9 and deflate 1 .. 9 --, on every path that compresses through the context.  With it such segments always take the split form of the LZ
 *                                         stage (lz_split, lz_split_min and PNA_F_LZ_FUSED no longer choose the one-kernel form, which has no sub-tiles; lz_split = 2 remains), the
 *                                         latency mode keeps its small blocks but runs whole segments (pna_gpu_timing.lz_units == 0; an explicit unit_log is overridden, and there are
 *                                         no tail units), and a words workspace that cannot be had is PNA_E_NOMEM instead of a fall-back.  NOT covered: zstd 10 .. 22 (table in global
 *                                         memory) ignore the option; segments of at most 16 KiB run the small geometry as before (its sub-tiles are 256 positions anyway; with
 *                                         small_geometry = 0 they run the large geometry with these sub-tiles).  Other bytes, same format
 *   "single_frame" [PNA_SINGLE_FRAME]     zstd: 1 = an entry's payload is ONE frame (one frame header, the 1 MiB segments' blocks behind each other, matches never
 *                                         cross a segment start) as the reference's encoder writes (lib/src/compress/zstandard.rs: one Encoder per entry);
 *                                         0 (default) = a frame per 1 MiB segment, which this library's decoder takes in parallel.  3 + 0..2 bytes per segment apart
 *   "zexec_par_min_mib" [PNA_ZEXEC_PAR_MIN_MIB]  decoder: single zstd frames of at least this many MiB (default 8; any size) take the header walk +
 *                                         wave-per-block parse + pointer-jumping execution; 0 = never
 *   "zdec_fallback_max_mib" [PNA_ZDEC_FALLBACK_MAX_MIB]  decoder: a zstd frame of more content than this that the parallel paths cannot take is refused (PNA_E_UNSUPPORTED)
 *                                         instead of decoded by one workgroup at ~11 MiB/s; 0 (default): no limit
 *   "zexec_win_mib" [PNA_ZEXEC_WIN_MIB]   decoder: the pointer-jumping execution runs a frame / stream in windows of whole blocks of at most this many MiB of output,
 *                                         one after the other (default and maximum 1 024: a word counts 31 bits from its window's start; scratch = 4 bytes per byte of a window)
 *   "stream_batch_mib" [PNA_STREAM_BATCH_MIB] (256), "stream_overlap_mib" [PNA_STREAM_OVERLAP_MIB] (24), "stream_gather_wgs" [PNA_STREAM_GATHER_WGS] (48): the streaming
 *                                         facade's pipeline -- largest device batch, how much may queue before a second batch is cut while one is on the device,
 *                                         workgroups of the copy-in kernel
 *   "lazy2" [PNA_LAZY2]                   how far a start looks ahead before it is taken, beyond the next position: 2 (default), 1, 0
 *   "strong_gtab" [PNA_STRONG_GTAB]       zstd levels 10..22 with the hash table in global memory (1, default) or in LDS (0)
 *   "lit_beside_seq" [PNA_LIT_BESIDE_SEQ] large zstd batches: the literal coder on a second stream next to the sequence coder (1, default)
 *   "xz_encode" [PNA_XZ_ENCODE]           0 (default): PNA_ALGO_XZ is PNA_E_UNSUPPORTED on every compress entry point; 1: the batch and the non-solid archive entry points write
 *                                         xz.  An option because these streams are multi-block with per-chunk state resets: their bytes differ from the reference's encoder
 *                                         (one block, one running model) and their ratio is lower -- a host chooses that knowingly ("XZ ON THE WRITE SIDE" below)
 *   "camellia" [PNA_CAMELLIA]             0 (default): PNA_ENC_CAMELLIA is PNA_E_UNSUPPORTED on every entry point that takes a cipher, and the read side refuses / reports
 *                                         PNA_VERIFY_UNSUPPORTED for Camellia entries; 1: Camellia-256 in CTR, CBC and GCM STREAM wherever AES-256 is taken -- the archive
 *                                         entry points (solid: CTR and GCM), pna_gpu_cipher_apply_device (CTR, CBC encryption), and extract / verify / diff / extract-select
 *                                         (k_cipher.hip).  An option so that a host which keeps the reference's CipherWriter for Camellia sees no change
 *   "kdf_device" [PNA_KDF_DEVICE]         0 (default): extract / verify / diff / extract-select derive every key on the host, one PHSF string after the other, as before;
 *                                         N >= 1: a window's distinct, not yet derived PHSF strings go through pna_gpu_kdf_batch when there are at least N of them (fewer:
 *                                         the host).  pna_gpu_kdf_batch called directly does not look at it ("KEY DERIVATION ON THE DEVICE" below)
 *   "kdf_mem_mib" [PNA_KDF_MEM_MIB]       MiB that pna_gpu_kdf_batch's Argon2 block memory may take (one allocation, kept by the context); 0 (default): a quarter of the
 *                                         device's free memory at the first batch, at most 32 GiB.  A batch runs in as many rounds as its jobs need to fit
 *   "max_chunk_size" [PNA_MAX_CHUNK_SIZE] (FDAT chunk size of the entry points without such a parameter), "sub_mib" [PNA_SUB_MIB], "stage_threads" [PNA_STAGE_THREADS],
 *   "diff_slot_mib" [PNA_DIFF_SLOT_MIB]   pna_gpu_diff_archive_host: MiB of each of the two page-locked (and two device) slots the files' bytes travel through (256)
 *   "extract_win_mib" [PNA_EXTRACT_WIN_MIB], "batch_piece_mib" [PNA_BATCH_PIECE_MIB], "inflate_serial" [PNA_INFLATE_SERIAL],
 *   "zdec_serial" [PNA_ZDEC_SERIAL], "zdec_dbg" [PNA_ZDEC_DBG] (diagnostics of the one-workgroup zstd decoder: bit 8 = small re-base distances, for its test), "stream_pool_mib" [PNA_STREAM_POOL_MIB], "stream_linger_us" [PNA_STREAM_LINGER_US] (-1 = adaptive): DESIGN.md. */
int  pna_gpu_set_option(pna_gpu_ctx *ctx, const char *name, long value);
const char *pna_gpu_strerror(int code);

/* Worst-case compressed size of one entry (zstd: ZSTD_compressBound-like; zlib: deflateBound-like; xz: every chunk stored -- 3 bytes per 8 KiB, the smallest
 * LZ block --, 24 bytes per 1 MiB block (header, end marker, padding, CRC64), 8 per Index record, 32 + the record count for stream header, Index framing and footer). */
size_t pna_gpu_bound(int algo, size_t src_len);

/* Level mapping of the reference, restated so callers can pass CompressionLevel values through unchanged:
 * lib/src/compress/zstandard.rs:43-57 (Default -> 3, clamp to min..max) and lib/src/compress/deflate.rs:89-101
 * (Default -> 6, clamp 0..9), lib/src/compress/xz.rs:36-46 (Default -> 6, clamp 0..9).  `level` < 0 with level == PNA_LEVEL_DEFAULT means default. */
/* The encoder has these parameter sets behind that scale ("Level sets"):
 *   stored   deflate 0 = Compression::none(): stored blocks only (zlib header 78 01)
 *   fast     zstd < 0 and 1, deflate 1..3: every position in the table, lazy deferral, look-back = the LDS window
 *   light    zstd 2: even-position PACKED table next to a 32 KiB window, backward adoption (two rounds), 1 MiB look-back, lazy deferral over three positions
 *   default  zstd 0 and 3..5: light + a third adoption round (up to 7 positions back) and two-step lazy deferral;  deflate 4..8: even-position table,
 *            adoption, lazy deferral over three positions
 *   high     zstd 6..9: default on a 16 KiB window with 55 206 slots;  deflate 9: + the third adoption round and two-step lazy deferral
 *   max      zstd 10..22: + the hash table in global memory, 2^19 slots per segment
 * xz runs zstd's LZ stage with matches of at most 273 bytes: xz 0 = the fast set (zstd 1), 1..3 = the default set (zstd 3), 4..6 = the high set (zstd 6..9),
 * 7..9 = the max set (zstd 10..22). */
#define PNA_LEVEL_DEFAULT  (-1000)
int  pna_gpu_clamp_level(int algo, int level);

/* XZ ON THE WRITE SIDE (option "xz_encode" = 1; the reference: XzEncoder::new(writer, level), lib/src/entry/write.rs:257-263).  Every stream is one that stock
 * liblzma decodes; its bytes are NOT liblzma's:
 *   per entry   one .xz stream: stream header (check = CRC64, liblzma's default), one block per 1 MiB segment of the entry, the Index, the stream footer; an empty
 *               entry is the 32-byte stream without a block.
 *   per block   a 12-byte header without size fields, one filter: LZMA2, dictionary-size byte 16 (1 MiB: the LZ stage never looks back beyond its segment); the
 *               chunks, the 0x00 end marker, padding to 4, the CRC64 of the segment's input bytes.
 *   per chunk   one LZMA2 chunk per LZ block of at most 64 KiB (option "blk_log": at most 16 here; a batch whose longest entry is shorter takes the power of two
 *               that holds it, 8 KiB at least; a batch in LATENCY MODE takes zstd's blocks there, 16 KiB up to 32 MiB of input and 32 KiB beyond -- a chunk is one
 *               serial chain --, but whole segments: the LZ stage's units are not used).  Every LZMA chunk resets the state and carries the properties lc 3, lp 0, pb 2 (control 0xE0 for a block's first
 *               chunk, 0xC0 for the others); the dictionary is reset at a block's start only, so matches reach back over the segment's earlier chunks.  A chunk
 *               whose LZMA form with its 6-byte header would not be smaller than its input with the 3-byte header of an uncompressed chunk is written as
 *               the latter (0x01 at a block's start, 0x02 elsewhere): no chunk takes more than its input + 3 bytes, which pna_gpu_bound relies on.  Match lengths are at
 *               most 273; a distance among the chunk's four latest is coded as a repeat.  The parse is the LZ stage's (greedy / lazy), not an optimal one.
 *   That independence of the chunks is the parallelism (one wave per chunk, k_xzenc.hip), and what it costs in ratio.
 * Entry points that take PNA_ALGO_XZ with the option: pna_gpu_compress_batch, pna_gpu_compress_batch_device, pna_gpu_create_archive_device and its _part, _enc,
 *   _meta and _chunked forms, pna_gpu_create_archive_host and its _enc, _meta, _chunked and _part forms (FHED compression byte 4; the cipher stage and the chunk
 *   cut work on payload bytes).  An entry is always coded inside one sub-batch -- its Index is sized over all its blocks --, so an entry whose workspace (about
 *   3.5 bytes per input byte) cannot be allocated fails with PNA_E_NOMEM instead of being cut; pna_gpu_last_error then names this limit, the sub-batch's and its
 *   longest entry's input bytes and the workspace they need.
 * PNA_E_UNSUPPORTED with or without the option: the solid entry points (pna_gpu_create_solid_archive_*), pna_gpu_compress_solid, the streaming facade
 *   (pna_gpu_stream_*) and pna_gpu_stream_entry_*; xz blocks smaller than a segment, other lc / lp / pb, an optimal parse: not built.
 * pna_gpu_last_timing of an xz call: ms_lz the LZ stage, ms_stats the CRC64 kernel, ms_lit the chunk coder, ms_seq sizes and offsets. */

/* STORED ENTRIES ON THE DEVICE (PNA_ALGO_STORE; the reference: Compression::No, `pna create --store`, CompressionWriter's arm without an encoder).  No codec
 * runs and the level is ignored (pna_gpu_clamp_level(PNA_ALGO_STORE, x) = 0): every payload length is known on the host, so the layout needs no device scan
 * and no read-back, and a payload goes from the source buffer to its place in the archive in ONE pass (k_store.hip) that also leaves the CRC-32 of what it
 * moved; k_store_fold turns those into the FDAT CRC fields and FEND.  Under a cipher the copy runs alone, the cipher stage works on the payloads where they
 * stand and the chunk CRC is taken over the ciphertext (k_frame), as on the compressed paths.
 *   record      FHED(kind 0, compression 0, enc, mode) | extra | fSIZ | facets | [PHSF] | [FDAT(iv or GCM stream header)] | FDAT(payload)* | FEND, byte-exact with
 *               the reference for given IVs; the payload stream is cut at max_chunk_size as FlattenWriter cuts it.  An empty file without a cipher has NO FDAT
 *               (FlattenWriter ignores empty writes), with CTR the IV chunk alone, with CBC the IV chunk and one padding block, with GCM STREAM the header and the
 *               empty final segment's tag.  As for the other algos a CBC or GCM entry must fit one chunk, and the IV / stream header is one chunk whatever
 *               max_chunk_size says.
 *   taken by    pna_gpu_create_archive_device and its _part, _enc, _meta, _chunked and _tree forms; pna_gpu_create_archive_host and its _enc, _meta, _chunked,
 *               _part and _tree forms; every pna_gpu_archive_*_bound (never below the bytes written).  Like every other algo a destination needs 16 bytes of room
 *               behind the last record wherever k_frame runs -- under a cipher and, without one, in the unfused form (option "store_unfused"; the default picks it
 *               for sub-batches whose longest chunk lies between 4 KiB and 1 MiB); only a call whose sub-batches all take the fused form gets by with a
 *               destination of exactly the archive's size.  Size the destination with the bound functions.  pna_gpu_append_archive_host reaches the _part form
 *               unchanged and takes PNA_ALGO_STORE with it.  AES in all three modes; Camellia under option "camellia", as elsewhere.  The device forms want
 *               16-byte aligned src_off, as for every algo.
 *   solid       pna_gpu_create_solid_archive_device, _enc_device and _tree_device: the serialised inner records ARE the stream -- k_store writes the inner payloads
 *               at their places in the destination's SDAT bodies, the inner FDAT CRCs come from the fold, nothing is copied twice.  SHED(compression 0, ..) |
 *               [PHSF] | [SDAT(iv / header)] | SDAT* | SEND, the stream cut into SDAT chunks of max_chunk_size bytes (default: one chunk up to 2^32 - 5 bytes;
 *               GCM STREAM: one chunk per segment).  For a stream of one chunk without a cipher the bytes are pna_create_archive(.., PNA_ALGO_STORE, solid = 1, ..)'s.
 *               The reference's own SDAT cut follows the write calls of its chunk writer and is not reproduced: as for every compressed solid stream here the
 *               guarantee is the decoded inner stream, not the SDAT boundaries.  CTR and GCM as for the other algos, CBC stays PNA_E_UNSUPPORTED.
 *               pna_gpu_create_solid_archive_host, _enc_host and _tree_host stream the stored stream in windows of "solid_win_mib" MiB like the compressed ones
 *               (GCM STREAM: of whole segments): a window's bytes go out as the parts of the SDAT chunks they belong to, the CRC register of a chunk that spans
 *               windows is chained from window to window and its CRC written with its last byte (k_crc_patch).  The bytes equal the device form's at every
 *               window size.
 *   not covered pna_create_archive keeps its host loop for PNA_ALGO_STORE (it needs no GPU).  pna_gpu_compress_batch[_device], pna_gpu_compress_solid, the
 *               streaming facade (pna_gpu_stream_*), pna_gpu_stream_entry_* and pna_gpu_create_archive_multi_host answer PNA_E_UNSUPPORTED as before.
 *   option      "store_unfused" [PNA_STORE_UNFUSED] which form payloads without a cipher take -- 0: the fused k_store + k_store_fold (one read of the payload);
 *               1: the copy-only form and k_frame (two reads, a chunk's CRC on one workgroup); -1 (default): per sub-batch by its longest data chunk -- fused
 *               above 1 MiB (a large entry is not CRC'd by one workgroup) and up to 4 KiB, unfused between: 10 000 x 1 MiB measured 8.6 ms unfused against
 *               12.2 ms fused, one entry of 4 GiB 839 ms against 4.6 ms (profiles/store_rate.txt).  The bytes are the same.  Stored solid streams always
 *               take the fused form for their inner payloads.
 * pna_gpu_debug_store_stats: the context's latest create call with PNA_ALGO_STORE (any pointer may be NULL) -- pieces (of at most 1 MiB of one data chunk) that
 * went through the fused k_store, pieces through its copy-only form, data chunks folded by k_store_fold, HIP-event milliseconds of the k_store launches. */
int  pna_gpu_debug_store_stats(pna_gpu_ctx *ctx, uint64_t *pieces_fused, uint64_t *pieces_copy_only, uint64_t *chunks_folded, double *ms_k_store);

/* ---- batch of independent entries: the data-parallel fan-out of spawn_entry_results()/create_entry()
 * (cli/src/command/core.rs:496-537,915-977).  Entry i becomes one independent stream in dst[i]
 * (zstd: concatenated frames; deflate: one zlib stream), exactly what FileEntryBuilder::build() hands to
 * NormalEntry as FDAT payload (lib/src/entry/builder/file.rs:131-135). */
int  pna_gpu_compress_batch(pna_gpu_ctx *ctx, int algo, int level, size_t n,
                            const void *const *src, const size_t *src_len,
                            void *const *dst, const size_t *dst_cap, size_t *dst_len);

/* Same, with the inputs already resident in HBM (bench / pipelined callers).
 *   d_src      device buffer holding all entries; entry i = [src_off[i], src_off[i] + src_len[i]);
 *              every src_off[i] must be a multiple of 16 and the buffer must extend 4 KiB past the last entry.
 *   d_dst      device buffer of dst_cap bytes receiving the compressed entries back to back.
 *   dst_off    host array of n+1 offsets (out): entry i's stream = d_dst[dst_off[i] .. dst_off[i+1]).
 * Work is enqueued on `hip_stream` (a hipStream_t, or NULL for the ctx's own stream) and the call returns after
 * the stream has finished (dst_off needs the sizes). */
int  pna_gpu_compress_batch_device(pna_gpu_ctx *ctx, int algo, int level, size_t n,
                                   const void *d_src, const uint64_t *src_off, const uint64_t *src_len,
                                   void *d_dst, size_t dst_cap, uint64_t *dst_off, void *hip_stream);

/* ---- non-solid archive assembled in HBM: what create_archive_file() (cli/src/command/create.rs:575-635) writes through
 * Archive::write_header / add_entry / finalize (lib/src/archive/write.rs:92-101,368-370,438-441) for file entries whose
 * records are FHED | fSIZ | FDAT | FEND (NormalEntry::write_chunks_to, lib/src/entry.rs:895-911; write_chunk and its
 * CRC-32, lib/src/io.rs:183-197, lib/src/format/chunk.rs:7-12).  The compressed payloads are written once, straight at
 * their archive offsets; the FDAT CRCs are computed on the device.  Same inputs as pna_gpu_compress_batch_device plus
 * names[i] (host strings, sanitised like EntryName::sanitize).  d_dst: 16-byte aligned device buffer of at least
 * pna_gpu_archive_bound() bytes; on return d_dst[0 .. *archive_len) is the complete .pna file and, if entry_off is not
 * NULL, entry_off[i] (n + 1 values) is the offset of entry i's FHED chunk.  Byte-identical to pna_create_archive()
 * (include/pna_archive.h) over the same entries. */
size_t pna_gpu_archive_bound(int algo, size_t n, const char *const *names, const uint64_t *src_len);
/* One shard of an archive whose entries are split over several producers (one rank per GPU): only the shard with
 * PNA_PART_HEAD carries the signature + AHED, only the one with PNA_PART_TAIL the AEND; the shards' outputs concatenated
 * in entry order are the archive (the ordered drain of drain_entry_results, cli/src/command/core.rs:471-493). */
#define PNA_PART_HEAD 1u
#define PNA_PART_TAIL 2u
int  pna_gpu_create_archive_part_device(pna_gpu_ctx *ctx, int algo, int level, size_t n, const char *const *names,
                                        const void *d_src, const uint64_t *src_off, const uint64_t *src_len,
                                        void *d_dst, size_t dst_cap, uint64_t *entry_off, uint64_t *archive_len,
                                        uint32_t part_flags, void *hip_stream);
int  pna_gpu_create_archive_device(pna_gpu_ctx *ctx, int algo, int level, size_t n, const char *const *names,
                                   const void *d_src, const uint64_t *src_off, const uint64_t *src_len,
                                   void *d_dst, size_t dst_cap, uint64_t *entry_off, uint64_t *archive_len,
                                   void *hip_stream);

/* ---- cipher stage: the reference stacks compress -> cipher -> sink (get_writer, lib/src/entry/write.rs:268-274); the cipher
 * writers CipherWriter::{CtrAes, CbcAes} (encryption_writer, lib/src/entry/write.rs:189-248: Ctr128BE<Aes256>, CBC + PKCS#7) run
 * here as kernels over the compressed payload where it already sits in the archive buffer, before the chunk CRC-32.
 * The key is the password hash the Rust host derives once per WriteOptions (derive_key_material, lib/src/entry/write.rs:64-72;
 * pna_kdf_pbkdf2_sha256 in pna_archive.h is the C++ host's equivalent); `phsf` is the PHC string that goes into each entry's PHSF
 * chunk.  Every entry gets its own IV (random::random_vec in to_hashed, lib/src/entry/write.rs:108-121): ivs[16 * i ..) for
 * entry i, or NULL to draw them from the OS.  Entry record: FHED(encryption, cipher_mode) | fSIZ | PHSF | FDAT(iv) |
 * FDAT(ciphertext) | FEND (lib/src/entry.rs:895-911; the IV is its own data piece: prepend_data_prefix, lib/src/entry/builder.rs:62-69). */
#define PNA_ENC_NONE      0     /* == Encryption::to_byte(), lib/src/entry/options.rs */
#define PNA_ENC_AES       1
#define PNA_ENC_CAMELLIA  2     /* Camellia-256, in the modes and on the entry points of AES-256 -- on a context with option "camellia" = 1; PNA_E_UNSUPPORTED unless option "camellia" is set */
#define PNA_MODE_CBC      0     /* == CipherMode::to_byte() */
#define PNA_MODE_CTR      1
#define PNA_MODE_GCM      2     /* "GCM STREAM": lib/src/cipher/aead.rs, lib/src/cipher/gcm.rs */
typedef struct {
    int encryption;             /* PNA_ENC_* */
    int cipher_mode;            /* PNA_MODE_* */
    uint8_t key[32];            /* AES-256 / Camellia-256 key; GCM: K_master, the per-entry stream keys are derived from it (HKDF) */
    const char *phsf;           /* body of the PHSF chunk */
    const uint8_t *ivs;         /* CBC / CTR: n x 16 bytes; GCM: n x 39 bytes (salt[32] || nonce_prefix[7] per entry); or NULL */
    uint32_t gcm_segment_size;  /* GCM: segment size written into the stream header (0 = 1 MiB, the reference's DEFAULT_SEGMENT_SIZE; at most 64 MiB) */
} pna_gpu_cipher;
/* PNA_MODE_GCM (archive entry points, non-solid): entry record FHED(enc, 2) | fSIZ | PHSF | FDAT(stream header, 75 bytes) |
 * FDAT(ciphertext || tag) | FEND.  The stream key is HKDF(K_master, salt, entry context) with the context bound to the entry's FHED
 * chunk and the PHSF string (derive_stream_key, aead.rs:184-199).  The payload is cut into segments of gcm_segment_size bytes, each
 * followed by its 16-byte tag (GcmEncryptWriter, lib/src/cipher/gcm.rs:48-100): nonce = prefix || counter || flag, flag 1 on the last
 * segment (an empty payload is one empty final segment).  An entry whose payload spans several FDAT chunks (beyond max_chunk_size) is
 * PNA_E_UNSUPPORTED with GCM. */
size_t pna_gpu_archive_enc_bound(int algo, size_t n, const char *const *names, const uint64_t *src_len, const pna_gpu_cipher *cipher);
/* pna_gpu_create_archive_part_device with a cipher (cipher == NULL or encryption == PNA_ENC_NONE: identical to it). */
int  pna_gpu_create_archive_enc_device(pna_gpu_ctx *ctx, int algo, int level, size_t n, const char *const *names,
                                       const void *d_src, const uint64_t *src_off, const uint64_t *src_len,
                                       const pna_gpu_cipher *cipher, void *d_dst, size_t dst_cap, uint64_t *entry_off,
                                       uint64_t *archive_len, uint32_t part_flags, void *hip_stream);
/* Per-entry metadata: chunks the host has ALREADY framed (length | type | data | CRC-32) and that NormalEntry::write_chunks_to places
 * around fSIZ (lib/src/entry.rs:895-911): `extra[i]` between FHED and fSIZ (user-defined chunks), `facets[i]` between fSIZ and PHSF / FDAT
 * (cTIM mTIM aTIM fPRM fUId fGId fONm fGNm xATR ...: try_for_each_metadata_facet, lib/src/entry.rs:124-180) -- what `pna create
 * --keep-timestamp --keep-permission --keep-xattr` adds.  NULL arrays or zero lengths mean none.  Every blob is checked (chunk lengths,
 * CRCs, none of the chunk types this library writes itself): PNA_E_INVAL otherwise.  The caller's bound grows by the blobs' lengths. */
typedef struct {
    const void *const *extra;  const size_t *extra_len;
    const void *const *facets; const size_t *facets_len;
} pna_gpu_entry_meta;
int  pna_gpu_create_archive_meta_device(pna_gpu_ctx *ctx, int algo, int level, size_t n, const char *const *names,
                                        const void *d_src, const uint64_t *src_off, const uint64_t *src_len,
                                        const pna_gpu_cipher *cipher, const pna_gpu_entry_meta *meta, void *d_dst, size_t dst_cap,
                                        uint64_t *entry_off, uint64_t *archive_len, uint32_t part_flags, void *hip_stream);
int  pna_gpu_create_archive_meta_host(pna_gpu_ctx *ctx, int algo, int level, size_t n, const char *const *names,
                                      const void *const *src, const size_t *src_len, const pna_gpu_cipher *cipher,
                                      const pna_gpu_entry_meta *meta, pna_sink_fn sink, void *user);
/* FlattenWriter::max_chunk_size (lib/src/util/io.rs:60-77; FileEntryBuilder::max_chunk_size, lib/src/entry/builder/file.rs:105-112; default u32::MAX,
 * lib/src/chunk.rs:28): an entry's stream -- after the cipher -- is cut into FDAT chunks of exactly max_chunk_size bytes, the last one holding the rest
 * (an IV / stream header stays the data piece of its own that prepend_data_prefix makes it).  The general forms of the archive entry points take it as a
 * parameter (0 = u32::MAX); the entry points above and below without one use the context's option "max_chunk_size" (pna_gpu_set_option, default 0).
 * Byte-identical to the reference's chunking up to chunks of 2^32 - 5 bytes (the device CRC takes type + data as one message below 2^32 bytes: an entry
 * whose compressed payload exceeds 4 GiB - 5 bytes is cut 4 bytes earlier than the reference would).  CBC and GCM entries must fit one chunk
 * (PNA_E_UNSUPPORTED otherwise; CTR -- the CLI's default -- has no such limit).  Bound: pna_gpu_archive_chunked_bound (+ the meta blobs' lengths). */
size_t pna_gpu_archive_chunked_bound(int algo, size_t n, const char *const *names, const uint64_t *src_len, const pna_gpu_cipher *cipher, uint32_t max_chunk_size);
int  pna_gpu_create_archive_chunked_device(pna_gpu_ctx *ctx, int algo, int level, size_t n, const char *const *names,
                                           const void *d_src, const uint64_t *src_off, const uint64_t *src_len,
                                           const pna_gpu_cipher *cipher, const pna_gpu_entry_meta *meta, uint32_t max_chunk_size, void *d_dst, size_t dst_cap,
                                           uint64_t *entry_off, uint64_t *archive_len, uint32_t part_flags, void *hip_stream);
int  pna_gpu_create_archive_chunked_host(pna_gpu_ctx *ctx, int algo, int level, size_t n, const char *const *names,
                                         const void *const *src, const size_t *src_len, const pna_gpu_cipher *cipher,
                                         const pna_gpu_entry_meta *meta, uint32_t max_chunk_size, uint32_t part_flags, pna_sink_fn sink, void *user);
/* ENTRY KINDS: `pna create some/tree` in ONE call.  create_entry (cli/src/command/core.rs:915-977) has four arms and writes them in walk order: a hard link
 * (HardLinkEntryBuilder::new, core.rs:938-943), a symbolic link (SymlinkEntryBuilder::new, core.rs:945-955), a directory (DirEntryBuilder, EntryHeader::for_dir; kept by
 * default, --keep-dir) and files, everything else.  The pna_gpu_create_*_tree_* entry points take the arms as kind[i] next to entry i; they are their counterparts'
 * parameter lists plus `kinds` (and cipher, meta and max_chunk_size where the counterpart has none).
 *   directory   FHED(kind 1, compression 0, encryption 0, cipher_mode 0) | extra[i] | facets[i] | FEND -- no fSIZ, no PHSF, no FDAT: what pna_archive_add_dir writes.
 *   links       FHED(kind 2 / 3, 0, 0, 0) | extra[i] | facets[i] | FDAT(target)* | FEND.  No fSIZ: only DataKind::FILE records one (lib/src/entry/builder.rs:630-632).
 *               The target is STORED and NOT ENCRYPTED even when the call has a cipher: new_link takes WriteOptions::store() (builder.rs:341-349), which is what
 *               core.rs:938,948 call; max_chunk_size cuts it as FlattenWriter cuts any stream (lib/src/util/io.rs:60-77).
 *   names       sanitised exactly as file names are.  The host still does read_link and gathers the metadata facets; it passes them in `link` and `meta`.
 * For an entry that is not a file src_len[i] must be 0 (PNA_E_INVAL otherwise) and its source pointer / offset is ignored; an unknown kind, an empty link target and
 * link == NULL with a link kind present are PNA_E_INVAL (pna_gpu_entry_kinds_check: the same checks without a context).  kinds == NULL or kinds->kind == NULL: the
 * counterpart's bytes, byte for byte.  entry_off[i] is filled for every entry.  cipher->ivs stays indexed by entry i: the slots of entries that are not files are
 * unused (nothing of them reaches the archive; no cipher unit or stream key is made for such an entry).  In a solid stream the same records stand between the file records -- every inner entry
 * there is a stored record already; the solid tree forms also place the files' meta chunks and cut the files' data at max_chunk_size.  Such an entry has no
 * segment: a sub-batch of directories and links alone launches no codec, write or framing kernel (its records travel in one copy).
 * Not covered: pna_gpu_create_archive_multi_host, pna_gpu_append_archive_host (append is reachable through part_flags) and the pna_gpu_stream_entry_* writer. */
#define PNA_KIND_FILE 0         /* == DataKind::to_byte() */
#define PNA_KIND_DIRECTORY 1
#define PNA_KIND_SYMLINK 2
#define PNA_KIND_HARDLINK 3
typedef struct {
    const uint8_t *kind;            /* n bytes; NULL: all files */
    const void *const *link;        /* HOST memory: target bytes of entry i (kinds 2, 3), else ignored */
    const size_t *link_len;
} pna_gpu_entry_kinds;
int  pna_gpu_entry_kinds_check(size_t n, const uint64_t *src_len, const pna_gpu_entry_kinds *kinds);
/* pna_gpu_archive_chunked_bound + the meta blobs' lengths + the links' targets and their chunk framing */
size_t pna_gpu_archive_tree_bound(int algo, size_t n, const char *const *names, const uint64_t *src_len, const pna_gpu_cipher *cipher,
                                  const pna_gpu_entry_meta *meta, uint32_t max_chunk_size, const pna_gpu_entry_kinds *kinds);
int  pna_gpu_create_archive_tree_device(pna_gpu_ctx *ctx, int algo, int level, size_t n, const char *const *names,
                                        const void *d_src, const uint64_t *src_off, const uint64_t *src_len,
                                        const pna_gpu_cipher *cipher, const pna_gpu_entry_meta *meta, uint32_t max_chunk_size, const pna_gpu_entry_kinds *kinds,
                                        void *d_dst, size_t dst_cap, uint64_t *entry_off, uint64_t *archive_len, uint32_t part_flags, void *hip_stream);
int  pna_gpu_create_archive_tree_host(pna_gpu_ctx *ctx, int algo, int level, size_t n, const char *const *names,
                                      const void *const *src, const size_t *src_len, const pna_gpu_cipher *cipher,
                                      const pna_gpu_entry_meta *meta, uint32_t max_chunk_size, const pna_gpu_entry_kinds *kinds, uint32_t part_flags, pna_sink_fn sink, void *user);
/* The solid forms (pna_gpu_create_solid_archive_enc_device / _host below, and pna_gpu_solid_archive_enc_bound). */
size_t pna_gpu_solid_archive_tree_bound(int algo, size_t n, const char *const *names, const uint64_t *src_len, const pna_gpu_cipher *cipher,
                                        const pna_gpu_entry_meta *meta, uint32_t max_chunk_size, const pna_gpu_entry_kinds *kinds);
int  pna_gpu_create_solid_archive_tree_device(pna_gpu_ctx *ctx, int algo, int level, size_t n, const char *const *names,
                                              const void *d_src, const uint64_t *src_off, const uint64_t *src_len,
                                              const pna_gpu_cipher *cipher, const pna_gpu_entry_meta *meta, uint32_t max_chunk_size, const pna_gpu_entry_kinds *kinds,
                                              void *d_dst, size_t dst_cap, uint64_t *archive_len, void *hip_stream);
int  pna_gpu_create_solid_archive_tree_host(pna_gpu_ctx *ctx, int algo, int level, size_t n, const char *const *names,
                                            const void *const *src, const size_t *src_len, const pna_gpu_cipher *cipher,
                                            const pna_gpu_entry_meta *meta, uint32_t max_chunk_size, const pna_gpu_entry_kinds *kinds,
                                            pna_sink_fn sink, void *user);
/* pna_gpu_create_archive_host (bounded in-flight window from host memory) with the cipher stage. */
int  pna_gpu_create_archive_enc_host(pna_gpu_ctx *ctx, int algo, int level, size_t n, const char *const *names,
                                     const void *const *src, const size_t *src_len, const pna_gpu_cipher *cipher,
                                     pna_sink_fn sink, void *user);
/* The cipher alone, in place, over n byte ranges of a device buffer: range i = d_buf[off[i] .. off[i] + len[i]) is one cipher
 * stream with IV ivs[16 * i ..).  CTR: encrypt == decrypt (DecryptReader::CtrAes, lib/src/entry/read.rs:83-88).  CBC: encryption
 * only (decrypt != 0 is PNA_E_UNSUPPORTED); the ciphertext is (len / 16 + 1) * 16 bytes long, the caller leaves that room. */
int  pna_gpu_cipher_apply_device(pna_gpu_ctx *ctx, const pna_gpu_cipher *cipher, int decrypt, size_t n, void *d_buf,
                                 const uint64_t *off, const uint64_t *len, void *hip_stream);

/* `pna create --solid` assembled in HBM: the inner entries are serialised as STORE records (FHED | fSIZ | FDAT | FEND, their
 * CRC-32 on the device) into one stream, the stream is compressed as ONE entry and every segment's output becomes one SDAT
 * chunk between SHED and SEND (create_archive_file's solid branch, cli/src/command/create.rs:594-598,603-617;
 * lib/src/archive/write.rs:443-470,575-580,716-727; SolidHeader::to_bytes, lib/src/entry/header.rs:274-282).
 * Arguments as pna_gpu_create_archive_device; inner entries >= 2 GiB are rejected (one FDAT chunk each). */
size_t pna_gpu_solid_archive_bound(int algo, size_t n, const char *const *names, const uint64_t *src_len);
int  pna_gpu_create_solid_archive_device(pna_gpu_ctx *ctx, int algo, int level, size_t n, const char *const *names,
                                         const void *d_src, const uint64_t *src_off, const uint64_t *src_len,
                                         void *d_dst, size_t dst_cap, uint64_t *archive_len, void *hip_stream);

/* With a cipher: one cipher stream over all SDAT bodies (into_solid_archive takes any cipher, lib/src/archive/write.rs:443-470).
 *   CTR: SHED(encryption, cipher_mode) | PHSF | SDAT(iv) | SDAT(ciphertext)* | SEND; cipher->ivs is ONE 16-byte IV or NULL.
 *   GCM: SHED | PHSF | SDAT(stream header, 75 bytes) | SDAT(segment ciphertext || tag)* | SEND -- the GCM STREAM layout of
 *        pna_gpu_create_archive_enc_device over the compressed solid stream, the stream key bound to the SHED chunk (entry_context,
 *        lib/src/cipher/aead.rs:167-190); cipher->ivs is ONE salt(32) || nonce_prefix(7) or NULL.
 *   CBC encryption would be one serial chain over the whole stream: PNA_E_UNSUPPORTED (the extract driver decrypts CBC solid streams,
 *   which is parallel).
 * pna_gpu_solid_archive_enc_bound: the destination capacity to offer (cipher == NULL: the plain bound). */
size_t pna_gpu_solid_archive_enc_bound(int algo, size_t n, const char *const *names, const uint64_t *src_len, const pna_gpu_cipher *cipher);
int  pna_gpu_create_solid_archive_enc_device(pna_gpu_ctx *ctx, int algo, int level, size_t n, const char *const *names,
                                             const void *d_src, const uint64_t *src_off, const uint64_t *src_len,
                                             const pna_gpu_cipher *cipher, void *d_dst, size_t dst_cap, uint64_t *archive_len,
                                             void *hip_stream);

/* The same from host memory, STREAMING for zstd and deflate, as SolidArchive::add_entry feeds its one encoder (lib/src/archive/write.rs:575-580): the
 * serialised inner entries reach the device in windows of `solid_win_mib` MiB (256) through two page-locked slots each way -- about four windows of
 * page-locked memory whatever the archive's size --, the sink receives the head, one piece per window, the tail; inner entries of ANY size (FDAT chunks
 * of at most 2^32 - 5 bytes, FlattenWriter's cut, lib/src/util/io.rs:60-77).  deflate: one zlib stream over all windows, its Adler-32 carried from
 * window to window on the device.  The bytes equal pna_gpu_create_solid_archive_device's.  n == 0 and zstd's option single_frame: the whole stream in
 * flight at once, inner entries below 2 GiB. */
int  pna_gpu_create_solid_archive_host(pna_gpu_ctx *ctx, int algo, int level, size_t n, const char *const *names,
                                       const void *const *src, const size_t *src_len, pna_sink_fn sink, void *user);
/* The same with a cipher, streaming too: the layouts of pna_gpu_create_solid_archive_enc_device (CTR: cipher->ivs ONE 16-byte IV; GCM: ONE
 * salt(32) || nonce_prefix(7); NULL: drawn from the OS), and for the same IV / salt the same bytes, at every solid_win_mib, with inner entries of ANY
 * size.  CTR: the keystream continues from window to window at the stream offset of the window's first compressed byte.  GCM STREAM: the segments are
 * cut from the whole compressed stream (GcmEncryptWriter, lib/src/cipher/gcm.rs:45-90) -- each window but the last holds back, in device memory, the
 * 1 .. gcm_segment_size bytes of its output not yet known to form a non-final segment and puts them in front of the next window's output.  Page-locked
 * memory (pna_gpu_debug_pinned_bytes): about four windows, plus two GCM segments (the output slots hold the carry); device memory: one segment of carry
 * on top of the plain form.  cipher == NULL or PNA_ENC_NONE: pna_gpu_create_solid_archive_host.  CBC: PNA_E_UNSUPPORTED; Camellia: PNA_E_UNSUPPORTED unless option "camellia" = 1 (then CTR and GCM, like AES). */
int  pna_gpu_create_solid_archive_enc_host(pna_gpu_ctx *ctx, int algo, int level, size_t n, const char *const *names,
                                           const void *const *src, const size_t *src_len, const pna_gpu_cipher *cipher,
                                           pna_sink_fn sink, void *user);

/* Same archive from host memory with a bounded in-flight window: entries stream through two page-locked staging slots
 * (<= ~1 GiB of input each); staging of sub-batch k+1, the H2D copy, the kernels of sub-batch k and the D2H copy of
 * sub-batch k-1 overlap.  The sink receives the signature + AHED, then one piece per sub-batch, then AEND.  Replaces the
 * reference's fan-out that keeps every compressed entry in RAM until the rayon scope ends
 * (cli/src/command/core.rs:496-537, cli/src/command/create.rs:575-635).  pna_create_archive() uses it for non-solid
 * zstd / deflate archives. */
int  pna_gpu_create_archive_host(pna_gpu_ctx *ctx, int algo, int level, size_t n, const char *const *names,
                                 const void *const *src, const size_t *src_len, pna_sink_fn sink, void *user);

/* ---- read side (extract / verify): replaces decompress_reader() -> zstd::stream::read::Decoder / flate2::read::ZlibDecoder
 * (lib/src/entry/read.rs:171-190; callers cli/src/command/extract.rs:594-640, verify.rs:140-188).  Entry i's payload (the
 * concatenated FDAT bodies) is decoded to raw_len[i] bytes (the entry's fSIZ).
 *   PNA_ALGO_ZSTD: one or more RFC 8878 frames without dictionary, offsets up to 2^28 - 4 (windows up to 128 MiB: every libzstd level without --long); a multi-frame payload must follow this library's
 *     segmentation (every frame but the last holds 1 MiB) because frames carry no content size -- single-frame payloads, which
 *     is what the reference writes, always work.
 *   PNA_ALGO_DEFLATE: one RFC 1950 zlib stream (any block types, sync-flush markers, window <= 32 KiB); Adler-32 is verified.
 *     Streams of 4 GiB and more (compressed or decoded) are decoded by their sync-flush delimited pieces -- what this library
 *     writes --, or, a foreign encoder's stream without such markers (one flate2 / zlib stream per entry: what the reference writes), in chunks between
 *     block starts found by trial -- dynamic and stored blocks; compressed positions are 64-bit, so the compressed size is not limited --; what
 *     fits neither (a stream of 4 GiB and more whose only block boundaries are fixed-Huffman blocks) is PNA_E_UNSUPPORTED (the wave-per-stream
 *     walk counts in 32 bits).
 *   Single streams of any size are executed in parallel (zstd frames of 2 GiB and more since the second half of round 4: the executor's windows,
 *     option "zexec_win_mib"), whatever their compressed size and however many literals they carry (the header walk and the literal scratch count in
 *     64 bits); a zstd frame that does not fit its pooled resources -- more than 2^31 - 1 sequences, more blocks or table sets than its content's
 *     size plans for -- is left to one workgroup (~11 MiB/s) unless the option "zdec_fallback_max_mib" refuses it.
 *   PNA_ALGO_XZ: ONE .xz stream (xz file format 1.0.4: stream header, blocks, Index, stream footer), as liblzma's XzEncoder::new(writer, level) writes it.
 *     Container: magic, stream flags (equal in header and footer), backward size, the Index and every block header are validated with their CRC32s; the
 *       Index is found from the end, so bytes behind the footer -- stream padding, a second stream -- are PNA_E_INVAL (a departure from the reference's
 *       reader, which stops at the first stream's end).
 *     Filters: exactly one, LZMA2 (id 0x21), dictionary-size byte 0 .. 40; Delta, BCJ and every other chain: PNA_E_UNSUPPORTED.
 *     Checks: None, CRC32 and CRC64 (liblzma's default) are verified on the device per block; SHA-256 and the unassigned types: PNA_E_UNSUPPORTED.
 *     Blocks are located from the Index (unpadded size and uncompressed size per record), so each decodes on its own, one wave per block, whether or
 *       not its header carries the optional size fields -- where it does they must agree with the Index.  A block of 4 GiB or more of decoded bytes is
 *       PNA_E_UNSUPPORTED; a stream of many blocks may be of any size.  raw_len[i] must be the sum of the Index records.
 *     LZMA2: every chunk kind -- 0x00 end, 0x01 / 0x02 uncompressed, 0x80 .. 0xFF LZMA with the four reset levels --, every lc / lp / pb with
 *       lc + lp <= 4.  Corrupt (PNA_E_INVAL): control bytes 0x03 .. 0x7F, a first chunk that does not reset the dictionary, a first LZMA chunk without
 *       properties, a match distance beyond min(dictionary size, bytes produced since the dictionary reset), an end-of-payload marker, a chunk or
 *       block that ends early or late or leaves compressed bytes unused, a range coder that does not start with a zero byte or end at zero.
 *     A single block is a serial chain on one wave (measured: 1.8 - 2.8 MiB/s per block, profiles/xz_rate.txt); the gain is entries and blocks side by side.
 *     (Streams this library writes -- XZ ON THE WRITE SIDE -- carry one block per MiB, so they are read in parallel.)
 * Errors: PNA_E_INVAL for corrupt / mismatching streams (pna_gpu_last_error names the entry), PNA_E_UNSUPPORTED for
 * dictionaries and other algorithms.
 *
 * PLACEMENT (pna_gpu_decompress_batch_device; the open decoders and pna_gpu_open_size_device below follow the same rules).  d_src and d_dst may be any device
 * addresses, aligned or not: only d_src + src_off[i] and d_dst + dst_off[i] matter (the entry points fold a base's low four bits into the offsets).  src_off[i] and dst_off[i] may be ANY byte offsets: no alignment, no padding, no order is asked for.
 * Stream i is the bytes [src_off[i], src_off[i] + src_len[i]) of d_src, its room the bytes [dst_off[i], dst_off[i] + raw_len[i]) of d_dst (an open decoder's:
 * dst_cap bytes).  Streams may touch; rooms may touch and may come in any order, but must not overlap each other or the
 * streams.  Nothing outside the rooms is written, whether the call succeeds or fails: not the bytes in front of a room that share an aligned word with its
 * first byte, not the bytes behind it.  After a failed call the rooms' contents are unspecified; after an open decoder's success so are the bytes of its room
 * behind the size it reports.  d_src is never written.  Reads: the decoders read outside a stream's own bytes, and ignore what they find there -- the
 * aligned 4-byte words (of d_src) that hold a stream's first and last byte (zlib), and up to 15 bytes behind a stream's end (zstd: the backward bit readers
 * open with two 8-byte loads from the first byte of a bit stream, which may be the last byte of a frame).  So the 15 bytes behind the end of the LAST stream
 * in d_src must be readable memory of any content; nothing in front of the 16-byte group that holds the first stream's first byte is read.  (pna_gpu_decompress_batch stages its payloads at 16-byte strides
 * with 64 bytes behind the last: more than is needed.) */
int  pna_gpu_decompress_batch(pna_gpu_ctx *ctx, int algo, size_t n, const void *const *src, const size_t *src_len,
                              void *const *dst, const size_t *raw_len);
int  pna_gpu_decompress_batch_device(pna_gpu_ctx *ctx, int algo, size_t n, const void *d_src, const uint64_t *src_off,
                                     const uint64_t *src_len, void *d_dst, const uint64_t *dst_off, const uint64_t *raw_len,
                                     void *hip_stream);

/* A zstd stream whose decoded size is recorded nowhere (the SDAT stream of a solid entry).  Step 1 counts its frames; the caller
 * provides frames x 1 MiB of room (this library's segmentation) -- for ONE frame, as the reference writes it, any capacity it sees fit;
 * step 2 decodes and reports the size found (PNA_E_INVAL when the stream does not fit).  src_off and dst_off of the open decoders and of
 * pna_gpu_open_size_device: any byte offsets, the room [dst_off, dst_off + dst_cap) alone is written, 15 readable bytes behind the stream -- PLACEMENT at
 * pna_gpu_decompress_batch_device. */
int  pna_gpu_zstd_stream_frames_device(pna_gpu_ctx *ctx, const void *d_src, uint64_t src_off, uint64_t src_len, uint32_t *n_frames, void *hip_stream);
int  pna_gpu_zstd_decompress_open_device(pna_gpu_ctx *ctx, const void *d_src, uint64_t src_off, uint64_t src_len, void *d_dst, uint64_t dst_off,
                                         uint64_t dst_cap, uint64_t *raw_len, void *hip_stream);

/* The same for one zlib stream (deflate entries without fSIZ, deflate solid streams). */
int  pna_gpu_inflate_open_device(pna_gpu_ctx *ctx, const void *d_src, uint64_t src_off, uint64_t src_len, void *d_dst, uint64_t dst_off,
                                 uint64_t dst_cap, uint64_t *raw_len, void *hip_stream);

/* The same for one .xz stream (xz entries without fSIZ, xz solid streams): its size is the sum of its Index records. */
int  pna_gpu_xz_decompress_open_device(pna_gpu_ctx *ctx, const void *d_src, uint64_t src_off, uint64_t src_len, void *d_dst, uint64_t dst_off,
                                       uint64_t dst_cap, uint64_t *raw_len, void *hip_stream);

/* The decoded size of one such stream (algo: PNA_ALGO_ZSTD, PNA_ALGO_DEFLATE, PNA_ALGO_XZ or PNA_ALGO_STORE), measured on the device before it is decoded, so that
 * the open decoders above can be given exactly the room it needs.  No output buffer is used; the scratch grows with src_len, not with the size.
 * GUARANTEE: *size is never below what the stream decodes to.  *exact = 1: *size IS that size -- always for xz streams (the sum of the Index records,
 * after the whole container walk; nothing is decoded), always for zlib streams (their blocks are walked and
 * counted: k_inflate's count pass, one wave per chunk between block starts) and for zstd frames that carry Frame_Content_Size (this library's);
 * *exact = 0: an upper bound -- a zstd frame without a content size (what the reference's solid writer emits) counts its raw and RLE blocks exactly and
 * each compressed block as Block_Maximum_Size (min(window, 128 KiB)).  The open decoders report the true size.  PNA_E_INVAL for bytes that are not a
 * well-formed stream (truncated, reserved block types, a content size its blocks contradict, a corrupt zlib block); reads as stated under PLACEMENT at
 * pna_gpu_decompress_batch_device (measuring reads the headers only: no read leaves the stream's bytes; zlib: its aligned 4-byte words); src_off is any byte offset
 * and the result does not depend on it.  PNA_E_UNSUPPORTED: zlib streams of 4 GiB of compressed bytes and more, or of more than 4 GiB of content, that have no dynamic or
 * stored blocks to split them at (fixed-Huffman blocks only). */
int  pna_gpu_open_size_device(pna_gpu_ctx *ctx, int algo, const void *d_src, uint64_t src_off, uint64_t src_len, uint64_t *size, int *exact, void *hip_stream);

/* Read-side driver for archives in host memory (normal and solid entries): `pna extract` (verify: pna_gpu_verify_archive_host below) (cli/src/command/extract.rs:594-640,
 * verify.rs:140-188; Archive::read_header + entries, lib/src/archive/read.rs:22-66; read_chunk's mandatory CRC check, lib/src/io.rs:117-149;
 * decrypt_reader / decompress_reader, lib/src/entry/read.rs:59-104,171-190).  The chunk walk and the small chunks' CRCs are host work;
 * the FDAT CRC-32s, the gather of every entry's data pieces, AES decryption -- CTR, CBC (PKCS#7 checked), GCM STREAM (key confirmation,
 * every segment tag verified) -- with the key derived from the PHSF string ("$argon2{d,i,id}$..." or "$pbkdf2-sha256$...") and `password`,
 * and zstd / deflate / xz / store decoding run on the device; entries without fSIZ are sized by the decoder.  cb is called once per entry in archive order (kind =
 * DataKind::to_byte(): 0 file, 1 directory, ...); `data` is valid during the call.  PNA_E_INVAL: structural damage, CRC mismatch, corrupt
 * stream, wrong password (GCM key confirmation, CBC padding), authentication failure; PNA_E_UNSUPPORTED: multipart archives,
 * Camellia unless option "camellia" = 1 (then decrypted like AES, in the same windows), xz streams outside the scope stated at pna_gpu_decompress_batch, solid streams with inner entries that are not stored.  Solid entries (SHED [PHSF] SDAT* SEND; plain or AES CTR / CBC / GCM):
 * SDAT CRCs and the inner FDAT CRCs on the device.  A solid stream or an entry without fSIZ has no recorded size: it is measured first
 * (pna_gpu_open_size_device), decoded into device memory of that size and copied once to host memory (an N-GiB solid stream: N GiB of host memory,
 * besides the archive); PNA_E_NOMEM, naming the size, when the device cannot hold it. */
/* `name` is the entry's PATH as the reference's reader exposes it (EntryHeader::path(), lib/src/entry/header.rs:91-94): the FHED name
 * normalised and reduced to its normal components (EntryName::sanitize, lib/src/entry/name.rs:148-156 -- no root, no "." / ".."), so a
 * callback that writes files below an output directory cannot be led outside it by a crafted archive.  FHED names that are not valid
 * UTF-8 (InvalidData in the reference, header.rs:143-146) or that contain a NUL byte (not representable here) fail with PNA_E_INVAL. */
typedef int (*pna_entry_fn)(void *user, size_t index, const char *name, int kind, const void *data, size_t len);
int  pna_gpu_extract_archive_host(pna_gpu_ctx *ctx, const void *archive, size_t archive_len, const void *password, size_t password_len,
                                  pna_entry_fn cb, void *user);

/* `pna experimental verify` (cli/src/command/verify.rs verify_archive): every entry checked, one verdict per entry, the walk goes on after damage.
 * The read-side driver above in verdict mode: the same chunk walk, windows, CRC-32, AES and decoding kernels, but a failure marks the entries it
 * concerns instead of ending the call -- per-chunk CRC verdicts, per-segment GCM tag verdicts and CBC padding verdicts are folded on the device
 * (k_verdict) into one status word per entry, and the decoders report a status per stream.  No decoded byte of a normal entry goes to the host (a
 * solid stream is still decoded into host memory, as extract does, to walk its inner entries).
 *   parts / part_len / n_parts: the archive, or the parts of a split archive in order (what pna_join_parts takes), read in place; an entry may span parts.
 *   vflags: PNA_VERIFY_FAST = chunk structure and CRC-32 only (no key derivation, no decryption, no decoding; every intact entry is OK, encrypted ones too).
 *   cb: one record per entry in archive order.  Solid blocks: one record per inner entry in deep mode; one record for the whole block (kind
 *     PNA_VERIFY_KIND_SOLID) in fast mode, when it is encrypted and no password is given, or when it fails -- unlike the reference, which counts the
 *     inner entries it read before the failure as ok.  `name` is the sanitised path extract hands out; NULL when the FHED is unreadable (a bad CRC, not
 *     UTF-8).  A chunk that fails its CRC is consumed (its length field trusted, as io::read_chunk does) and the walk resumes behind it; a bad FHED makes
 *     the chunks up to the next FEND / SEND one PNA_VERIFY_KIND_BROKEN record.  Each broken entry is its own record (the reference merges neighbouring
 *     failures into one).  A wrong fSIZ is PNA_VERIFY_SIZE_HINT on an OK record: a stream that fails against its fSIZ is decoded once more without it.
 *   Without a password, encrypted entries are PNA_VERIFY_SKIPPED; with one, every PHSF string is derived once per call.
 * Returns PNA_OK when the walk reached AEND, even when entries failed (summary->failed says so); PNA_E_INVAL with summary->broken = 1 when it could
 * not go on (a truncated chunk, no AEND, a part missing) -- every entry before the break has its record; HIP, allocation and callback errors
 * (PNA_E_SINK) as usual.  A zlib stream of 4 GiB and more that cannot be split into chunks still fails the call, as in extract. */
#define PNA_VERIFY_FAST            1u   /* chunk structure + CRC-32 only: no key derivation, no decryption, no decoding */
/* status of one record */
#define PNA_VERIFY_OK              0
#define PNA_VERIFY_SKIPPED         1    /* encrypted, no password given */
#define PNA_VERIFY_BAD_CRC         2    /* a chunk of the entry failed its CRC-32 */
#define PNA_VERIFY_BAD_STRUCTURE   3    /* bad header chunk, unknown critical chunk, entry without FHED, ... */
#define PNA_VERIFY_BAD_AUTH        4    /* GCM: key confirmation or a segment tag */
#define PNA_VERIFY_BAD_DECRYPT     5    /* CBC length / PKCS#7 padding */
#define PNA_VERIFY_BAD_STREAM      6    /* corrupt zstd / zlib stream, content checksum, Adler-32 */
#define PNA_VERIFY_UNSUPPORTED     7    /* Camellia unless option "camellia" = 1, an xz stream with a SHA-256 check or a filter chain, ...: what this build does not decode */
/* flags of one record */
#define PNA_VERIFY_SIZE_HINT       1u   /* fSIZ present and != the decoded size (a warning; status stays OK) */
#define PNA_VERIFY_UNAUTHENTICATED 2u   /* AES / Camellia CBC / CTR: a wrong password cannot be told from damage (verify.rs is_unauthenticated) */
#define PNA_VERIFY_KIND_SOLID  (-1)     /* record of a whole solid block (fast mode, skipped, or failed) */
#define PNA_VERIFY_KIND_BROKEN (-2)     /* chunks that belong to no readable entry header */
typedef struct { uint64_t total, ok, failed, skipped, unsupported; uint32_t unauthenticated_failure, broken; } pna_verify_summary;
typedef int (*pna_verify_fn)(void *user, size_t index, const char *name /* NULL if unknown */, int kind, int status,
                             uint32_t flags, uint64_t size /* decoded bytes; 0 in fast mode */, const char *detail);
int  pna_gpu_verify_archive_host(pna_gpu_ctx *ctx, const void *const *parts, const size_t *part_len, size_t n_parts,
                                 const void *password, size_t password_len, uint32_t vflags,
                                 pna_verify_fn cb, void *user, pna_verify_summary *summary);

/* `pna experimental diff` (cli/src/command/diff.rs diff_archive -> compare_entry -> streams_equal(fs_file, entry.reader())): is the archive still
 * equal to the files, and if not, which entries differ and from which byte.  The verify driver above with a second input: for every entry the host
 * is asked for the filesystem side (`source`), the files' bytes are copied to the device next to the decoded entries -- through two page-locked
 * slots of option "diff_slot_mib" [PNA_DIFF_SLOT_MIB] (default 256) MiB each and two device slots of that size, on a stream of their own, a file
 * larger than a slot in pieces -- and k_diff finds the first differing byte of every entry.  No decoded byte of a normal entry goes to the host; a solid
 * stream is copied to the host once to walk its inner headers (as verify does) and its inner entries are compared on the device where the stream lies.
 *   source: called once per entry that has a readable name, in archive order, before the entry is decrypted or decoded; it fills *out: fs_kind, and
 *     for PNA_DIFF_FS_FILE the file's bytes, for PNA_DIFF_FS_SYMLINK the link's target bytes.  `data` must stay valid until that entry's record
 *     callback has been called, and not longer (a host may mmap per entry and munmap in the record callback).  Bytes that lie in a buffer of
 *     pna_gpu_host_alloc are copied from there without staging.  stored_size is the entry's fSIZ, UINT64_MAX if it has none.  PNA_DIFF_FS_IGNORE is
 *     the host's filter: the entry is not compared.  A non-zero return ends the call with PNA_E_SINK.
 *   cb: one record per entry in archive order; index / name / kind as in verify (PNA_VERIFY_KIND_SOLID for a solid block that is skipped or fails,
 *     PNA_VERIFY_KIND_BROKEN for chunks of no readable header; name NULL where verify's is).  status, following compare_entry (diff.rs:336-421):
 *       SAME; MISSING; TYPE_MISMATCH (entry kind against fs_kind); SIZE_DIFFERS -- fSIZ present and != len, decided before anything of the entry is
 *       decrypted or decoded (diff.rs:361-365); CONTENTS_DIFFER -- every other difference of a file's content, a stream without fSIZ (or whose fSIZ
 *       equals len) that decodes to another length included; SYMLINK_DIFFERS; NOT_COMPARED (PNA_DIFF_FS_IGNORE, directories, hard links, other
 *       kinds); SKIPPED (encrypted, no password); DAMAGED -- a compared entry that fails a check: verify_status is the PNA_VERIFY_* status verify
 *       gives that entry and flags carries PNA_VERIFY_UNAUTHENTICATED where verify sets it.  MISSING, TYPE_MISMATCH, SIZE_DIFFERS and NOT_COMPARED
 *       entries are not gathered, decrypted or decoded; their chunks' CRCs are still checked and the finding is their verify_status (0 = none).
 *     first_diff: CONTENTS_DIFFER / SYMLINK_DIFFERS -- the offset of the first byte that differs; where one side is a strict prefix of the other, the
 *       shorter length.  UINT64_MAX otherwise.  (The reference does not report it.)  size: the entry's decoded bytes where it was decoded, else 0.
 *     link_target: hard-link entries whose path is a file on the host (PNA_DIFF_FS_FILE) are NOT_COMPARED and their decoded target (at most 64 KiB)
 *       is handed out here, NUL-terminated -- whether two paths are the same file is the host's question (is_same_file).  NULL otherwise.
 *   Mode, mtime, uid / gid and the other metadata chunks stay with the host (compare_file_metadata: metadata interpretation is not this library's).
 * The walk goes on after damage; return codes, summary->broken and the callback-error rule (PNA_E_SINK) as in verify.  PNA_E_UNSUPPORTED in a build
 * without k_diff.  Page-locked memory: the two slots (pna_gpu_debug_pinned_bytes shows them), whatever the archive's size. */
#define PNA_DIFF_FS_MISSING   0
#define PNA_DIFF_FS_FILE      1
#define PNA_DIFF_FS_DIR       2
#define PNA_DIFF_FS_SYMLINK   3    /* data = the link's target bytes */
#define PNA_DIFF_FS_OTHER     4
#define PNA_DIFF_FS_IGNORE    5    /* the host's filter: entry not compared */
#define PNA_DIFF_SAME             0
#define PNA_DIFF_MISSING          1
#define PNA_DIFF_TYPE_MISMATCH    2
#define PNA_DIFF_SIZE_DIFFERS     3
#define PNA_DIFF_CONTENTS_DIFFER  4
#define PNA_DIFF_SYMLINK_DIFFERS  5
#define PNA_DIFF_NOT_COMPARED     6
#define PNA_DIFF_SKIPPED          7
#define PNA_DIFF_DAMAGED          8
typedef struct { int fs_kind; const void *data; uint64_t len; } pna_diff_file;
typedef struct { uint64_t total, same, differ /* missing + type + size + contents + symlink */, not_compared, skipped, damaged; uint32_t broken, pad; } pna_diff_summary;
typedef int (*pna_diff_source_fn)(void *user, size_t index, const char *name, int kind, uint64_t stored_size /* fSIZ, UINT64_MAX if none */,
                                  pna_diff_file *out);
typedef int (*pna_diff_fn)(void *user, size_t index, const char *name /* NULL if unknown */, int kind, int status, int verify_status, uint32_t flags,
                           uint64_t size, uint64_t first_diff, const char *link_target);
int  pna_gpu_diff_archive_host(pna_gpu_ctx *ctx, const void *const *parts, const size_t *part_len, size_t n_parts,
                               const void *password, size_t password_len, pna_diff_source_fn source, pna_diff_fn cb, void *user,
                               pna_diff_summary *summary);
/* The latest pna_gpu_diff_archive_host call of the context: streams handed to the decoders, bytes k_diff compared, its HIP-event time (any pointer may
 * be NULL).  Tests pin "SIZE_DIFFERS costs no decode" with it; not on any product path. */
int  pna_gpu_debug_diff_stats(pna_gpu_ctx *ctx, uint64_t *decoded_streams, uint64_t *compared_bytes, double *ms_k_diff);

/* `pna extract archive.pna path...` (cli/src/command/extract.rs:1038-1121 filter_entry: a reader is built for the kept entries only): extract for the
 * entries the host chooses, each to host memory or to device memory of the caller's.  The extract driver's stages and failure semantics over windows
 * that hold the selected entries only; parts / part_len / n_parts as in pna_gpu_verify_archive_host (a split archive is read in place).
 *   select: called once per entry, in archive order, before anything of that entry is uploaded; index, name (the sanitised path; a name that is not
 *     UTF-8 or holds a NUL fails the call with PNA_E_INVAL) and kind are what pna_entry_fn gets, stored_size is the entry's fSIZ (UINT64_MAX if it
 *     has none).  It fills *out: PNA_EXTRACT_SKIP (the preset), PNA_EXTRACT_HOST, or PNA_EXTRACT_DEVICE with d_dst / cap.  A non-zero return ends the
 *     call with PNA_E_SINK; `where` outside 0..2, or PNA_EXTRACT_DEVICE with d_dst NULL and cap > 0, with PNA_E_INVAL.
 *   cb: one record per SELECTED entry, in archive order (entries without data -- directories ... -- with len 0).  HOST: `data` are the decoded bytes in
 *     host memory, valid during the call.  DEVICE: the decoded bytes have been written to d_dst[0 .. len) -- byte-exactly, nothing of the entry went to
 *     the host -- and `data` is d_dst; a window's records follow its kernels, so the callback may use d_dst.  cap < the decoded size:
 *     PNA_EXTRACT_TOO_SMALL, nothing written, data NULL, len = the size needed (for an entry without fSIZ the size the decoder found).
 *   Structural damage, a bad CRC, a corrupt stream, a wrong password or an authentication failure on a selected entry: PNA_E_INVAL, as in extract.  The
 *   small chunks the host walks (FHED, fSIZ, PHSF, FEND ...) are CRC-checked for every entry.  The data chunks (FDAT) of entries that are NOT selected are
 *   neither uploaded nor checked -- a deliberate departure from the reference, whose io::read_chunk checks every chunk it passes: taking one file out of
 *   a large archive must not cost the whole archive over the host link.  PNA_EXTRACT_CHECK_ALL restores the reference's behaviour: those chunks are
 *   uploaded and CRC-checked, but not gathered or decoded (as pna_gpu_diff_archive_host treats NOT_COMPARED entries).
 *   Upload: a window's H2D copies are the records (FHED .. FEND) of its selected entries; records at most PNA_EXTRACT_GAP_MAX bytes apart travel as one
 *   copy (pna_extract_plan_runs).  Windows are cut by the bytes uploaded ("extract_win_mib"), not by the archive span they reach over.
 *   Keys: a PHSF string is derived only when a selected stream needs it, once per call.
 *   Solid blocks: a block is one stream -- uploaded, decrypted (an encrypted block without a password fails the call, as in extract) and decoded whole,
 *   even when nothing turns out to be wanted from it: the inner entries' names lie in the decoded stream.  It is copied to the host once for its header
 *   walk, as extract / verify / diff do; `select` is then asked for every inner entry, HOST records point into that copy, DEVICE records are copied on the
 *   device from the decoded stream where it lies.
 * PNA_E_UNSUPPORTED in a build without k_pick (and for what extract does not decode). */
#define PNA_EXTRACT_SKIP    0   /* not wanted: no record, nothing of the entry gathered, decrypted or decoded */
#define PNA_EXTRACT_HOST    1   /* decoded bytes handed out in host memory during the record callback (what extract does today) */
#define PNA_EXTRACT_DEVICE  2   /* decoded bytes written to d_dst[0 .. len), cap bytes available there */
typedef struct { int where; void *d_dst; uint64_t cap; } pna_extract_dest;
typedef int (*pna_extract_select_fn)(void *user, size_t index, const char *name, int kind,
                                     uint64_t stored_size /* fSIZ, UINT64_MAX if none */, pna_extract_dest *out);
#define PNA_EXTRACT_OK         0
#define PNA_EXTRACT_TOO_SMALL  1   /* DEVICE: cap < decoded size; nothing written, len = the size needed */
typedef int (*pna_extract_record_fn)(void *user, size_t index, const char *name, int kind, int status,
                                     const void *data /* HOST: host bytes, valid during the call; DEVICE: d_dst; NULL when TOO_SMALL */,
                                     uint64_t len);
/* total: entries `select` was asked about; selected = to_host + to_device + too_small */
typedef struct { uint64_t total, selected, to_host, to_device, too_small; } pna_extract_summary;
#define PNA_EXTRACT_CHECK_ALL  1u  /* xflags: also upload and CRC-check the FDAT / SDAT chunks of entries that are not selected */
int  pna_gpu_extract_select_host(pna_gpu_ctx *ctx, const void *const *parts, const size_t *part_len, size_t n_parts,
                                 const void *password, size_t password_len, uint32_t xflags,
                                 pna_extract_select_fn select, pna_extract_record_fn cb, void *user,
                                 pna_extract_summary *summary);
/* The upload plan of a window (host code, no device): records [rec_off[i], rec_off[i] + rec_len[i]) in archive order, none inside another; the wanted
 * ones (wanted[i] != 0, rec_len[i] > 0) become runs, two wanted records whose gap is at most gap_max bytes sharing one -- the gap's bytes travel with
 * them.  run_off / run_len (room for n each; either may be NULL) and *n_runs receive the runs.  PNA_E_INVAL for null arguments or records out of order.
 * PNA_EXTRACT_GAP_MAX is the driver's gap_max: a host-to-device copy costs some 10 us before its first byte moves, the time in which the link carries
 * several hundred KiB, so a gap of 64 KiB is always cheaper to send than to cut at, and what it wastes stays small against the records around it. */
#define PNA_EXTRACT_GAP_MAX  65536u
int  pna_extract_plan_runs(const uint64_t *rec_off, const uint64_t *rec_len, const uint8_t *wanted, size_t n,
                           uint64_t gap_max, uint64_t *run_off, uint64_t *run_len, size_t *n_runs);
/* KEY DERIVATION ON THE DEVICE.  An encrypted entry's key is the password hash its PHSF chunk names: Argon2 (RFC 9106, version 0x13; the reference's
 * default is argon2id m=19456,t=2,p=1) or PBKDF2-HMAC-SHA256 (600 000 rounds), 32 bytes.  pna_gpu_kdf_batch derives n keys from ONE password and n salts /
 * parameter sets, all in host memory: Argon2's block fill and PBKDF2's chain run on the device (k_kdf.hip: one Argon2 lane per 32 wave lanes, one PBKDF2
 * job per wave lane), H0, the seed blocks, the final H' and HMAC's key set-up on the host.  keys receives n x 32 bytes.
 *   The device takes: Argon2 with lanes <= 16, t_cost <= 64, 8 lanes <= m_cost_kib <= 2^20, whose blocks fit the block memory (option "kdf_mem_mib"); PBKDF2
 *   with any rounds >= 1; password_len <= 1024, salt_len <= 64.  Any other job of the batch is derived by pna_kdf_argon2 / pna_kdf_pbkdf2_sha256 in the same
 *   call.  kind: PNA_KDF_ARGON2D / PNA_KDF_ARGON2I / PNA_KDF_ARGON2ID_JOB (t_cost, m_cost_kib, lanes; rounds ignored) or PNA_KDF_PBKDF2_SHA256_JOB (rounds; the others ignored).
 *   status (n ints, may be NULL): PNA_OK, or the code with which the host function refuses the job's parameters (PNA_E_INVAL: m < 8 lanes, t = 0, rounds = 0,
 *   an unknown kind, ...) -- the other jobs still run and the call returns PNA_OK.  With status == NULL the first such job fails the call.
 *   Drains hip_stream (NULL: the context's).  Keys are byte-equal to the host functions' whatever path a job took.
 * pna_phsf_parse (host code, no device): a PHSF string -- "$argon2id$v=19$m=<KiB>,t=<passes>,p=<lanes>$<salt>" (argon2d / argon2i alike, "v=19$" optional,
 * absent parameters at the argon2 crate's defaults 19456 / 2 / 1) or "$pbkdf2-sha256$i=<rounds>,l=<len>$<salt>" (600 000) -- as a job.  The salt's bytes
 * (B64 without padding, what follows it from the next '$' on ignored) go to salt_buf, *salt_len receives their number and job->salt / salt_len name them.
 * PNA_E_INVAL: malformed; PNA_E_UNSUPPORTED: another hash, an Argon2 version other than 0x13, or a cost beyond what the read side accepts from an archive
 * (m <= 4 GiB, t <= 64, p <= 256, rounds <= 10 000 000); PNA_E_DSTSIZE: salt_cap too small.
 * pna_gpu_debug_kdf_stats: the context's latest pna_gpu_kdf_batch (any pointer may be NULL) -- jobs the kernels derived, jobs the host functions derived,
 * rounds of the block memory (0: no Argon2 job on the device), HIP-event time of the kernels.  After a driver call under "kdf_device" that had a key to
 * derive: the sums over that call's batches, one per window at most -- all zero when every window stayed below the threshold and the keys came from the host
 * one by one.  Not on any product path. */
#define PNA_KDF_ARGON2D           0
#define PNA_KDF_ARGON2I           1
#define PNA_KDF_ARGON2ID_JOB      2   /* (pna_archive.h's PNA_KDF_ARGON2ID = 0 names a choice of pna_kdf_derive, as PNA_KDF_PBKDF2_SHA256 does) */
#define PNA_KDF_PBKDF2_SHA256_JOB 3
typedef struct { int kind; uint32_t t_cost, m_cost_kib, lanes, rounds; const void *salt; size_t salt_len; } pna_kdf_job;
int  pna_gpu_kdf_batch(pna_gpu_ctx *ctx, const void *password, size_t password_len, size_t n, const pna_kdf_job *jobs,
                       uint8_t *keys, int *status, void *hip_stream);
int  pna_phsf_parse(const char *phsf, size_t len, pna_kdf_job *job, uint8_t *salt_buf, size_t salt_cap, size_t *salt_len);
int  pna_gpu_debug_kdf_stats(pna_gpu_ctx *ctx, uint64_t *device_jobs, uint64_t *host_jobs, uint64_t *rounds, double *ms_kernels);
/* The latest pna_gpu_extract_select_host call of the context (any pointer may be NULL): bytes of its H2D archive copies; streams taken through the decode
 * stage (every selected entry that has data -- a stored one's decode is the identity -- and every solid stream); key derivations; bytes k_pick moved and
 * its HIP-event time.  Not on any product path. */
int  pna_gpu_debug_extract_stats(pna_gpu_ctx *ctx, uint64_t *uploaded_bytes, uint64_t *decoded_streams,
                                 uint64_t *kdf_runs, uint64_t *picked_bytes, double *ms_k_pick);
/* k_pick alone, for its test: n ranges d_src[src_off[i] .. +len[i]) -> d_dst[i][0 .. len[i]) (src_off, d_dst, len: host arrays).  The 16-byte groups
 * of d_src that hold a range's first and last byte must be readable.  Drains hip_stream (NULL: the context's); picked_bytes and ms_k_pick of
 * pna_gpu_debug_extract_stats then hold this call's. */
int  pna_gpu_debug_pick_device(pna_gpu_ctx *ctx, size_t n, const void *d_src, const uint64_t *src_off,
                               void *const *d_dst, const uint64_t *len, void *hip_stream);

/* pna_gpu_create_archive_host for ONE PART of an archive (PNA_PART_HEAD: signature + AHED first, PNA_PART_TAIL: AEND last): what
 * `pna append` writes behind the existing entries (PNA_PART_TAIL only) and `pna update` for the entries it re-creates (neither flag). */
int  pna_gpu_create_archive_part_host(pna_gpu_ctx *ctx, int algo, int level, size_t n, const char *const *names,
                                      const void *const *src, const size_t *src_len, uint32_t part_flags, pna_sink_fn sink, void *user);
/* One process driving several GPUs (SURVEY 8(b) `device_ids, n_devices`): n_ctx contexts (pna_gpu_init per device; they may share a
 * device), the entries cut into contiguous index ranges balanced by bytes, one range per context on a thread of its own through the bounded
 * host pipeline, the parts handed to the sink in index order -- the reference's fan-out + ordered drain (cli/src/command/core.rs:496-537,
 * 471-493) with devices in place of worker threads; no device-to-device traffic.  The archive equals pna_gpu_create_archive_host's (every range runs with
 * the block size of the whole call's input bytes). */
int  pna_gpu_create_archive_multi_host(pna_gpu_ctx *const *ctxs, size_t n_ctx, int algo, int level, size_t n, const char *const *names,
                                       const void *const *src, const size_t *src_len, pna_sink_fn sink, void *user);
/* Zero-staging input.  The reference reads every file into memory of its own (fs::read, cli/src/command/core.rs:889-913 write_from_path) before the
 * encoder sees it; a device needs the bytes in PAGE-LOCKED memory to copy them at the link's rate.  pna_gpu_host_alloc hands the host such a buffer to
 * read its files into (read_exact into the slot instead of fs::read into a Vec): the host-memory create entry points (pna_gpu_create_archive_host and its
 * _enc / _meta / _chunked / _part forms, pna_gpu_append_archive_host) send a batch whose entries all lie in buffers of this call to the device straight
 * from there -- no pageable -> page-locked copy, one host thread instead of eight --; runs of entries that are contiguous at a 16-byte stride travel as
 * one copy.  A batch with an entry elsewhere is staged as before.  A buffer must stay untouched until the create call that reads it has returned;
 * pna_gpu_host_free gives it back (pna_gpu_destroy frees what is left). */
int  pna_gpu_host_alloc(pna_gpu_ctx *ctx, size_t bytes, void **out);
int  pna_gpu_host_free(pna_gpu_ctx *ctx, void *buf);

/* `pna append` (cli/src/command/append.rs:504-560 run_append_archive: open_archive_then_seek_to_end, add the new entries in order,
 * finalize): `archive` is the existing image (or its last part); *write_at receives the offset of its AEND chunk, and the sink receives
 * the bytes that belong there -- the n new entries, compressed on the device, then AEND.  The result, archive[0 .. write_at) followed by
 * the sink's bytes, is the archive `pna create` writes from all entries at once -- the same chunks in the same order; byte for byte where both calls
 * choose the same block size (option `latency_max_mib` = 0 pins it: by default the block size of a call follows the CALL's input bytes, section "levels",
 * so the old entries' payloads are those of the call that made them). */
int  pna_gpu_append_archive_host(pna_gpu_ctx *ctx, int algo, int level, const void *archive, size_t archive_len, size_t n,
                                 const char *const *names, const void *const *src, const size_t *src_len, uint64_t *write_at,
                                 pna_sink_fn sink, void *user);

/* ---- several GPUs, one process per GPU: rank r compresses the contiguous index range r of the entries into an archive PART in its HBM
 * (pna_gpu_create_archive_part_device: PNA_PART_HEAD on the first rank, PNA_PART_TAIL on the last), and the parts in rank order are the archive -- the
 * fan-out and ordered drain of cli/src/command/core.rs:496-537,471-493 with GPUs in place of worker threads.  The one exchange step is the ordered
 * gather: an all-gather of the parts' sizes (8 bytes per rank), then every rank sends its part to `root` (ncclSend / ncclRecv in one group: a link per
 * peer over xGMI), which receives them at the prefix sums of the sizes.  RCCL is loaded with dlopen at the first call (PNA_E_UNSUPPORTED when the
 * host has none).  Bootstrap as with NCCL: rank 0 calls pna_gpu_comm_unique_id and hands the 128 bytes to the other ranks by whatever channel the
 * host has (the reference has none: it is a single process), every rank calls pna_gpu_comm_init.  All calls are collective.
 *   sizes  (host, nranks values, may be NULL) receives every part's length on every rank; *total their sum;
 *   d_out / out_cap matter on `root` only.  The root's capacity travels with the sizes, so the verdict is COLLECTIVE: when the parts do not fit, every
 *   rank returns PNA_E_DSTSIZE and no rank has sent anything (the communicator stays usable; sizes / total are filled in, so the host can retry with
 *   a larger destination).
 * pna_gpu_gather_ordered_start posts the gather and returns: what it waits for is the 16-bytes-per-rank size exchange on the communicator's own
 * stream -- which runs BEHIND the transfers of the gathers posted before it (one stream per communicator: a second start therefore blocks until the first
 * gather is done; the overlap that matters, a gather beside the NEXT piece's compression, comes from calling start after that compression was launched) --;
 * the transfers are ordered behind the work already queued on `hip_stream` (the producer of d_local) and run on the communicator's stream, so
 * they overlap whatever the host launches next (the next piece's compression into another buffer).  pna_gpu_gather_wait blocks until the posted
 * gathers are done; d_local and d_out belong to the gather until then.  pna_gpu_gather_ticket = how many gathers the communicator has posted (the
 * latest one's ticket), pna_gpu_gather_wait_for(ticket) waits for the gathers up to that one only -- the double-buffering host waits for the gather
 * that used a buffer two pieces ago while the latest still travels.  pna_gpu_gather_ordered = start + wait.
 * pna_gather_verdict is the host arithmetic every rank runs on the gathered (size, capacity) pairs (exported: the CPU tests pin it). */
#define PNA_COMM_ID_BYTES 128
typedef struct pna_gpu_comm pna_gpu_comm;
int  pna_gpu_comm_unique_id(void *id128);
int  pna_gpu_comm_init(int device_id, const void *id128, int nranks, int rank, pna_gpu_comm **out);
void pna_gpu_comm_destroy(pna_gpu_comm *comm);
const char *pna_gpu_comm_last_error(const pna_gpu_comm *comm);
int  pna_gpu_gather_ordered(pna_gpu_comm *comm, const void *d_local, uint64_t local_len, int root, void *d_out, uint64_t out_cap,
                            uint64_t *sizes, uint64_t *total, void *hip_stream);
int  pna_gpu_gather_ordered_start(pna_gpu_comm *comm, const void *d_local, uint64_t local_len, int root, void *d_out, uint64_t out_cap,
                                  uint64_t *sizes, uint64_t *total, void *hip_stream);
int  pna_gpu_gather_wait(pna_gpu_comm *comm);
uint64_t pna_gpu_gather_ticket(const pna_gpu_comm *comm);
int  pna_gpu_gather_wait_for(pna_gpu_comm *comm, uint64_t ticket);
int  pna_gather_verdict(const uint64_t *pairs, int nranks, int root, uint64_t *sizes, uint64_t *offs);
/* offs[r] = where rank r's part starts in the gathered stream, offs[nranks] = the total (host arithmetic; what the gather above uses) */
int  pna_gather_offsets(const uint64_t *sizes, int nranks, uint64_t *offs);

/* ---- Archive::write_file / write_stream_entry (lib/src/archive/write.rs:276-299,730-777): an entry written WHILE its data arrives.
 * The record has no fSIZ (the size is not known when FHED goes out): FHED, the caller's already framed extra + metadata chunks
 * (`meta`, may be NULL), then the compressed stream as FDAT chunks -- one per burst the encoder hands to the ChunkStreamWriter
 * (lib/src/chunk/write.rs:32-47: every write() becomes a chunk of at most max_chunk_size bytes; the encoders flush in bursts of at most
 * 32 KiB, the size of the FDAT / SDAT pieces in the reference's stream-written fixtures) --, then FEND.  begin() emits FHED + meta,
 * write() buffers like CompressionWriter::write, finish() compresses (group commit with the context's other writers), emits the FDAT
 * chunks and FEND and frees the writer; abort() frees it without output (the archive is then unusable, as in the reference).
 * max_chunk_size 0 = u32::MAX.  Thread rules: those of pna_gpu_stream_*. */
typedef struct pna_gpu_entry_writer pna_gpu_entry_writer;
int  pna_gpu_stream_entry_begin(pna_gpu_ctx *ctx, int algo, int level, const char *name, const void *meta, size_t meta_len,
                                uint32_t max_chunk_size, pna_sink_fn sink, void *user, pna_gpu_entry_writer **out);
int  pna_gpu_stream_entry_write(pna_gpu_entry_writer *w, const void *buf, size_t len);
int  pna_gpu_stream_entry_finish(pna_gpu_entry_writer *w);
void pna_gpu_stream_entry_abort(pna_gpu_entry_writer *w);

/* ---- streaming facade with the shape of CompressionWriter<W> (lib/src/compress.rs:32-41,66-75):
 * write() buffers, finish() == try_into_inner(): compresses and pushes the stream into the sink (== W::write).
 * THREADS: unlike the rest of this header, the stream functions may be called from any number of host threads on ONE context at
 * the same time -- that is how the reference drives its encoders (one writer per rayon task, cli/src/command/core.rs:505-517).
 * finish() is a group commit: concurrent finishes are collected into one device batch (the thread that finds no batch in flight
 * leads it; finishes arriving meanwhile form the next batch) and every caller receives its own stream through its own sink on
 * its own thread.  Each stream object belongs to one thread; do not mix stream calls with the context's other entry points without
 * external synchronisation.  PNA_STREAM_LINGER_US (environment) fixes how long a leader waits for stragglers before it submits; unset: 200 us once more than one
 * writer has been seen, nothing for a lone writer. */
typedef struct pna_gpu_stream pna_gpu_stream;
int  pna_gpu_stream_new(pna_gpu_ctx *ctx, int algo, int level, pna_sink_fn sink, void *user, pna_gpu_stream **out);
int  pna_gpu_stream_write(pna_gpu_stream *s, const void *buf, size_t len);
int  pna_gpu_stream_flush(pna_gpu_stream *s);           /* no-op like the buffered encoders' flush        */
int  pna_gpu_stream_finish(pna_gpu_stream *s);          /* consumes s                                      */
void pna_gpu_stream_abort(pna_gpu_stream *s);           /* drop without output (failed builder is discarded) */
/* device batches run / entries carried / largest batch so far on behalf of pna_gpu_stream_finish (any pointer may be NULL) */
int  pna_gpu_stream_stats(pna_gpu_ctx *ctx, uint64_t *batches, uint64_t *entries, uint64_t *largest_batch);

/* ---- solid mode: one logical stream, split into independent 1 MiB frames inside the kernels
 * (replaces the single serial encoder of SolidArchive, lib/src/archive/write.rs:443-470,575-580,716-727). */
int  pna_gpu_compress_solid(pna_gpu_ctx *ctx, int algo, int level, const void *src, size_t src_len,
                            pna_sink_fn sink, void *user);

/* ---- introspection used by tests and the benchmark */
typedef struct {
    double   ms_lz, ms_stats, ms_lit, ms_seq, ms_pack;   /* HIP-event time of each stage of the last batch (large zstd batches run the literal coder
                                                          * beside the sequence coder on a second stream: ms_lit is then ~0 and ms_seq covers both) */
    uint64_t in_bytes, out_bytes, n_segments, n_blocks;
    double   ms_frame;                                   /* k_frame (pna_gpu_create_archive_device only)       */
    double   ms_cipher;                                  /* k_aes_* (archives written with a cipher)           */
    double   ms_lz_match;                                /* of ms_lz: the match kernel (k_lzm) launches of the split LZ stage, summed */
    uint64_t lz_match_launches;                          /* ... and how many there were (0: the batch went through the one-kernel form).  After a DEFLATE DECODE call: the large foreign
                                                          * streams that were decoded in chunks between block starts found by trial (the others of that size took one wave's walk) */
    uint32_t blk_log;                                    /* block size of the last (sub-)batch = 1 << blk_log: 17, or 13..16 in latency mode   */
    uint32_t lz_units;                                   /* latency mode: workgroups (units) of the LZ stage's launch; 0: one per segment       */
} pna_gpu_timing;
int  pna_gpu_last_timing(const pna_gpu_ctx *ctx, pna_gpu_timing *out);

/* Which forms of the decoders the latest decode call of the context ran (tests assert that the form they are about was not re-routed).
 * zstd calls fill the first three fields, deflate calls the last three, xz calls none; the others are 0. */
typedef struct {
    uint64_t zstd_executor_frames;    /* frames executed by the parallel executor (option zexec_par_min_mib)                                  */
    uint64_t zstd_workgroup_frames;   /* frames decoded by the one-workgroup kernel (zdec_serial, or frames the bounded pipeline could not take) */
    uint64_t zstd_listed_entries;     /* entries whose frames were listed one by one (frames off this library's grid, skippable frames)        */
    uint64_t inflate_lane_pieces;     /* pieces the lane-per-piece decoder walked (0: it did not run: fewer than 1 024 pieces, inflate_serial)  */
    uint64_t inflate_lane_streams;    /* streams it decoded (the others took the wave-per-stream walk or the chunk decoder)                    */
    uint64_t inflate_chunk_streams;   /* large foreign streams decoded in chunks between block starts found by trial                           */
} pna_gpu_decode_forms;
int  pna_gpu_last_decode_forms(const pna_gpu_ctx *ctx, pna_gpu_decode_forms *out);

/* LZ-stage outputs of the last device batch for one block (tests compare them with the oracle's pna_lz_block).
 * seqs: packed u64 (off:20 | ml:18<<20 | ll:18<<38). Copies at most cap_* items; returns counts. */
int  pna_gpu_debug_block(pna_gpu_ctx *ctx, uint32_t block, uint64_t *seqs, uint32_t cap_seqs, uint32_t *nseq,
                         uint8_t *lits, uint32_t cap_lits, uint32_t *nlit);

/* Host walk through the device CRC schedule of k_frame with the same tables; returns crc32("FDAT" || payload).
 * CPU-only tests use it to check the table construction; it is not on any product path. */
uint32_t pna_gpu_debug_crc_schedule(const void *payload, size_t len);

/* Page-locked staging memory the context holds (the host pipelines' slots): tests pin the bounded-memory claims with it; not on any product path. */
uint64_t pna_gpu_debug_pinned_bytes(pna_gpu_ctx *ctx);

/* Diagnostic build of the LZ kernel (ctx created with flag 0x100): per-phase s_memtime sums over all waves, cleared on read. */
int  pna_gpu_debug_lz_stamps(pna_gpu_ctx *ctx, unsigned long long *out8);

/* ---- benchmark support (not part of the reference's surface): fills d_dst with `n_files` synthetic files of
 * `file_len` bytes each (file i at i * stride), bit-identical to oracle/corpus_model.c. kind: 0 enwik-style text,
 * 1 random-text, 2 random bytes, 3 zeros, 4 repeated byte. */
int  pna_bench_corpus_fill_device(pna_gpu_ctx *ctx, int kind, uint64_t first_file, uint64_t n_files,
                                  uint64_t file_len, uint64_t stride, void *d_dst, void *hip_stream);
/* The reference's fan-out (one entry per task, FIFO, cli/src/command/core.rs:496-537) on `threads` host threads over the streaming
 * facade: stream_new / one write of the whole entry / finish into a counting sink.  Returns seconds; *out_bytes = compressed bytes
 * the sinks received, *rc = first error. */
double pna_bench_stream_threads(pna_gpu_ctx *ctx, int algo, int level, unsigned threads, size_t n, const void *const *src,
                                const size_t *src_len, uint64_t *out_bytes, int *rc);

#ifdef __cplusplus
}
#endif
#endif
