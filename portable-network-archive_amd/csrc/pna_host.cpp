// pna_host.cpp -- context, options, level sets and the ENCODE core of libpna_gpu.so (plans, the entropy / framing launches of one sub-batch, the
// device-resident entry points); the LZ stage's host side lives in pna_lz.cpp, the host pipelines, the read side and the streaming facade live in pna_pipeline.cpp, pna_extract.cpp, pna_decode.cpp and
// pna_stream.cpp, what they share in pna_ctx.h.
#include "pna_ctx.h"
#include "xz_enc_core.h"
static const TuningName TUNING_NAMES[] = {
    {"lz_split", "PNA_LZ_SPLIT", &Tuning::lz_split, 0, 2}, {"lz_split_blocks", "PNA_LZ_SPLIT_BLOCKS", &Tuning::lz_split_blocks, 8, 1 << 17},
    {"lz_split_min", "PNA_LZ_SPLIT_MIN", &Tuning::lz_split_min, 0, 1 << 30}, {"lz_pbuf_fail", "PNA_LZ_PBUF_FAIL", &Tuning::lz_pbuf_fail, 0, 1},
    {"max_chunk_size", "PNA_MAX_CHUNK_SIZE", &Tuning::max_chunk_size, 0, 0xFFFFFFFFl},
    {"sub_mib", "PNA_SUB_MIB", &Tuning::sub_mib, 1, 16384}, {"stage_threads", "PNA_STAGE_THREADS", &Tuning::stage_threads, 0, 64},
    {"extract_win_mib", "PNA_EXTRACT_WIN_MIB", &Tuning::extract_win_mib, 1, 1 << 20}, {"batch_piece_mib", "PNA_BATCH_PIECE_MIB", &Tuning::batch_piece_mib, 0, 1 << 20}, {"solid_win_mib", "PNA_SOLID_WIN_MIB", &Tuning::solid_win_mib, 1, 1 << 16}, {"diff_slot_mib", "PNA_DIFF_SLOT_MIB", &Tuning::diff_slot_mib, 1, 1 << 14},
    {"inflate_serial", "PNA_INFLATE_SERIAL", &Tuning::inflate_serial, 0, 1}, {"zdec_serial", "PNA_ZDEC_SERIAL", &Tuning::zdec_serial, 0, 1}, {"zdec_dbg", "PNA_ZDEC_DBG", &Tuning::zdec_dbg, 0, 15},
    {"blk_log", "PNA_BLK_LOG", &Tuning::blk_log, 0, PNA_BLK_LOG}, {"unit_log", "PNA_LZ_UNIT_LOG", &Tuning::unit_log, 0, 20},
    {"latency_max_mib", "PNA_LATENCY_MAX_MIB", &Tuning::latency_max_mib, 0, 1 << 20}, {"hist_by_block", "PNA_HIST_BY_BLOCK", &Tuning::hist_by_block, -1, 1},
    {"d2h_wgs", "PNA_D2H_WGS", &Tuning::d2h_wgs, 0, 4096}, {"trace", "PNA_TRACE", &Tuning::trace, 0, 1}, {"dev_layout", "PNA_DEV_LAYOUT", &Tuning::dev_layout, 0, 1}, {"strong_gtab", "PNA_STRONG_GTAB", &Tuning::strong_gtab, 0, 1}, {"win32k", "PNA_WIN32K", &Tuning::win32k, 0, 2}, {"tab3", "PNA_TAB3", &Tuning::tab3, 0, 1}, {"far1", "PNA_FAR1", &Tuning::far1, 0, 1}, {"seq_hist", "PNA_SEQ_HIST", &Tuning::seq_hist, 0, 1}, {"strong2", "PNA_STRONG2", &Tuning::strong2, 0, 1}, {"small_geometry", "PNA_SMALL_GEOMETRY", &Tuning::small_geometry, 0, 1}, {"mtile", "PNA_MTILE", &Tuning::mtile, 0, 2048}, {"zexec_par_min_mib", "PNA_ZEXEC_PAR_MIN_MIB", &Tuning::zexec_par_min_mib, 0, 1 << 20}, {"zexec_win_mib", "PNA_ZEXEC_WIN_MIB", &Tuning::zexec_win_mib, 1, 1024}, {"zdec_fallback_max_mib", "PNA_ZDEC_FALLBACK_MAX_MIB", &Tuning::zdec_fallback_max_mib, 0, 1 << 30}, {"stream_batch_mib", "PNA_STREAM_BATCH_MIB", &Tuning::stream_batch_mib, 1, 1 << 16}, {"stream_gather_wgs", "PNA_STREAM_GATHER_WGS", &Tuning::stream_gather_wgs, 0, 4096}, {"stream_overlap_mib", "PNA_STREAM_OVERLAP_MIB", &Tuning::stream_overlap_mib, 0, 1 << 16}, {"single_frame", "PNA_SINGLE_FRAME", &Tuning::single_frame, 0, 1}, {"lazy2", "PNA_LAZY2", &Tuning::lazy2, 0, 2}, {"tail_units", "PNA_TAIL_UNITS", &Tuning::tail_units, 0, 1}, {"lit_beside_seq", "PNA_LIT_BESIDE_SEQ", &Tuning::lit_beside_seq, 0, 1},
    {"xz_encode", "PNA_XZ_ENCODE", &Tuning::xz_encode, 0, 1}, {"camellia", "PNA_CAMELLIA", &Tuning::camellia, 0, 1},
    {"kdf_device", "PNA_KDF_DEVICE", &Tuning::kdf_device, 0, 1 << 30}, {"kdf_mem_mib", "PNA_KDF_MEM_MIB", &Tuning::kdf_mem_mib, 0, 32768},
    {"store_unfused", "PNA_STORE_UNFUSED", &Tuning::store_unfused, -1, 1},
};

extern "C" const char *pna_gpu_strerror(int code) {
    switch (code) {
        case PNA_OK: return "ok";
        case PNA_E_NODEVICE: return "no usable HIP device";
        case PNA_E_INVAL: return "invalid argument";
        case PNA_E_NOMEM: return "out of memory";
        case PNA_E_DSTSIZE: return "destination too small";
        case PNA_E_HIP: return "HIP error";
        case PNA_E_SINK: return "sink callback failed";
        case PNA_E_UNSUPPORTED: return "algorithm not supported by this build";
        default: return "unknown error";
    }
}
extern "C" const char *pna_gpu_last_error(const pna_gpu_ctx *ctx) { return ctx ? ctx->err.c_str() : "null context"; }

static bool mtile_ok(long v) { return v == 0 || v == 256 || v == 512 || v == 1024 || v == 2048; }
extern "C" int pna_gpu_init(pna_gpu_ctx **out, int device_id, uint32_t flags) {
    if (!out) return PNA_E_INVAL;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return PNA_E_NODEVICE;
    if (device_id < 0 || device_id >= n) return PNA_E_INVAL;
    if (hipSetDevice(device_id) != hipSuccess) return PNA_E_NODEVICE;
    pna_gpu_ctx *c = new pna_gpu_ctx();
    c->device = device_id;
    { int cus = 0; if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device_id) == hipSuccess && cus > 0) c->n_cus = (uint32_t)cus; }
    c->flags = (flags & PNA_F_DEFAULT) ? (F_HUF | F_FSE | F_LAZY | F_FAR | F_ADOPT | F_INS2) : (flags & INIT_LEVEL_SET);
    c->flags &= ~F_REP;                    // repeat-offset codes are not produced by this build
    for (const TuningName &t : TUNING_NAMES)
        if (const char *e = getenv(t.env)) { const long v = atol(e); if (v >= t.lo && v <= t.hi && (t.field != &Tuning::mtile || mtile_ok(v))) c->tun.*(t.field) = v; }
    if (const char *pm = getenv("PNA_STREAM_POOL_MIB")) c->pool_cap = (size_t)std::min<unsigned long>(strtoul(pm, nullptr, 10), 1ul << 20) << 20;
    if (const char *lg = getenv("PNA_STREAM_LINGER_US")) c->comb_linger_us = (uint32_t)std::min<unsigned long>(strtoul(lg, nullptr, 10), 100000ul);
    if (!(flags & PNA_F_DEFAULT)) c->flags |= flags & INIT_DIAG;  // diagnostics (pna_dev.h): phase stamps, the serial fallback in k_lz, the one-kernel / two-phase sequence coder
    c->flags |= flags & (PNA_F_LZ_FUSED | PNA_F_LZ_WAVEPARSE);  // the form of the LZ stage: honoured next to PNA_F_DEFAULT as well
    c->call_flags = c->flags;
    if (hipStreamCreate(&c->stream) != hipSuccess) { delete c; return PNA_E_NODEVICE; }
    for (auto &e : c->ev) if (hipEventCreate(&e) != hipSuccess) { delete c; return PNA_E_NODEVICE; }
    {   // the predefined sequence tables of this device (k_entropy.hip g_def_tab): built by the first context on it
        static std::mutex mu; static bool built[64] = {};
        std::lock_guard<std::mutex> lk(mu);
        if (device_id >= 0 && device_id < 64 && !built[device_id]) {
            launch_default_tables(c->stream);
            if (hipStreamSynchronize(c->stream) != hipSuccess || hipGetLastError() != hipSuccess) { delete c; return PNA_E_HIP; }
            built[device_id] = true;
        }
    }
    *out = c;
    return PNA_OK;
}

extern "C" int pna_gpu_set_option(pna_gpu_ctx *c, const char *name, long value) {
    if (!c || !name) return PNA_E_INVAL;
    if (!strcmp(name, "stream_pool_mib")) { if (value < 0) return PNA_E_INVAL; c->pool_cap = (size_t)std::min<long>(value, 1l << 20) << 20; return PNA_OK; }
    if (!strcmp(name, "stream_linger_us")) { c->comb_linger_us = value < 0 ? 0xFFFFFFFFu : (uint32_t)std::min<long>(value, 100000); return PNA_OK; }
    for (const TuningName &t : TUNING_NAMES)
        if (!strcmp(name, t.name)) {
            if (t.field == &Tuning::mtile && !mtile_ok(value)) return fail(c, PNA_E_INVAL, "mtile: 0, 256, 512, 1024 or 2048");
            if (value < t.lo || value > t.hi) return fail(c, PNA_E_INVAL, "option value out of range");
            if (t.field == &Tuning::blk_log && value != 0 && value < (long)BLK_LOG_MIN) return fail(c, PNA_E_INVAL, "blk_log: 0 or 13..17");
            c->tun.*(t.field) = value; return PNA_OK;
        }
    return fail(c, PNA_E_INVAL, "unknown option");
}

extern "C" void pna_gpu_shutdown(pna_gpu_ctx *c) {
    if (c) { for (void *a : c->pool_arenas) (void)hipHostFree(a); c->pool_arenas.clear(); c->pool_free.clear(); for (auto &b : c->s_out) b.release(); for (auto &b : c->st_in) b.release(); for (auto &b : c->st_out) b.release(); for (auto &b : c->s_segs) b.release();
             if (c->s_h2d) (void)hipStreamDestroy(c->s_h2d); if (c->s_d2h) (void)hipStreamDestroy(c->s_d2h); for (auto &e : c->s_ev) if (e) (void)hipEventDestroy(e); }
    if (!c) return;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    for (DevBuf *b : {&c->plan, &c->d_tail, &c->blk, &c->tabs, &c->seqs, &c->lits, &c->litc, &c->seqc, &c->seqw, &c->pbuf, &c->seg_size,
                      &c->seg_off, &c->stage_in, &c->stage_out, &c->z_words, &c->z_rep, &c->z_zxf, &c->z_spec, &c->z_big, &c->z_one, &c->ctab, &c->c_vocab, &c->c_cum, &c->c_phr,
                      &c->gtab, &c->fr_desc, &c->fr_blob, &c->fr_segdst, &c->fr_entoff, &c->crc_tabs, &c->aes_tabs, &c->ci_units, &c->ci_ivs, &c->ci_keys, &c->ci_gcm, &c->ci_spread, &c->ci_spread_desc, &c->z_vp, &c->z_pb, &c->z_mode, &c->x_arc, &c->x_pk, &c->x_raw[0], &c->x_raw[1], &c->x_desc, &c->x_place, &c->x_flag, &c->x_tags, &c->x_plen, &c->aes_dtabs, &c->solid_plain, &c->solid_desc, &c->solid_blob, &c->solid_place, &c->solid_adler, &c->solid_carry, &c->z_ents, &c->z_frames, &c->z_lit, &c->z_fx, &c->z_blocks, &c->z_tabs, &c->z_seqs, &c->z_hlist, &c->z_slist, &c->z_work, &c->z_fb, &c->z_cbase, &c->z_apart}) b->release();
    for (auto &b : c->lent) (void)hipHostFree((void *)b.first);          // (buffers the host never gave back)
    c->lent.clear();
    for (PinBuf *b : {&c->h_entoff, &c->h_plan, &c->h_tail, &c->h_desc, &c->h_blob, &c->h_segdst, &c->h_segoff, &c->hp_in[0], &c->hp_in[1], &c->hp_in[2], &c->hp_in[3], &c->hp_out[0], &c->hp_out[1]}) b->release();
    for (DevBuf *b : {&c->dp_in[0], &c->dp_in[1], &c->dp_in[2], &c->dp_in[3], &c->dp_out[0], &c->dp_out[1]}) b->release();
    for (auto &e : c->ev_in) if (e) (void)hipEventDestroy(e);
    for (auto &e : c->ev_out) if (e) (void)hipEventDestroy(e);
    for (auto &e : c->ev_lz) if (e) (void)hipEventDestroy(e);
    for (auto &e : c->lzm_ev) if (e) (void)hipEventDestroy(e);
    for (auto &e : c->ev_ci) if (e) (void)hipEventDestroy(e);
    for (auto &e : c->ev_en) if (e) (void)hipEventDestroy(e);
    if (c->ev_join) (void)hipEventDestroy(c->ev_join);
    if (c->ev_fork) (void)hipEventDestroy(c->ev_fork);
    if (c->aux) (void)hipStreamDestroy(c->aux);
    if (c->cp_in) (void)hipStreamDestroy(c->cp_in);
    if (c->cp_out) (void)hipStreamDestroy(c->cp_out);
    for (DevBuf *b : {&c->v_crc, &c->v_seg, &c->v_ent, &c->v_out, &c->df_dev[0], &c->df_dev[1], &c->df_pieces, &c->df_first}) b->release();
    for (auto &b : c->df_pin) b.release();
    if (c->df_cp) (void)hipStreamDestroy(c->df_cp);
    for (auto &e : c->df_ev_cp) if (e) (void)hipEventDestroy(e);
    for (auto &e : c->df_ev_k) if (e) (void)hipEventDestroy(e);
    for (auto &e : c->df_tev) if (e) (void)hipEventDestroy(e);
    c->xs_pieces.release();
    for (DevBuf *b : {&c->st_pieces, &c->st_lits, &c->st_chunks, &c->st_states}) b->release();
    for (auto &e : c->st_ev) if (e) (void)hipEventDestroy(e);
    for (DevBuf *b : {&c->xz_in, &c->xz_scan, &c->xz_blocks, &c->xz_pieces, &c->xz_acc, &c->cam_tabs, &c->ci_ckeys, &c->kdf_mem, &c->kdf_jobs, &c->kdf_seeds, &c->kdf_fin}) b->release();
    for (auto &e : c->kdf_ev) if (e) (void)hipEventDestroy(e);
    for (auto &e : c->xs_tev) if (e) (void)hipEventDestroy(e);
    if (c->x_cp) (void)hipStreamDestroy(c->x_cp);
    for (auto &e : c->x_ev) if (e) (void)hipEventDestroy(e);
    if (c->x_done) (void)hipEventDestroy(c->x_done);
    for (auto &e : c->ev) if (e) (void)hipEventDestroy(e);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

extern "C" size_t pna_gpu_bound(int algo, size_t n) {
    if (algo == PNA_ALGO_STORE) return n;
    // xz: every chunk stored (3 bytes per block of the smallest size), 24 bytes per 1 MiB block, the stream's header, Index and footer (xz_enc_core.h)
    if (algo == PNA_ALGO_XZ) return (size_t)xze_bound(n);
    // (per block of the SMALLEST size a batch may be cut into -- latency mode, BLK_LOG_MIN --: deflate 5 bytes of stored-block header + 5 of sync flush,
    // zstd 3 bytes of block header; per segment / 128 KiB the older, coarser allowances)
    constexpr size_t BMIN = (size_t)1 << BLK_LOG_MIN;
    if (algo == PNA_ALGO_DEFLATE) { size_t b = (n + BMIN - 1) / BMIN; if (!b) b = 1; return n + b * 10 + (n >> PNA_BLK_LOG) * 16 + 64; }
    size_t segs = (n + SEG_SIZE - 1) / SEG_SIZE; if (segs == 0) segs = 1;
    size_t blks = (n + BMIN - 1) / BMIN + segs;
    return n + segs * 6 + blks * 3 + 16;
}

extern "C" int pna_gpu_clamp_level(int algo, int level) {
    if (algo == PNA_ALGO_ZSTD) {            // lib/src/compress/zstandard.rs:13,43-57 (min_c_level .. 22, default 3)
        if (level == PNA_LEVEL_DEFAULT) return 3;
        if (level < -131072) return -131072;
        return level > 22 ? 22 : level;
    }
    if (algo == PNA_ALGO_DEFLATE) {         // lib/src/compress/deflate.rs:33-38,89-101
        if (level == PNA_LEVEL_DEFAULT) return 6;
        // Custom(n) => Compression::new((n as u32).clamp(0, 9)): a negative n wraps to a large u32 and clamps to 9 (deflate.rs:89-101)
        return (uint32_t)level > 9u ? 9 : level;
    }
    if (algo == PNA_ALGO_XZ) {              // lib/src/compress/xz.rs:36-46 (default 6, 0 .. 9)
        if (level == PNA_LEVEL_DEFAULT) return 6;
        return level < 0 ? 0 : (level > 9 ? 9 : level);
    }
    return 0;
}

// Parameter sets behind the reference's level scale (CompressionLevel -> ZstdCompressionLevel / flate2::Compression,
// lib/src/compress/zstandard.rs:43-57, deflate.rs:89-101; PNA_LEVEL_DEFAULT and zstd level 0 = the default):
//   stored    deflate 0                      Compression::none(): stored blocks only (no match finder, header 78 01)
//   fast      zstd < 0 and 1, deflate 1..3   every position in the table, look-back = the LDS window, no backward adoption; lazy deferral as below
//   light     zstd 2,         deflate 4..8   + even-position table, backward adoption (two rounds), 1 MiB look-back (zstd), lazy deferral over three positions
//   default   zstd 0, 3                      + a third adoption round (matches move back by up to 7 positions): ratio at the reference's default level (round 4)
//   high      zstd 4..9,      deflate 9      the default set on the 16 KiB-window geometry (more table slots, more candidates verified in HBM / L2) + a fourth adoption round over eight positions, 15 back bytes; deflate: + third round
//   max       zstd 10..22                    + the match kernel's hash table in global memory: 2^19 slots per segment instead of what LDS holds
// (the match finder's geometry per set: lz_level_set, pna_lz.cpp)
static uint32_t level_flags(const pna_gpu_ctx *c, int algo, int level) {
    const int lv = pna_gpu_clamp_level(algo, level);
    const bool fast = algo == PNA_ALGO_DEFLATE ? lv <= 3 : (lv < 0 || lv == 1);
    const bool balanced = false;   // (the set without lazy deferral -- zstd 2, deflate 4..5 until round 3 -- is as fast as the default set since the parse kernel looks ahead for free; the levels take the default set, the bits remain)
    const bool strong = algo == PNA_ALGO_DEFLATE ? lv >= 9 : (lv >= 3 || lv == 0);      // (zstd 0 = the default = 3; round 4: the third adoption round from the default level on)
    if (fast) return c->flags & ~(F_FAR | F_ADOPT | F_INS2 | F_STRONG);      // (lazy deferral stays: the parse kernel does it for free -- zstd-1 2.510 -> 2.54 at the same speed)
    if (balanced) return c->flags & ~(F_LAZY | F_STRONG);
    if (strong && (c->flags & F_ADOPT) && (c->flags & F_LAZY)) return c->flags | F_STRONG;
    return c->flags;
}
// xz runs the LZ stage of a zstd level (matches capped at LZMA's 273 bytes): xz 0 the fast set, 1..3 the default set, 4..6 the high set, 7..9 the max set
static const int XZ_LZ_LEVEL[10] = {1, 3, 3, 3, 6, 6, 6, 10, 10, 10};
void set_call_level(pna_gpu_ctx *c, int algo, int level) {
    if (algo == PNA_ALGO_STORE) { c->call_xz = c->call_stored = false; return; }              // no codec runs: the level means nothing (pna_gpu_clamp_level: 0)
    c->call_xz = algo == PNA_ALGO_XZ;
    if (c->call_xz) { level = XZ_LZ_LEVEL[pna_gpu_clamp_level(PNA_ALGO_XZ, level)]; algo = PNA_ALGO_ZSTD; }
    c->call_flags = level_flags(c, algo, level);
    c->call_stored = algo == PNA_ALGO_DEFLATE && pna_gpu_clamp_level(algo, level) == 0;
    c->lz = lz_level_set(c, algo, level, c->call_xz);
}

// blocks an entry of `len` bytes takes in the per-block workspace (sub-batches are cut by block count); a forced block size counts as such
extern "C" int pna_gpu_last_timing(const pna_gpu_ctx *c, pna_gpu_timing *out) {
    if (!c || !out) return PNA_E_INVAL;
    *out = c->timing; out->blk_log = c->last_blk_log; out->lz_units = c->last_units; return PNA_OK;
}
extern "C" int pna_gpu_last_decode_forms(const pna_gpu_ctx *c, pna_gpu_decode_forms *out) {
    if (!c || !out) return PNA_E_INVAL;
    *out = c->forms; return PNA_OK;
}

// ---------------------------------------------------------------------------------------------------------
// ---- CRC-32 tables of the framing kernel (k_frame.hip explains the algebra)
uint32_t crc_gf2_mulmod(uint32_t a, uint32_t b);
uint32_t crc_gf2_xpow(uint64_t e);
static uint32_t gf2_mulmod(uint32_t a, uint32_t b) {          // a * b mod P, reflected bit order (bit 31 = x^0)
    uint32_t p = 0;
    for (int i = 0; i < 32; i++) { if (a & 0x80000000u) p ^= b; a <<= 1; b = (b & 1) ? (b >> 1) ^ 0xEDB88320u : b >> 1; }
    return p;
}
static uint32_t gf2_xpow(uint64_t e) {                        // x^e mod P
    uint32_t r = 0x80000000u, base = 0x40000000u;
    while (e) { if (e & 1) r = gf2_mulmod(base, r); base = gf2_mulmod(base, base); e >>= 1; }
    return r;
}
static void build_crc_tabs(CrcTabs &t) {
    for (uint32_t i = 0; i < 256; i++) { uint32_t v = i; for (int k = 0; k < 8; k++) v = (v & 1) ? (v >> 1) ^ 0xEDB88320u : v >> 1; t.T[0][i] = v; }
    for (int k = 1; k < 4; k++) for (uint32_t i = 0; i < 256; i++) t.T[k][i] = (t.T[k - 1][i] >> 8) ^ t.T[0][t.T[k - 1][i] & 0xFF];
    const uint32_t z = gf2_xpow(8ull * 16320);
    for (int j = 0; j < 4; j++) for (uint32_t b = 0; b < 256; b++) t.Z[j][b] = gf2_mulmod(z, b << (8 * j));
    for (int j = 0; j < 8; j++) t.sh[j] = gf2_xpow(8ull * 64 << j);
    for (int m = 1; m <= 4; m++) for (uint32_t k = 0; k < 64; k++) t.pw[m - 1][k] = gf2_xpow(8ull * 64 * m * k);
}
uint32_t crc_gf2_mulmod(uint32_t a, uint32_t b) { return gf2_mulmod(a, b); }
uint32_t crc_gf2_xpow(uint64_t e) { return gf2_xpow(e); }
int ensure_crc(pna_gpu_ctx *c) {
    if (c->crc_ready) return PNA_OK;
    CrcTabs t; build_crc_tabs(t);
    if (c->crc_tabs.ensure(sizeof(t))) return fail(c, PNA_E_NOMEM, "crc tables");
    HIPCHK(c, hipMemcpy(c->crc_tabs.p, &t, sizeof(t), hipMemcpyHostToDevice));
    c->crc_ready = true;
    return PNA_OK;
}

// Host walk through k_frame's CRC schedule with the same tables (lane states, Z_16320 between tiles, fold tree): lets the
// CPU-only test suite check the algebra and the table construction against pna_crc32 without a GPU.  Not a product path.
extern "C" uint32_t pna_gpu_debug_crc_schedule(const void *payload, size_t len) {
    static const CrcTabs t = [] { CrcTabs x; build_crc_tabs(x); return x; }();      // initialised once, thread-safe (C++11 static)
    const uint8_t *pl = (const uint8_t *)payload;
    const uint64_t n = 4 + (uint64_t)len, ntile = (n + 16383) / 16384, pad = ntile * 16384 - n;
    static const uint8_t ty[4] = {0x46 ^ 0xFF, 0x44 ^ 0xFF, 0x41 ^ 0xFF, 0x54 ^ 0xFF};
    uint32_t lane[256] = {0};
    for (uint64_t k = 0; k < ntile; k++)
        for (uint32_t l = 0; l < 256; l++) {
            uint32_t s = lane[l];
            s = t.Z[0][s & 0xFF] ^ t.Z[1][(s >> 8) & 0xFF] ^ t.Z[2][(s >> 16) & 0xFF] ^ t.Z[3][s >> 24];
            for (uint32_t j = 0; j < 16; j++) {
                uint32_t w = 0;
                for (uint32_t b = 0; b < 4; b++) {
                    const uint64_t p = k * 16384 + l * 64 + 4 * j + b;
                    const uint8_t v = p < pad ? 0 : (p < pad + 4 ? ty[p - pad] : pl[p - pad - 4]);
                    w |= (uint32_t)v << (8 * b);
                }
                const uint32_t x = s ^ w;
                s = t.T[3][x & 0xFF] ^ t.T[2][(x >> 8) & 0xFF] ^ t.T[1][(x >> 16) & 0xFF] ^ t.T[0][x >> 24];
            }
            lane[l] = s;
        }
    for (uint32_t j = 0; j < 8; j++) {
        const uint32_t st = 1u << j;
        for (uint32_t l = 0; l < 256; l += 2 * st) lane[l] = gf2_mulmod(t.sh[j], lane[l]) ^ lane[l + st];
    }
    return ~lane[0];
}

// names[e] for the batch's global entry index e; solid: one SDAT chunk per segment of the (single) entry; cipher + ivs (16 bytes per
// global entry index): the payloads are encrypted in place before their CRC-32 is taken
// largest FDAT chunk the device paths write: the CRC kernel takes "FDAT" || data as one message of at most 2^32 - 1 bytes (the reference's default cuts
// at u32::MAX: the same chunks unless an entry's compressed payload exceeds 4 GiB - 5 bytes)
uint64_t chunk_limit(uint32_t max_chunk) { return max_chunk ? std::min<uint64_t>(max_chunk, 0xFFFFFFFBull) : 0xFFFFFFFBull; }
size_t meta_len(const pna_gpu_entry_meta *m, size_t e) {
    if (!m) return 0;
    return (m->extra && m->extra_len ? m->extra_len[e] : 0) + (m->facets && m->facets_len ? m->facets_len[e] : 0);
}
// a blob of already framed chunks: lengths consistent, CRCs right, none of the chunk types this library writes itself
bool meta_blob_ok(const uint8_t *p, size_t n) {
    size_t pos = 0;
    while (pos < n) {
        PnaChunk ch;
        if (next_chunk(p, n, pos, ch)) return false;
        for (const char *own : {"FHED", "FDAT", "FEND", "fSIZ", "PHSF", "SHED", "SDAT", "SEND", "AHED", "AEND", "ANXT"}) if (memcmp(ch.type, own, 4) == 0) return false;
        if (!chunk_crc_ok(ch)) return false;
    }
    return true;
}
// prefix = FHED | fSIZ | rest  ->  FHED | extra | fSIZ | facets | rest   (NormalEntry::write_chunks_to, lib/src/entry.rs:895-911)
void splice_meta(std::vector<uint8_t> &pre, const pna_gpu_entry_meta *m, size_t e) {
    if (!meta_len(m, e)) return;
    const size_t c0 = 12 + (size_t)rd_be32(pre.data()), c1 = 12 + (size_t)rd_be32(pre.data() + c0);
    std::vector<uint8_t> out(pre.begin(), pre.begin() + c0);
    if (m->extra && m->extra_len && m->extra_len[e]) out.insert(out.end(), (const uint8_t *)m->extra[e], (const uint8_t *)m->extra[e] + m->extra_len[e]);
    out.insert(out.end(), pre.begin() + c0, pre.begin() + c0 + c1);
    if (m->facets && m->facets_len && m->facets_len[e]) out.insert(out.end(), (const uint8_t *)m->facets[e], (const uint8_t *)m->facets[e] + m->facets_len[e]);
    out.insert(out.end(), pre.begin() + c0 + c1, pre.end());
    pre.swap(out);
}

// stage times of a finished sub-batch from its events (the stream has been waited for)
static int collect_timing(pna_gpu_ctx *c, bool defl, uint32_t nseg, uint32_t nblk, bool with_cipher) {
    float ms[6] = {0, 0, 0, 0, 0, 0}, msf = 0;
    (void)hipEventElapsedTime(&msf, c->ev[6], c->ev[7]);
    c->timing.ms_frame += msf;
    float mc = 0;                                             // the cipher kernels run inside the "pack" interval: report them apart
    if (with_cipher) { (void)hipEventElapsedTime(&mc, c->ev_ci[0], c->ev_ci[1]); c->timing.ms_cipher += mc; c->timing.ms_pack -= mc; }
    if (defl) {
        for (int i = 0; i < 6; i++) (void)hipEventElapsedTime(&ms[i], c->ev[i], c->ev[i + 1]);
    } else {
        // k_lz: first launch to last completion; the entropy stage's statistics, literal and sequence parts; "pack" = from the end of the
        // entropy stage to the end of the write kernels (plan + scan + layout + write)
        (void)hipEventElapsedTime(&ms[0], c->ev_lz[0], c->ev_lz[1]);
        for (int i = 0; i < 3; i++) (void)hipEventElapsedTime(&ms[1 + i], c->ev_en[i], c->ev_en[i + 1]);
        (void)hipEventElapsedTime(&ms[4], c->ev_en[3], c->ev[6]);
    }
    c->timing.ms_lz += ms[0]; c->timing.ms_stats += ms[1]; c->timing.ms_lit += ms[2]; c->timing.ms_seq += ms[3];
    c->timing.ms_pack += ms[4] + ms[5];
    for (size_t i = 0; i + 1 < c->lzm_used; i += 2) { float m = 0; (void)hipEventElapsedTime(&m, c->lzm_ev[i], c->lzm_ev[i + 1]); c->timing.ms_lz_match += m; c->timing.lz_match_launches += i / 2 < c->lzm_nl.size() ? c->lzm_nl[i / 2] : 1u; }
    c->timing.n_segments += nseg; c->timing.n_blocks += nblk;
    return PNA_OK;
}

// ---- One sub-batch, in stages (run_subbatch below is their driver): plan -> compress -> prefixes -> layout (device, or host after a wait for the
// segment sizes) -> write + carry + spread -> cipher -> frame + offsets + timing.
// The arguments of one run_subbatch call, which every stage reads
struct SubBatch { pna_gpu_ctx *c; int algo; const uint8_t *d_src; const uint64_t *src_off, *src_len; size_t e0, e1;
                  uint8_t *d_dst; size_t dst_cap; uint64_t out_base; uint64_t *dst_off; hipStream_t st; bool timed; const FrameJob *fj; };
// option trace: the HOST's time line of the sub-batch (what it does before and next to the kernels), printed when the call ends
struct HostMarks {
    bool on; std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    std::vector<std::pair<const char *, double>> marks;
    void mark(const char *what) { if (on) marks.emplace_back(what, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count()); }
    void print(size_t ne) const { if (on && !marks.empty()) { fprintf(stderr, "[pna sub-batch] %zu entries, host:", ne); for (auto &m : marks) fprintf(stderr, "  %s %.2f", m.first, m.second); fprintf(stderr, " ms\n"); } }
};
// LATENCY MODE: a small batch -- the CompressionWriter seam with a handful of writers in flight, one entry of
// `pna_gpu_compress_batch` -- has fewer segments than the chip has CUs, and its time is the length of the per-segment and per-block serial
// chains (one workgroup walks a segment's 256 tiles; one lane codes a block's sequences).  Such a batch is cut finer: blocks of 8 .. 64 KiB
// inside the same frames (blk_log), and the LZ stage runs one workgroup per UNIT of 1 << unit_log bytes whose table is pre-warmed with
// everything before it (lz_prewarm), which gives the very matches of the segment-long walk.  Both follow from the batch's size alone
// (and pna_gpu_set_option), are reported by pna_gpu_last_timing, and are parameters of the oracle's model.
static void plan_geometry(const pna_gpu_ctx *c, int algo, uint64_t in_total, uint64_t nseg_est, SubPlan &p) {
    const bool latency = c->tun.latency_max_mib > 0 && in_total <= ((uint64_t)c->tun.latency_max_mib << 20) && nseg_est <= 1024 && !(c->call_flags & INIT_DIAG_STAMP);
    uint32_t blk_log = blk_log_for_longest(c, p.max_len), unit_log = 20;
    if (algo == PNA_ALGO_XZ) {
        // xz: an LZ block is an LZMA2 chunk, 64 KiB at most (a shorter longest entry: the power of two that holds it), and a chunk is one wave's serial chain.  In
        // latency mode the blocks are zstd's there -- 16 KiB up to 32 MiB of input, 32 KiB beyond --, a quarter or half of the chain for a model that starts anew
        // more often.  Whole segments always: the LZ stage's units are not used, the coder behind it is what an xz call waits for.
        if (latency && blk_log == 16 && !c->tun.blk_log) blk_log = std::max<uint64_t>(in_total, c->call_total) <= (32ull << 20) ? 14u : 15u;
    } else if (blk_log == PNA_BLK_LOG && algo != PNA_ALGO_ZSTD && c->tun.latency_max_mib > 0 && !(c->call_flags & INIT_DIAG_STAMP) && !(latency && in_total <= (64ull << 20))) {
        // deflate beyond 64 MiB of input: whole segments, and 64 KiB blocks up to 384 MiB of the call's input (96 / 192 / 256 MiB: 1.78 / 2.19 / 2.52 -> 1.66 / 1.99 / 2.20 ms;
        // ratio 2.540 -> 2.536: every dynamic block repeats the code description, so the blocks stay larger than zstd's)
        if (std::max<uint64_t>(in_total, c->call_total) <= (384ull << 20)) blk_log = 16;
    } else if (latency && blk_log == PNA_BLK_LOG && algo != PNA_ALGO_ZSTD) {
        // blocks: 16 KiB up to 16 MiB of input (a block's sequence chain then is ~1 000 steps), then growing with the batch so that the
        // block count -- per-block fixed costs of the entropy kernels -- stays near 1 024 .. 2 048
        blk_log = 14;
        while (blk_log < PNA_BLK_LOG && (in_total >> blk_log) > 2048) blk_log++;
        // units: about one per CU (256), never smaller than a block
        unit_log = blk_log;
        while (unit_log < 20 && (in_total >> unit_log) > 384) unit_log++;
    } else if (blk_log == PNA_BLK_LOG && algo == PNA_ALGO_ZSTD && c->tun.latency_max_mib > 0 && !(c->call_flags & INIT_DIAG_STAMP)) {       // (latency_max_mib = 0: 128 KiB blocks whatever the batch)
        // zstd, measured again on the round's final kernels (LAB_LOG.md 4.10: one device batch of n x 1 MiB): what a batch below ~1 GiB costs is its blocks' chains, so
        // the blocks stay small well beyond the latency mode -- 16 KiB up to 32 MiB of input, 32 KiB up to 384 MiB, 64 KiB up to 1 GiB (256 MiB: 3.3 -> 2.5 ms, 512: 5.2 -> 4.6;
        // ratio 2.847 -> 2.844 / 2.846), the call's whole input deciding where a large call is cut into sub-batches --, and UNITS pay only while they fit ONE round of
        // the chip's CUs (every unit replays the packed table's walk up to its start): up to 64 MiB of input; beyond, whole segments (80 MiB: 2.55 -> 2.0 ms)
        const uint64_t sz = std::max<uint64_t>(in_total, c->call_total);
        blk_log = sz <= (32ull << 20) ? 14u : (sz <= (384ull << 20) ? 15u : (sz <= (1ull << 30) ? 16u : (uint32_t)PNA_BLK_LOG));
        if (latency && in_total <= (64ull << 20)) {
            unit_log = blk_log;
            while (unit_log < 20 && (in_total >> unit_log) > c->n_cus) unit_log++;
        }
    }
    if (c->tun.unit_log) unit_log = (uint32_t)std::max<long>(c->tun.unit_log, blk_log);
    // option mtile: whole segments -- a unit's pre-warm (lz_prewarm / lz_prewarm3) replays a tile's inserts as ONE contest, which is not what sub-tiles leave in the table
    if (c->tun.mtile && !(algo == PNA_ALGO_ZSTD && c->lz.gtab)) unit_log = 20;
    if (unit_log < blk_log) unit_log = blk_log;
    p.latency = latency; p.blk_log = blk_log; p.unit_log = unit_log;
}
// The plan: the geometry, then the segment, unit, block -> segment and entry -> first segment tables, counted first and then written straight into
// the page-locked blob that travels to the device in one copy (several threads for the batches of 10^5 .. 10^6 small entries, where these loops are a
// tenth of the call), the workspace for the kernels.  A sub-batch without segments leaves p.nseg = 0 and queues nothing.
static int plan_subbatch(const SubBatch &sb, HostMarks &hm, SubPlan &p) {
    pna_gpu_ctx *c = sb.c; const int algo = sb.algo; const FrameJob *fj = sb.fj;
    const uint64_t *src_off = sb.src_off, *src_len = sb.src_len; const size_t e0 = sb.e0, ne_all = sb.e1 - sb.e0;
    const unsigned host_nt = host_loop_threads(ne_all);
    struct PlanPart { uint64_t in_total = 0, nseg_est = 0, max_len = 0, n_short = 0, n_mid = 0, max_mid = 0; uint32_t sg = 0, bk = 0, un = 0; bool misaligned = false, any_empty = false; };
    std::vector<PlanPart> pp(host_nt);
    // an entry that is not a file (FrameJob::recs) is no frame at all: no segment, no block, its source offset unread -- an EMPTY FILE is one empty frame (any_empty)
    const EntryRecords *recs = fj ? fj->recs : nullptr;
    par_ranges(ne_all, host_nt, [&](unsigned t, size_t a, size_t b) {
        PlanPart q;
        for (size_t e = e0 + a; e < e0 + b; e++) {
            if (recs && recs->len(e)) continue;
            const uint64_t len = src_len[e];
            q.in_total += len; q.nseg_est += len ? (len + SEG_SIZE - 1) / SEG_SIZE : 1; q.max_len = std::max<uint64_t>(q.max_len, len);
            q.misaligned |= (src_off[e] & 15) != 0; q.any_empty |= len == 0;
            // SHORT segments (pna_dev.h SMALL_SEG): an entry of at most that many bytes, or the last segment of a longer one
            const uint64_t last = len ? ((len - 1) & (SEG_SIZE - 1)) + 1 : 0;
            q.n_short += (last > 0 && last <= SMALL_SEG) ? 1u : 0u; if (last > SMALL_SEG && last <= MID_SEG) { q.n_mid++; q.max_mid = std::max(q.max_mid, last); }
        }
        pp[t] = q;
    });
    uint64_t in_total = 0, nseg_est = 0, max_len = 0, n_short = 0, n_mid = 0, max_mid = 0;
    bool any_empty = false;
    for (const PlanPart &q : pp) {
        in_total += q.in_total; nseg_est += q.nseg_est; max_len = std::max(max_len, q.max_len); any_empty |= q.any_empty; n_short += q.n_short; n_mid += q.n_mid; max_mid = std::max(max_mid, q.max_mid);
        if (q.misaligned) return fail(c, PNA_E_INVAL, "entry offset not 16-byte aligned");
    }
    if (fj && fj->stream_len) {
        // one window of a solid stream: block size, latency form and units follow from the whole stream, as in its one-shot run, so that the window's
        // segments are coded as they are there (a window is whole segments: the short ones are the stream's own)
        in_total = fj->stream_len; nseg_est = (in_total + SEG_SIZE - 1) / SEG_SIZE; max_len = in_total;
    }
    p.max_len = max_len; p.any_empty = any_empty;
    p.frame_max_payload = (fj && !fj->solid && !fj->cipher && max_len <= 16384) ? (uint32_t)std::min<size_t>(pna_gpu_bound(algo, (size_t)max_len), 0xFFFFFFFFu) : 0u;
    plan_geometry(c, algo, in_total, nseg_est, p);
    const uint32_t blk_log = p.blk_log, unit_log = p.unit_log, bsz = 1u << blk_log;
    // first segment / block / unit of every range of entries (the ranges of par_ranges): counted per range, then a prefix sum over the ranges
    par_ranges(ne_all, host_nt, [&](unsigned t, size_t a, size_t b) {
        uint32_t sg = 0, bk = 0, un = 0;
        for (size_t e = e0 + a; e < e0 + b; e++) {
            const uint64_t len = src_len[e];
            if (len == 0) { if (!(recs && recs->len(e))) sg++; continue; }
            const uint64_t full = len >> 20, rest = len & (SEG_SIZE - 1);
            sg += (uint32_t)(full + (rest ? 1 : 0));
            bk += (uint32_t)((full << (20 - blk_log)) + ((rest + bsz - 1) >> blk_log));
            if (unit_log < 20) un += (uint32_t)((full << (20 - unit_log)) + ((rest + (1u << unit_log) - 1) >> unit_log));
        }
        pp[t].sg = sg; pp[t].bk = bk; pp[t].un = un;
    });
    uint32_t nseg = 0, nblk = 0, nunits = 0;
    for (PlanPart &q : pp) { const uint32_t a = q.sg, b = q.bk, u = q.un; q.sg = nseg; q.bk = nblk; q.un = nunits; nseg += a; nblk += b; nunits += u; }
    if (nseg == 0) return PNA_OK;
    hm.mark("counted");
    // Layout of the blob: [segs | units | blk_seg | entry_first_seg]
    const size_t o_units = ((size_t)nseg * sizeof(SegDesc) + 15) & ~(size_t)15, o_blkseg = (o_units + (size_t)nunits * sizeof(SegDesc) + 15) & ~(size_t)15,
                 o_entry = (o_blkseg + (size_t)(nblk + 1) * 4 + 15) & ~(size_t)15, plan_bytes = o_entry + (ne_all + 2) * 4;
    if (c->plan.ensure(plan_bytes) || c->h_plan.ensure(plan_bytes)) return fail(c, PNA_E_NOMEM, "workspace allocation failed");
    SegDesc *segs = (SegDesc *)c->h_plan.p, *units = (SegDesc *)((uint8_t *)c->h_plan.p + o_units);   // (the previous sub-batch has been waited for: the staging is free)
    c->tail_used = 0;
    uint32_t *blk_seg = (uint32_t *)((uint8_t *)c->h_plan.p + o_blkseg), *entry_first_seg = (uint32_t *)((uint8_t *)c->h_plan.p + o_entry);
    // option single_frame (zstd): an entry's segments form ONE frame -- the frame header in front of the first segment only, the last-block bit on the entry's
    // last block only (SegDesc::first bit 2 tells k_plan / k_write); the blocks are what they are in the frame-per-segment form
    const uint32_t sf_bit = (algo == PNA_ALGO_ZSTD && c->tun.single_frame) ? 4u : 0u;
    // a window of a deflate stream (FrameJob::run): its first segment starts the stream only in the first window, its last one ends it only in the last
    const uint32_t first_bit = (fj && (fj->run & DRUN_CONT)) ? 0u : 1u, last_bit = (fj && (fj->run & DRUN_OPEN)) ? 0u : 2u;
    par_ranges(ne_all, host_nt, [&](unsigned t, size_t a, size_t b) {
        uint32_t sg = pp[t].sg, bk = pp[t].bk, un = pp[t].un;
        for (size_t e = e0 + a; e < e0 + b; e++) {
            entry_first_seg[e - e0] = sg;
            const uint64_t len = src_len[e], off = src_off[e];
            if (recs && recs->len(e)) continue;
            if (len == 0) { segs[sg++] = SegDesc{off, 0, bk, (uint32_t)e, 3, 0, 0, blk_log, 0}; continue; }
            for (uint64_t q = 0; q < len; q += SEG_SIZE) {
                const uint32_t sl = (uint32_t)std::min<uint64_t>(SEG_SIZE, len - q);
                const SegDesc s{off + q, sl, bk, (uint32_t)e, (q == 0 ? first_bit : 0u) | (q + SEG_SIZE >= len ? last_bit : 0u) | sf_bit, 0, sl, blk_log, 0};
                const uint32_t nb = (sl + bsz - 1) >> blk_log;
                for (uint32_t b2 = 0; b2 < nb; b2++) blk_seg[bk + b2] = sg;
                bk += nb; segs[sg++] = s;
                if (unit_log < 20)
                    for (uint32_t u = 0; u < sl; u += 1u << unit_log) { SegDesc us = s; us.u0 = u; us.u1 = std::min<uint32_t>(sl, u + (1u << unit_log)); units[un++] = us; }
            }
        }
    });
    entry_first_seg[ne_all] = nseg;
    const bool unit_mode = unit_log < 20 && nunits > 0;
    c->last_blk_log = blk_log; c->last_units = unit_mode ? nunits : 0;
    // zstd entropy stage, two forms: statistics per block (k_hist) + tables + three-lane state chains (k_seqa) + token-parallel packing (k_seqb) while
    // the chain waves fit the chip's SIMDs (<= 40 960 blocks); beyond, statistics per segment inside k_stats and the one-kernel coder k_seq.  The init
    // diagnostics INIT_DIAG_SEQ_ONE / INIT_DIAG_SEQ_TWO and option hist_by_block force one.
    // (batches whose segments hold one block each -- entries of at most a block --: statistics per segment and the sequence coder with a lane per segment)
    const bool single_block = max_len <= bsz;
    const bool hist_on = algo == PNA_ALGO_ZSTD && !(c->call_flags & INIT_DIAG_SEQ_ONE) && !single_block &&
                         ((c->call_flags & INIT_DIAG_SEQ_TWO) || (c->tun.hist_by_block < 0 ? nblk <= 40960u : c->tun.hist_by_block != 0));
    // round 5: large zstd batches behind the split LZ stage -- the parse kernel counts the sequence codes per block into the segments' counters, k_stats walks the literals only
    const bool seq_hist = algo == PNA_ALGO_ZSTD && !hist_on && !single_block && c->tun.seq_hist != 0;
    const size_t o_hist = ((size_t)(nblk + 1) * sizeof(BlkInfo) + 15) & ~(size_t)15, blk_bytes = o_hist + ((hist_on || seq_hist) ? (size_t)nseg * 448 * 4 : 0);
    if (c->blk.ensure(blk_bytes) || c->tabs.ensure((size_t)nseg * std::max(sizeof(SegTables), sizeof(DeflTables))) ||
        (algo == PNA_ALGO_DEFLATE && c->ctab.ensure(((size_t)(nblk + 1) << (blk_log - 11)) * 16)) ||
        c->seqs.ensure((size_t)(nblk + 1) * seq_cap_of(blk_log) * 8) || c->lits.ensure((size_t)(nblk + 1) << blk_log) ||
        c->litc.ensure((size_t)(nblk + 1) << blk_log) || (algo == PNA_ALGO_ZSTD && c->seqc.ensure((size_t)(nblk + 1) << blk_log)) ||
        (algo == PNA_ALGO_ZSTD && c->seqw.ensure(hist_on ? (size_t)(nblk + 1) * seq_cap_of(blk_log) * 8 : 64)) ||
        c->seg_size.ensure((size_t)nseg * 8) || c->seg_off.ensure(((size_t)nseg + 1 + 2 * ((size_t)nseg / 4096 + 2)) * 8)) {     // (+ the scratch of the hierarchical scan)
        if (!c->call_xz) return fail(c, PNA_E_NOMEM, "workspace allocation failed");
        // xz: the sub-batch cannot be made smaller than its longest entry (the entry's Index is sized over all its blocks), so name that limit
        char msg[256];
        snprintf(msg, sizeof msg, "workspace allocation failed: an xz entry must fit one sub-batch -- this one holds %llu input bytes (longest entry %llu) and needs about %llu bytes of device workspace",
                 (unsigned long long)in_total, (unsigned long long)max_len, (unsigned long long)((size_t)(nblk + 1) * (seq_cap_of(blk_log) * 8 + (2ull << blk_log))));
        return fail(c, PNA_E_NOMEM, msg);
    }
    uint8_t *hp = (uint8_t *)c->h_plan.p, *dp = (uint8_t *)c->plan.p;
    c->d_segs = (SegDesc *)dp; c->d_units = (SegDesc *)(dp + o_units); c->d_blk_seg = (uint32_t *)(dp + o_blkseg); c->d_entry_seg = (uint32_t *)(dp + o_entry);
    c->d_hist = (uint32_t *)((uint8_t *)c->blk.p + o_hist);
    HIPCHK(c, hipMemcpyAsync(dp, hp, plan_bytes, hipMemcpyHostToDevice, sb.st));
    HIPCHK(c, hipMemsetAsync(c->blk.p, 0, blk_bytes, sb.st));                     // BlkInfo of every block and, behind them, the segments' histogram counters
    // the short segments' geometry (k_lzms): a launch flag tells the large geometry's kernels to skip them; a sub-batch of short segments only launches none of those
    p.small_fl = (c->tun.small_geometry && (n_short || n_mid))
        ? (FLAG_HAS_SMALL | (n_short ? FLAG_TIER1 : 0u) | (n_mid ? FLAG_TIER2 | ((max_mid <= 8192 ? 0u : (max_mid <= 12288 ? 1u : 2u)) << FLAG_T2_SHIFT) : 0u) | (max_len <= MID_SEG ? FLAG_ALL_SMALL : 0u)) : 0u;
    p.nseg = nseg; p.nblk = nblk; p.nunits = nunits; p.unit_mode = unit_mode; p.single_block = single_block; p.hist_on = hist_on; p.seq_hist = seq_hist;
    p.wave_blk = max_len <= 32768 && nseg >= 4096;
    p.segs = segs; p.entry_first_seg = entry_first_seg;
    return PNA_OK;
}
// The kernel chains of the codec: LZ stage, then deflate's stage 1 (codes, sizes, offsets) or zstd's entropy stage and k_plan -- every segment's
// compressed size and offset in c->seg_size / c->seg_off.
static int compress_subbatch(const SubBatch &sb, const SubPlan &p) {
    pna_gpu_ctx *c = sb.c; const uint8_t *d_src = sb.d_src; const hipStream_t st = sb.st; const bool timed = sb.timed;
    const uint32_t nseg = p.nseg, nblk = p.nblk, blk_log = p.blk_log;
    const bool defl = sb.algo == PNA_ALGO_DEFLATE;
    if (timed) HIPCHK(c, hipEventRecord(c->ev[0], st));
    if (!defl) {
        // zstd (and xz, whose LZ stage is zstd's with matches of at most 273 bytes): everything stays on `st` -- a hand-over to the auxiliary stream and back costs ~45 us of idle device, a tenth of a small batch --, except the
        // literal coder of large batches, which runs on the auxiliary stream next to the sequence coder (option lit_beside_seq)
        if (!c->aux) {
            { int lo = 0, hi = 0; (void)hipDeviceGetStreamPriorityRange(&lo, &hi);      // (lowest priority: what runs here fills in beside the main stream's kernels)
              HIPCHK(c, hipStreamCreateWithPriority(&c->aux, hipStreamNonBlocking, lo)); }
            for (auto &e : c->ev_lz) HIPCHK(c, hipEventCreate(&e));
            for (auto &e : c->ev_en) HIPCHK(c, hipEventCreate(&e));
            HIPCHK(c, hipEventCreateWithFlags(&c->ev_join, hipEventDisableTiming));
            HIPCHK(c, hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming));
        }
        HIPCHK(c, hipEventRecord(c->ev_lz[0], st));
    }
    { const int rc = lz_run(c, sb.algo, d_src, p, st, timed); if (rc) return rc; }       // the LZ stage, every codec and form (pna_lz.cpp)
    if (defl) {
        if (timed) HIPCHK(c, hipEventRecord(c->ev[1], st));
        launch_deflate_stage1(d_src, c->d_segs, nseg, c->d_blk_seg, nblk, (const uint64_t *)c->seqs.p,
                              (const uint8_t *)c->lits.p, (BlkInfo *)c->blk.p, (const uint4 *)c->ctab.p, (DeflTables *)c->tabs.p, (uint8_t *)c->litc.p,
                              (uint64_t *)c->seg_size.p, (uint64_t *)c->seg_off.p, st, timed ? &c->ev[2] : nullptr, c->call_flags, c->call_stored,
                              /* a wave per segment: many small entries */ p.wave_blk);
    } else {
        const bool xz = sb.algo == PNA_ALGO_XZ;
        HIPCHK(c, hipEventRecord(c->ev_lz[1], st));
        HIPCHK(c, hipEventRecord(c->ev_en[0], st));
        if (xz) {
            // xz: the segments' CRC64 (timed as the statistics stage), the chunk coder (as the literal stage), sizes and offsets (as the sequence stage); the scratch is the literal
            // coder's (a slot of the block's size per block), the sizes and accumulators live where the zstd tables would
            launch_xzenc_stage(d_src, c->d_segs, nseg, (uint32_t)std::min<uint64_t>(p.max_len, SEG_SIZE), c->d_blk_seg, nblk, (const uint64_t *)c->seqs.p, (BlkInfo *)c->blk.p, (uint8_t *)c->litc.p, (uint64_t *)c->tabs.p,
                               (uint64_t *)c->seg_size.p, (uint64_t *)c->seg_off.p, st, &c->ev_en[1]);
            if (timed) { HIPCHK(c, hipEventRecord(c->ev[4], st)); HIPCHK(c, hipEventRecord(c->ev[5], st)); }
            HIPCHK(c, hipGetLastError());
            return PNA_OK;
        }
        launch_entropy_chunk(c->d_segs, 0, nseg, c->d_blk_seg, 0, nblk, (const uint64_t *)c->seqs.p,
                             (const uint8_t *)c->lits.p, (BlkInfo *)c->blk.p, (SegTables *)c->tabs.p, (uint8_t *)c->litc.p, (uint8_t *)c->seqc.p,
                             (uint32_t *)c->seqw.p, c->call_flags, blk_log, p.hist_on ? c->d_hist : nullptr, st, &c->ev_en[1],
                             c->tun.lit_beside_seq ? c->aux : nullptr, c->ev_fork, c->ev_join, p.single_block, c->lzp_hist_all ? c->d_hist : nullptr);
        if (timed) HIPCHK(c, hipEventRecord(c->ev[4], st));
        launch_plan(c->d_segs, nseg, (BlkInfo *)c->blk.p, (const SegTables *)c->tabs.p, (uint64_t *)c->seg_size.p,
                    (uint64_t *)c->seg_off.p, c->call_flags, st);
        if (timed) HIPCHK(c, hipEventRecord(c->ev[5], st));
    }
    HIPCHK(c, hipGetLastError());
    return PNA_OK;
}
// The framing of a sub-batch as the host lays it out: descriptors and prefixes for k_frame in the page-locked staging (c->h_desc, h_blob, h_segdst),
// and what the cipher stage and the spread of entries of several FDAT chunks / GCM segments need
struct SubLayout {
    FrameDesc *fds = nullptr; uint8_t *blob = nullptr; uint64_t *segdst = nullptr; size_t blob_len = 0;
    size_t nunit = 0;                                        // framed units: entries, FDAT chunks, or the SDAT chunks of the solid stream
    uint64_t layout_need = 0; bool layout_over = false;      // the sub-batch's worst-case size with its prefixes; an entry whose worst case exceeds one FDAT chunk
    uint64_t total = 0;                                      // archive bytes of the sub-batch
    std::vector<GcmMaterial> gmat; std::vector<GcmEntry> gents;
    // GCM STREAM segments of this sub-batch, in order (an entry has ceil(payload / segment_size) of them, at least one): counter-mode IV
    // (nonce || 2) and the round keys of the stream they belong to; `spread`: pieces of the compact payload that move to their place between the tags
    std::vector<uint8_t> giv; SegKeys gkeys;
    struct SpreadPiece { uint64_t src, dst; uint32_t len; };
    std::vector<SpreadPiece> spread; uint64_t spread_bytes = 0;
    std::vector<std::pair<uint64_t, uint64_t>> spread_copy;     // (archive offset, length) of the compact payloads to save first
    std::vector<CipherUnit> cunits;
    uint64_t carry_in = 0, carry_in_len = 0, carry_out = 0;     // windowed GCM: where the carry goes in / the next one starts (0: none)
    // bytes [from, from + len) of the compact payload being laid out move to `dst`, in pieces of at most 1 MiB
    void move(uint64_t from, uint64_t dst, uint64_t len) {
        for (uint64_t o = 0; o < len; o += (1u << 20)) spread.push_back(SpreadPiece{spread_bytes + from + o, dst + o, (uint32_t)std::min<uint64_t>(1u << 20, len - o)});
    }
    // ... which is saved first: the `len` bytes at archive offset `at` (the pieces of the next payload come from behind it)
    void save(uint64_t at, uint64_t len) { spread_copy.emplace_back(at, len); spread_bytes += (len + 15) & ~(uint64_t)15; }
    // GCM STREAM segments first .. first + K - 1 of a stream (GcmEncryptWriter, lib/src/cipher/gcm.rs:48-100): `plen` compact payload bytes from archive
    // offset `base` on, cut into segments of G bytes (the last one the rest); segment k goes to base + k * stride, its tag behind it, and only the stream's
    // last segment -- the last of these if `final_last` -- carries nonce flag 1.  Appends every segment's counter IV, CTR units and tag descriptor and, for
    // K > 1, the spread that moves segments k >= 1 to their places.
    void gcm_segments(const GcmMaterial &gm, uint64_t first, uint64_t K, bool final_last, uint64_t plen, uint64_t G, uint64_t base, uint64_t stride) {
        for (uint64_t k = 0; k < K; k++) {
            const uint64_t sl = std::min<uint64_t>(G, plen - k * G), so = base + k * stride, q = first + k;     // q: the segment's counter in the stream
            const uint32_t si = (uint32_t)(giv.size() / 16);
            GcmEntry ge{so, (uint32_t)sl, 0, {0, 0, 0, 0}, {0, 0, 0, 0}};
            uint8_t iv[16];
            gcm_segment(gm, (uint32_t)q, final_last && k + 1 == K, ge, iv);
            giv.insert(giv.end(), iv, iv + 16);
            gkeys.push(si, gm.key);
            for (uint64_t o = 0; o < sl; o += CTR_UNIT) cunits.push_back(CipherUnit{so + o, o, (uint32_t)std::min<uint64_t>(CTR_UNIT, sl - o), si});
            gents.push_back(ge);
            if (k >= 1) move(k * G, so, sl);
        }
        if (K > 1) save(base, std::min(plen, K * G));
    }
};
// While the kernels run: the staging of the framing and the name-dependent part of every entry record (FHED and fSIZ chunks with their CRCs); GCM
// STREAM: every stream's key material.
static int frame_prefixes(const SubBatch &sb, const SubPlan &p, SubLayout &L) {
    pna_gpu_ctx *c = sb.c; const int algo = sb.algo; const FrameJob *fj = sb.fj; const uint64_t *src_len = sb.src_len; const size_t e0 = sb.e0, e1 = sb.e1;
    const bool gcm = fj->cipher && fj->cipher->cipher_mode == PNA_MODE_GCM;
    const uint32_t gcm_seg = gcm ? gcm_seg_size(fj->cipher) : 0u;
    if (fj->solid) {
        if (e1 - e0 != 1) return fail(c, PNA_E_INVAL, "a solid stream is one entry");
        L.nunit = p.nseg;
        // (GCM: one SDAT chunk per GCM segment of the compressed stream -- at most the worst-case output / segment size + 1 of them)
        const uint64_t carry_in = fj->crun ? fj->crun->carry_len : 0;
        const size_t ucap = gcm ? (size_t)((pna_gpu_bound(algo, (size_t)src_len[e0]) + carry_in) / gcm_seg) + 2 : L.nunit;
        if (c->h_desc.ensure(ucap * sizeof(FrameDesc)) || c->h_blob.ensure(ucap * 8 + 16) || c->h_segdst.ensure((size_t)(p.nseg + 1) * 8))
            return fail(c, PNA_E_NOMEM, "framing staging");
        L.fds = (FrameDesc *)c->h_desc.p; L.blob = (uint8_t *)c->h_blob.p; L.segdst = (uint64_t *)c->h_segdst.p;
        if (gcm) { L.gmat.resize(1); gcm_solid_material(fj->cipher, fj->ivs, algo, L.gmat[0]); }
        return PNA_OK;
    }
    const size_t ne_all = e1 - e0;
    const unsigned host_nt = host_loop_threads(ne_all);
    L.nunit = ne_all;
    // bounds, one pass over the entries on the host-loop threads: the prefixes' worst case per range of entries (a range's prefixes are written
    // from its bound offset on, so the ranges need no compaction pass afterwards), the extra FDAT chunks (every chunk behind an entry's first needs a
    // descriptor and 8 prefix bytes: at most one per max_chunk_size bytes of the worst-case output), and what the device-side layout must know --
    // whether every worst-case payload fits one chunk, and the worst-case size of the sub-batch
    struct FramePart { size_t bound = 0, extra = 0; uint64_t need = 0; bool over = false; };
    std::vector<FramePart> fp(host_nt);
    const uint64_t CHb = chunk_limit(fj->max_chunk);
    // an entry that is not a file: its finished record is its prefix and all of it -- a descriptor "without a data chunk" (FrameDesc::pad bit 0), which k_frame copies
    // and leaves alone: no data CRC, no FEND (the record has both); no stream key, no cipher unit
    const EntryRecords *recs = fj->recs;
    auto record_desc = [&](size_t e, size_t at) { const size_t rl = (size_t)recs->len(e); memcpy(L.blob + at, recs->at(e), rl); return FrameDesc{0, 0, (uint32_t)at, (uint32_t)rl, 1u}; };
    par_ranges(ne_all, host_nt, [&](unsigned t, size_t a, size_t b) {
        FramePart q;
        for (size_t e = e0 + a; e < e0 + b; e++) {
            if (recs && recs->len(e)) { q.bound += (size_t)recs->len(e); q.need += recs->len(e); continue; }
            const size_t pb = (fj->cipher ? frame_entry_prefix_enc_bound(fj->names[e], fj->cipher->phsf) : frame_entry_prefix_bound(fj->names[e])) + meta_len(fj->meta, e);
            const uint64_t wb = pna_gpu_bound(algo, (size_t)src_len[e]);
            q.bound += pb; q.extra += (size_t)((wb + 64 + 16 * (src_len[e] >> 12)) / CHb); q.need += pb + wb + 16; q.over |= wb > CHb;
        }
        fp[t] = q;
    });
    size_t bound = 0, extra_chunks = 0;
    for (FramePart &q : fp) { const size_t bq = q.bound; q.bound = bound; bound += bq; extra_chunks += q.extra; L.layout_need += q.need; L.layout_over |= q.over; }
    if (c->h_desc.ensure((ne_all + extra_chunks + 1) * sizeof(FrameDesc)) || c->h_blob.ensure(bound + 8 * extra_chunks + 16) || c->h_segdst.ensure((size_t)(p.nseg + 1) * 8))
        return fail(c, PNA_E_NOMEM, "framing staging");
    FrameDesc *fds = L.fds = (FrameDesc *)c->h_desc.p; uint8_t *blob = L.blob = (uint8_t *)c->h_blob.p; L.segdst = (uint64_t *)c->h_segdst.p;
    if (gcm) {
        // GCM STREAM: per entry a stream header, an HKDF stream key bound to its FHED chunk, round keys, hash subkey, E(K, J0);
        // a few host threads share the entries (SHA-256 / HKDF / key schedule: a few microseconds each) while k_lz runs
        L.gmat.resize(ne_all);
        const GcmCallKeys keys = gcm_call_keys(fj->cipher->key, fj->cipher->phsf, strlen(fj->cipher->phsf));
        const unsigned nt = (unsigned)std::min<size_t>(8, std::max<size_t>(1, ne_all / 256));
        std::vector<std::thread> th;
        for (unsigned t = 0; t < nt; t++)
            th.emplace_back([&, t]() {
                for (size_t e = e0 + t; e < e1; e += nt)
                    if (!(recs && recs->len(e))) gcm_entry_material(fj->cipher, keys, fj->ivs + 39 * e, gcm_seg, fj->names[e], algo, L.gmat[e - e0]);
            });
        for (auto &x : th) x.join();
    }
    if (!fj->cipher && !fj->meta) {
        // plain entries: the prefixes are written straight into the staging blob, every range of entries back to back from the range's bound offset
        // (the few unused bytes between two ranges travel with the blob; nothing refers to them)
        par_ranges(ne_all, host_nt, [&](unsigned t, size_t a, size_t b) {
            size_t at = fp[t].bound;
            for (size_t i = a; i < b; i++) {
                if (recs && recs->len(e0 + i)) { fds[i] = record_desc(e0 + i, at); at += fds[i].prefix_len; continue; }
                const size_t pl = frame_entry_prefix_into(blob + at, fj->names[e0 + i], algo, src_len[e0 + i]);
                fds[i] = FrameDesc{0, 0, (uint32_t)at, (uint32_t)pl, 0};
                at += pl;
            }
        });
        L.blob_len = bound;
        return PNA_OK;
    }
    std::vector<uint8_t> tmp;
    for (size_t e = e0; e < e1; e++) {
        if (recs && recs->len(e)) { fds[e - e0] = record_desc(e, L.blob_len); L.blob_len += fds[e - e0].prefix_len; continue; }
        tmp.clear();
        if (gcm) frame_entry_prefix_enc(tmp, fj->names[e], algo, src_len[e], fj->cipher->encryption, PNA_MODE_GCM, fj->cipher->phsf, L.gmat[e - e0].header, 75);
        else if (fj->cipher) frame_entry_prefix_enc(tmp, fj->names[e], algo, src_len[e], fj->cipher->encryption, fj->cipher->cipher_mode, fj->cipher->phsf, fj->ivs + 16 * e, 16);
        else frame_entry_prefix(tmp, fj->names[e], algo, src_len[e], 0);
        splice_meta(tmp, fj->meta, e);
        memcpy(blob + L.blob_len, tmp.data(), tmp.size());
        fds[e - e0] = FrameDesc{0, 0, (uint32_t)L.blob_len, (uint32_t)tmp.size(), 0};
        L.blob_len += tmp.size();
    }
    return PNA_OK;
}
// The host layout of a solid stream (seg_off: the segment offsets, waited for): one SDAT chunk per segment (= per zstd frame / per run of deflate
// blocks): [len "SDAT" | payload | crc]; with GCM one per GCM segment.  `pos`: where the stream's chunks start, then where they end.
static int layout_solid(const SubBatch &sb, const SubPlan &p, const uint64_t *seg_off, SubLayout &L, uint64_t &pos) {
    pna_gpu_ctx *c = sb.c; const FrameJob *fj = sb.fj; const uint32_t nseg = p.nseg;
    auto sdat = [&](size_t k, uint64_t at, uint64_t cl) {           // the header of SDAT chunk k at archive offset `at`, `cl` bytes of data
        uint8_t *pf = L.blob + 8 * k;
        put_be32(pf, cl);
        memcpy(pf + 4, "SDAT", 4);
        L.fds[k] = FrameDesc{at, (uint32_t)cl, (uint32_t)(8 * k), 8u, 0};
    };
    sb.dst_off[sb.e0] = pos;
    if (!fj->cipher || fj->cipher->cipher_mode != PNA_MODE_GCM) {
        const uint64_t ctr_base = fj->crun ? fj->crun->pos : 0;
        for (uint32_t sg = 0; sg < nseg; sg++) {
            const uint64_t plen = seg_off[sg + 1] - seg_off[sg];
            sdat(sg, pos, plen);
            L.segdst[sg] = pos + 8;
            if (fj->cipher)                                    // one cipher stream over all SDAT bodies: the keystream position runs on (over windows too)
                for (uint64_t o = 0; o < plen; o += CTR_UNIT)
                    L.cunits.push_back(CipherUnit{pos + 8 + o, ctr_base + (seg_off[sg] - seg_off[0]) + o, (uint32_t)std::min<uint64_t>(CTR_UNIT, plen - o), 0u});
            pos += 8 + plen + 4;
        }
        L.blob_len = 8 * (size_t)nseg;
        if (fj->crun) fj->crun->pos += seg_off[nseg] - seg_off[0];
        return PNA_OK;
    }
    // GCM STREAM over the solid stream (into_solid_archive takes any cipher, lib/src/archive/write.rs:443-470; GcmEncryptWriter, lib/src/cipher/
    // gcm.rs:48-100): the head carries the stream header as its first SDAT chunk; here one SDAT chunk per GCM segment, ciphertext || tag.  The
    // write kernels put the compressed stream down in one piece behind the first chunk header, segments k >= 1 then move forward by 28 k
    // bytes (tag and CRC of the chunk before + their own chunk header), as a GCM entry of several segments does.
    // A window of a windowed stream (fj->crun): the carry of the window before goes in front of the window's output, segment counters
    // start at crun->seg, and unless the window is the stream's last, the tail that does not yet form a non-final segment (1 .. G bytes)
    // is held back as the next carry.
    SolidCipherRun *cr = fj->crun;
    const uint64_t C = cr ? cr->carry_len : 0, P = C + seg_off[nseg] - seg_off[0], G = gcm_seg_size(fj->cipher), J = cr ? cr->seg : 0;
    const bool last = !cr || cr->final_win;
    const uint64_t K = last ? (P ? (P + G - 1) / G : (J ? 0 : 1)) : (P ? (P - 1) / G : 0);
    const uint64_t E = last ? P : K * G;                                 // the bytes that go out in this window's segments
    if (J + K > 0xFFFFFFFFull) return fail(c, PNA_E_INVAL, "GCM segment counter overflow");
    const uint64_t B = pos + 8;
    if (B + P + 16 > sb.dst_cap) return fail(c, PNA_E_DSTSIZE, "device destination too small");      // (the compact stream, carry included)
    for (uint32_t sg = 0; sg < nseg; sg++) L.segdst[sg] = B + C + (seg_off[sg] - seg_off[0]);
    if (C) { L.carry_in = B; L.carry_in_len = C; }
    if (P > E) L.carry_out = B + E;
    if (cr) { cr->seg = J + K; cr->carry_len = P - E; }
    for (uint64_t k = 0; k < K; k++) sdat((size_t)k, pos + k * (G + 28), std::min<uint64_t>(G, P - k * G) + 16);
    L.gcm_segments(L.gmat[0], J, K, last, P, G, B, G + 28);
    pos += E + 28 * K;
    L.nunit = (size_t)K; L.blob_len = 8 * (size_t)K;
    return PNA_OK;
}
// The host layout of file entries (seg_off: the segment offsets, waited for): [prefix | payload | crc | FEND] per entry; the write kernels put every
// segment straight at its final place, k_frame adds the rest (no second copy of the payload).
// FlattenWriter cuts an entry's stream into FDAT chunks of max_chunk_size bytes, the last one holding the rest (lib/src/util/io.rs:60-77:
// the open chunk is topped up before a new one starts; FileEntryBuilder::max_chunk_size, lib/src/entry/builder/file.rs:105-112; default
// u32::MAX, lib/src/chunk.rs:28).  The write kernels put an entry's payload down in one piece behind the first FDAT header; for an entry of
// K > 1 chunks the payload is saved to a scratch buffer and chunks 1 .. K - 1 move forward by 12 k bytes (CRC of the chunk before +
// their own length / type), k_frame then takes one descriptor per chunk.  The same pass serves the GCM STREAM layout below.
static int layout_entries(const SubBatch &sb, const SubPlan &p, const uint64_t *seg_off, SubLayout &L, uint64_t &pos) {
    pna_gpu_ctx *c = sb.c; const FrameJob *fj = sb.fj; const size_t e0 = sb.e0, e1 = sb.e1;
    const uint64_t CH = chunk_limit(fj->max_chunk);
    std::vector<FrameDesc> units; units.reserve(e1 - e0);
    const int mode = fj->cipher ? fj->cipher->cipher_mode : -1;
    const bool cbc = mode == PNA_MODE_CBC, gcm = mode == PNA_MODE_GCM, ctr = mode == PNA_MODE_CTR;
    const uint64_t G = gcm ? gcm_seg_size(fj->cipher) : 0;
    for (size_t e = e0; e < e1; e++) {
        const uint32_t s0 = p.entry_first_seg[e - e0], s1 = p.entry_first_seg[e - e0 + 1];
        const FrameDesc f0 = L.fds[e - e0];                // prefix of the entry: FHED | fSIZ | ... | first FDAT header
        sb.dst_off[e] = pos;
        if (f0.pad & 1) { FrameDesc u = f0; u.arc_off = pos; units.push_back(u); pos += f0.prefix_len; continue; }   // not a file: its prefix_len bytes and nothing else
        const uint64_t p0 = pos + f0.prefix_len;           // where the payload starts
        uint64_t plen = seg_off[s1] - seg_off[s0];         // the entry's compressed stream, then what the cipher makes of it
        for (uint32_t sg = s0; sg < s1; sg++) L.segdst[sg] = p0 + (seg_off[sg] - seg_off[s0]);
        if (cbc) {
            // CBC chains the whole entry (one lane) and appends the PKCS#7 padding block, in place
            L.cunits.push_back(CipherUnit{p0, 0, (uint32_t)plen, (uint32_t)(e - e0)});
            plen = (plen / 16 + 1) * 16;
            if (plen > CH) return fail(c, PNA_E_UNSUPPORTED, "CBC entry beyond one FDAT chunk");
        } else if (gcm) {
            // GCM STREAM: the payload in segments of segment_size bytes, every segment followed by its 16-byte tag; all but the last carry nonce
            // flag 0, the last one (possibly full, possibly empty) flag 1; counters 0, 1, ...  Segments k >= 1 move forward by 16 k bytes before the cipher runs.
            const uint64_t K = plen ? (plen + G - 1) / G : 1;
            if (K > 0xFFFFFFFFull) return fail(c, PNA_E_INVAL, "GCM segment counter overflow");
            if (plen + 16 * K > CH) return fail(c, PNA_E_UNSUPPORTED, "GCM entry beyond one FDAT chunk");
            L.gcm_segments(L.gmat[e - e0], 0, K, true, plen, G, p0, G + 16);
            plen += 16 * K;
        }
        // the FDAT chunks: CH bytes each, the last one the rest (an empty payload is one empty chunk)
        const uint64_t K = plen ? (plen + CH - 1) / CH : 1;
        for (uint64_t k = 0; k < K; k++) {
            const uint64_t cl = std::min<uint64_t>(CH, plen - k * CH), cstart = p0 + k * (CH + 12);   // the chunk's data in the archive
            FrameDesc u;
            if (k == 0) { u = f0; u.arc_off = pos; }
            else { u.prefix_off = (uint32_t)L.blob_len; u.prefix_len = 8; u.arc_off = cstart - 8; memcpy(L.blob + L.blob_len + 4, "FDAT", 4); L.blob_len += 8; }
            uint8_t *lenf = &L.blob[u.prefix_off + u.prefix_len - 8];  // FDAT chunk length, big-endian
            put_be32(lenf, cl);
            u.payload_len = (uint32_t)cl; u.pad = k + 1 < K ? 2u : 0u;
            units.push_back(u);
            if (k >= 1) L.move(k * CH, cstart, cl);
            if (ctr)                                       // CTR keeps the length and may be cut anywhere: the keystream position runs on over the chunks
                for (uint64_t o = 0; o < cl; o += CTR_UNIT)
                    L.cunits.push_back(CipherUnit{cstart + o, k * CH + o, (uint32_t)std::min<uint64_t>(CTR_UNIT, cl - o), (uint32_t)(e - e0)});
        }
        if (K > 1) L.save(p0, plen);
        pos += f0.prefix_len + plen + 12 * (K - 1) + 4 + 12;
    }
    L.nunit = units.size();
    memcpy(L.fds, units.data(), L.nunit * sizeof(FrameDesc));
    return PNA_OK;
}
// The write kernels: every segment's output at wbase + segdst[segment] (a deflate window of a solid stream: k_dwrite, then k_dfold); windowed GCM: the
// carry of the window before in front of their output, then the new carry out of it; entries of several FDAT chunks / GCM segments: the compact
// payloads saved, then the pieces behind the first one put at their places
static int write_stage(const SubBatch &sb, const SubPlan &p, const SubLayout &L, const uint64_t *d_segdst, uint8_t *wbase) {
    pna_gpu_ctx *c = sb.c; const hipStream_t st = sb.st; uint8_t *d_dst = sb.d_dst;
    if (sb.algo == PNA_ALGO_DEFLATE && sb.fj && sb.fj->adler_carry) {
        if (!launch_deflate_write_run) return fail(c, PNA_E_UNSUPPORTED, "deflate windows: this build has no k_dfold");
        launch_deflate_write_run(sb.d_src, c->d_segs, c->d_blk_seg, p.nblk, (const BlkInfo *)c->blk.p, d_segdst, (const uint64_t *)c->seg_size.p,
                                 (const uint8_t *)c->litc.p, c->d_entry_seg, wbase, st, c->call_stored, /* a wave per block */ p.wave_blk, sb.fj->adler_carry, sb.fj->run);
    }
    else if (sb.algo == PNA_ALGO_XZ) launch_xzenc_write(sb.d_src, c->d_segs, c->d_blk_seg, p.nblk, (const BlkInfo *)c->blk.p, d_segdst, (const uint64_t *)c->seg_size.p, (const uint8_t *)c->litc.p,
                                                        (const uint64_t *)c->tabs.p, p.nseg, c->d_entry_seg, (uint32_t)(sb.e1 - sb.e0), wbase, st, p.wave_blk);
    else if (sb.algo == PNA_ALGO_DEFLATE) launch_deflate_write(sb.d_src, c->d_segs, c->d_blk_seg, p.nblk, (const BlkInfo *)c->blk.p, d_segdst, (const uint64_t *)c->seg_size.p,
                                                               (const uint8_t *)c->litc.p, c->d_entry_seg, (uint32_t)(sb.e1 - sb.e0), wbase, st, c->call_stored, p.wave_blk);
    else launch_write(sb.d_src, c->d_segs, p.nseg, c->d_blk_seg, p.nblk, (const BlkInfo *)c->blk.p, (const SegTables *)c->tabs.p, d_segdst, (const uint8_t *)c->lits.p,
                      (const uint8_t *)c->litc.p, (const uint8_t *)c->seqc.p, wbase, p.any_empty, st, /* a wave per block */ p.wave_blk);
    if (L.carry_in) HIPCHK(c, hipMemcpyAsync(d_dst + L.carry_in, sb.fj->crun->carry, L.carry_in_len, hipMemcpyDeviceToDevice, st));
    if (L.carry_out) HIPCHK(c, hipMemcpyAsync(sb.fj->crun->carry, d_dst + L.carry_out, sb.fj->crun->carry_len, hipMemcpyDeviceToDevice, st));
    if (L.spread.empty()) return PNA_OK;
    std::vector<PlaceDescH> pd(L.spread.size());
    for (size_t i = 0; i < L.spread.size(); i++) pd[i] = PlaceDescH{L.spread[i].src, L.spread[i].dst, L.spread[i].len, 0};
    if (c->ci_spread.ensure(L.spread_bytes + 64) || c->ci_spread_desc.ensure(pd.size() * sizeof(PlaceDescH) + 16)) return fail(c, PNA_E_NOMEM, "chunk workspace");
    uint64_t sp = 0;
    for (auto &cp : L.spread_copy) { HIPCHK(c, hipMemcpyAsync((uint8_t *)c->ci_spread.p + sp, d_dst + cp.first, cp.second, hipMemcpyDeviceToDevice, st)); sp += (cp.second + 15) & ~(uint64_t)15; }
    HIPCHK(c, hipMemcpyAsync(c->ci_spread_desc.p, pd.data(), pd.size() * sizeof(PlaceDescH), hipMemcpyHostToDevice, st));
    launch_gather(c->ci_spread_desc.p, (uint32_t)pd.size(), (const uint8_t *)c->ci_spread.p, d_dst, st);
    HIPCHK(c, hipStreamSynchronize(st));                      // pd goes out of scope
    return PNA_OK;
}
// Plain file entries of one FDAT chunk each (no cipher; the worst case of every payload below the chunk limit and of the whole sub-batch below the
// destination's capacity): the archive layout is computed on the device (k_layout) and the host never waits in the middle of the sub-batch.
static int layout_device(const SubBatch &sb, const SubPlan &p, const SubLayout &L, HostMarks &hm) {
    pna_gpu_ctx *c = sb.c; const hipStream_t st = sb.st; const size_t ne = sb.e1 - sb.e0;
    if (c->fr_desc.ensure(ne * sizeof(FrameDesc)) || c->fr_blob.ensure(L.blob_len + 16) || c->fr_segdst.ensure((size_t)(p.nseg + 1) * 8) ||
        c->fr_entoff.ensure((ne + 2 + 2 * (ne / 1024 + 2)) * 8) || c->h_entoff.ensure((ne + 2) * 8)) return fail(c, PNA_E_NOMEM, "framing workspace");
    int rc = ensure_crc(c); if (rc) return rc;
    HIPCHK(c, hipMemcpyAsync(c->fr_desc.p, L.fds, ne * sizeof(FrameDesc), hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(c->fr_blob.p, L.blob, L.blob_len, hipMemcpyHostToDevice, st));
    uint64_t *d_ent = (uint64_t *)c->fr_entoff.p;
    launch_layout((FrameDesc *)c->fr_desc.p, (uint8_t *)c->fr_blob.p, c->d_entry_seg, (const uint64_t *)c->seg_off.p, (uint32_t)ne, p.nseg, sb.out_base,
                  (uint64_t *)c->fr_segdst.p, d_ent, d_ent + ne + 1, st);
    rc = write_stage(sb, p, L, (const uint64_t *)c->fr_segdst.p, sb.d_dst); if (rc) return rc;       // (no carry, no spread: entries of one chunk)
    if (sb.timed) HIPCHK(c, hipEventRecord(c->ev[6], st));
    launch_frame((const FrameDesc *)c->fr_desc.p, (uint32_t)ne, (const uint8_t *)c->fr_blob.p, (const CrcTabs *)c->crc_tabs.p,
                 sb.d_dst, (uint64_t)sb.dst_cap & ~(uint64_t)15, frame_fend_crc(), "FDAT", true, st, p.frame_max_payload);
    if (sb.timed) HIPCHK(c, hipEventRecord(c->ev[7], st));
    // the entry offsets (when the caller wants them) and the sub-batch's length travel back behind the kernels: the call's one wait
    uint64_t *h_ent = (uint64_t *)c->h_entoff.p;
    if (sb.fj->want_offsets) HIPCHK(c, hipMemcpyAsync(h_ent, d_ent, (ne + 2) * 8, hipMemcpyDeviceToHost, st));
    else HIPCHK(c, hipMemcpyAsync(h_ent + ne, d_ent + ne, 16, hipMemcpyDeviceToHost, st));
    hm.mark("framing queued");
    HIPCHK(c, hipStreamSynchronize(st));
    hm.mark("device done"); hm.print(ne);
    HIPCHK(c, hipGetLastError());
    if (sb.fj->want_offsets) memcpy(sb.dst_off + sb.e0, h_ent, ne * 8);
    sb.dst_off[sb.e1] = h_ent[ne];
    c->last_nblk = p.nblk;
    return sb.timed ? collect_timing(c, sb.algo == PNA_ALGO_DEFLATE, p.nseg, p.nblk, false) : PNA_OK;
}
// The cipher stage over the laid-out payloads, in place, before k_frame takes their CRC-32: CTR, CBC, or GCM STREAM (CTR under per-segment keys + tags)
static int cipher_stage(const SubBatch &sb, const SubLayout &L) {
    pna_gpu_ctx *c = sb.c; const FrameJob *fj = sb.fj; const hipStream_t st = sb.st; const size_t e0 = sb.e0, e1 = sb.e1;
    const bool gcm = fj->cipher->cipher_mode == PNA_MODE_GCM;
    if (fj->solid && fj->cipher->cipher_mode == PNA_MODE_CBC) return fail(c, PNA_E_UNSUPPORTED, "solid archives: CTR and GCM on the device path (CBC encryption is one serial chain over the whole stream)");
    if (c->ci_units.ensure(L.cunits.size() * sizeof(CipherUnit) + 16) || c->ci_ivs.ensure((e1 - e0) * 16 + 16)) return fail(c, PNA_E_NOMEM, "cipher workspace");
    BlockKey key; key.expand(fj->cipher->encryption, fj->cipher->key);
    HIPCHK(c, hipMemcpyAsync(c->ci_units.p, L.cunits.data(), L.cunits.size() * sizeof(CipherUnit), hipMemcpyHostToDevice, st));
    int rc;
    if (gcm) {
        if (c->ci_gcm.ensure(L.gents.size() * sizeof(GcmEntry) + 16) || c->ci_ivs.ensure(L.giv.size() + 16)) return fail(c, PNA_E_NOMEM, "cipher workspace");
        HIPCHK(c, hipMemcpyAsync(c->ci_ivs.p, L.giv.data(), L.giv.size(), hipMemcpyHostToDevice, st));
        rc = L.gkeys.upload(c, st); if (rc) return rc;
        HIPCHK(c, hipMemcpyAsync(c->ci_gcm.p, L.gents.data(), L.gents.size() * sizeof(GcmEntry), hipMemcpyHostToDevice, st));
        HIPCHK(c, hipStreamSynchronize(st));                  // (the copies read host vectors)
    } else HIPCHK(c, hipMemcpyAsync(c->ci_ivs.p, fj->ivs + 16 * e0, (e1 - e0) * 16, hipMemcpyHostToDevice, st));
    const CipherUnit *units = (const CipherUnit *)c->ci_units.p; const uint32_t nu = (uint32_t)L.cunits.size(); const uint8_t *ivs = (const uint8_t *)c->ci_ivs.p;
    rc = fj->cipher->cipher_mode == PNA_MODE_CBC ? cipher_cbc_enc(c, units, nu, ivs, sb.d_dst, key, st)
                                                 : cipher_ctr(c, units, nu, ivs, sb.d_dst, key, gcm ? &L.gkeys : nullptr, st);   // (GCM: per-segment keys)
    if (rc) return rc;
    if (gcm) launch_gcm_tag((const GcmEntry *)c->ci_gcm.p, (uint32_t)L.gents.size(), sb.d_dst, st);
    return cipher_mark(c, 1, st);
}
// A sub-batch without a single file (the tree entry points: a run of directories and links): no segment, so no LZ, entropy, write or framing launch --
// the finished records, which lie back to back in the call's blob, go to their place in one copy
static int records_subbatch(const SubBatch &sb) {
    pna_gpu_ctx *c = sb.c; const EntryRecords &r = *sb.fj->recs;
    const uint64_t b0 = r.off[sb.e0], bytes = r.off[sb.e1] - b0;
    if (sb.out_base + bytes + 16 > sb.dst_cap) return fail(c, PNA_E_DSTSIZE, "device destination too small");
    for (size_t e = sb.e0; e <= sb.e1; e++) sb.dst_off[e] = sb.out_base + (r.off[e] - b0);
    if (bytes) HIPCHK(c, hipMemcpyAsync(sb.d_dst + sb.out_base, r.blob.data() + b0, bytes, hipMemcpyHostToDevice, sb.st));
    HIPCHK(c, hipStreamSynchronize(sb.st));
    return PNA_OK;
}
// Compression::No (CompressionWriter's `No` arm, lib/src/compress.rs: the bytes go through as they are): the codec-free sub-batch.  Every payload length is
// known here, so the whole layout is the host's -- no device scan, no read-back -- and the payloads go from the source buffer straight to their places:
//   without a cipher   k_store<true> (copy + the pieces' CRC registers) and k_store_fold (the chunks' CRC fields, FEND);
//                      option store_unfused: k_store<false> and k_frame, the form the fused one is measured against;
//   with a cipher      k_store<false>, the cipher stage over the payloads where they stand, k_frame over the ciphertext -- as on the compressed paths.
// The framing bytes (records of entries that are not files, prefixes, the headers of further data chunks) travel in one blob and k_gather puts them down.
// Record: FHED(kind 0, compression 0, enc, mode) | extra | fSIZ | facets | [PHSF] | [FDAT(iv / GCM header)] | FDAT(payload)* | FEND, the payload stream cut
// at max_chunk_size as FlattenWriter cuts it.  An empty file without a cipher, or under CTR, has no FDAT of its own (FlattenWriter ignores empty writes);
// CBC always writes its padding block, GCM STREAM the empty final segment's tag.  GCM segments go where they stand between their tags at once: no spread.
// One WINDOW of a stored solid stream from host memory (pna_gpu_create_solid_archive_*_host with PNA_ALGO_STORE, pna_pipeline.cpp solid_stream): the window's bytes
// -- serialised inner records, their CRCs already in place -- are stream positions [pos, pos + len) of a stream of fj->stream_len bytes, and go out as the pieces of
// the SDAT chunks they belong to: SDAT chunk k holds stream bytes [k SCH, (k + 1) SCH) (SCH = chunk_limit(max_chunk); GCM STREAM: one chunk per segment -- the windows
// are whole segments, solid_sizes sees to that, so a segment never spans two), its header goes out with its first byte, its CRC with its last.  k_store's copy-only
// form places the bytes, the cipher runs over them where they stand (CTR: the keystream position is the stream position), k_frame's piece mode takes the raw CRC
// register of every piece of a chunk, the host chains the registers of a chunk that spans windows (SolidStoreRun) and k_crc_patch writes the CRCs that are
// complete.  The bytes are create_solid_store's for every window size.
static int store_solid_window(const SubBatch &sb) {
    pna_gpu_ctx *c = sb.c; const FrameJob *fj = sb.fj; const hipStream_t st = sb.st;
    SolidStoreRun *sr = fj->srun;
    if (!sr || sb.e1 - sb.e0 != 1 || !launch_store) return fail(c, PNA_E_UNSUPPORTED, "algorithm not implemented on the device path");
    const bool gcm = fj->cipher && fj->cipher->cipher_mode == PNA_MODE_GCM;
    if (fj->cipher && fj->cipher->cipher_mode == PNA_MODE_CBC) return fail(c, PNA_E_UNSUPPORTED, "solid archives: CTR and GCM on the device path (CBC encryption is one serial chain over the whole stream)");
    const uint64_t G = gcm ? gcm_seg_size(fj->cipher) : 0, SCH = gcm ? G : chunk_limit(fj->max_chunk), plain_len = fj->stream_len;
    const uint64_t w0 = sr->pos, w1 = w0 + sb.src_len[sb.e0], so = sb.src_off[sb.e0];
    if (w1 > plain_len || (gcm && (w0 % G || (w1 % G && w1 != plain_len)))) return fail(c, PNA_E_INVAL, "internal: a stored window does not fit its stream");
    const uint64_t K = (plain_len + SCH - 1) / SCH;           // SDAT chunks (= GCM segments) of the whole stream
    std::vector<uint8_t> blob; std::vector<PlaceDescH> lits; std::vector<StorePiece> pieces; std::vector<FrameDesc> fds;
    struct Part { uint64_t len, crc_at; bool ends; };       // a chunk's piece inside the window: its bytes (tag included), where its CRC goes if the chunk ends here
    std::vector<Part> parts;
    SubLayout L;
    if (gcm) { L.gmat.resize(1); gcm_solid_material(fj->cipher, fj->ivs, PNA_ALGO_STORE, L.gmat[0]); }
    uint64_t pos = sb.out_base;
    sb.dst_off[sb.e0] = pos;
    for (uint64_t k = w0 / SCH; k < K && k * SCH < w1; k++) {
        const uint64_t cs = k * SCH, ce = std::min(cs + SCH, plain_len), a = std::max(cs, w0), b = std::min(ce, w1);
        if (a == cs) {
            uint8_t h[8]; put_be32(h, (uint32_t)(ce - cs + (gcm ? 16 : 0))); memcpy(h + 4, "SDAT", 4);
            lits.push_back(PlaceDescH{blob.size(), pos, 8u, 0}); blob.insert(blob.end(), h, h + 8); pos += 8;
        }
        for (uint64_t o = 0; o < b - a; o += STORE_PIECE) pieces.push_back(StorePiece{so + (a - w0) + o, pos + o, (uint32_t)std::min<uint64_t>(STORE_PIECE, b - a - o), 0});
        if (gcm) {
            const uint32_t si = (uint32_t)(L.giv.size() / 16);
            GcmEntry ge{pos, (uint32_t)(b - a), 0, {0, 0, 0, 0}, {0, 0, 0, 0}};
            uint8_t iv[16];
            gcm_segment(L.gmat[0], (uint32_t)k, k + 1 == K, ge, iv);
            L.giv.insert(L.giv.end(), iv, iv + 16);
            L.gkeys.push(si, L.gmat[0].key);
            for (uint64_t o = 0; o < b - a; o += CTR_UNIT) L.cunits.push_back(CipherUnit{pos + o, o, (uint32_t)std::min<uint64_t>(CTR_UNIT, b - a - o), si});
            L.gents.push_back(ge);
        } else if (fj->cipher)
            for (uint64_t o = 0; o < b - a; o += CTR_UNIT) L.cunits.push_back(CipherUnit{pos + o, a + o, (uint32_t)std::min<uint64_t>(CTR_UNIT, b - a - o), 0u});
        const uint64_t pl = b - a + (gcm ? 16 : 0);
        fds.push_back(FrameDesc{pos, (uint32_t)pl, 0u, 0u, 4u | (a == cs ? 0u : 8u)});
        pos += pl;
        parts.push_back(Part{pl, pos, b == ce});
        if (b == ce) pos += 4;
    }
    if (pos + 16 > sb.dst_cap) return fail(c, PNA_E_DSTSIZE, "device destination too small");
    const size_t np = pieces.size(), nl = lits.size(), nf = fds.size();
    if (c->fr_blob.ensure(blob.size() + 16) || c->st_lits.ensure(nl * sizeof(PlaceDescH) + 16) || c->st_pieces.ensure(np * sizeof(StorePiece) + 16) ||
        c->fr_desc.ensure(nf * sizeof(FrameDesc) + 16) || c->st_states.ensure(nf * 4 + 16) || c->st_chunks.ensure(nf * sizeof(CrcPatchH) + 16))
        return fail(c, PNA_E_NOMEM, "stored workspace");
    int rc = ensure_crc(c); if (rc) return rc;
    if (!blob.empty()) HIPCHK(c, hipMemcpyAsync(c->fr_blob.p, blob.data(), blob.size(), hipMemcpyHostToDevice, st));
    if (nl) HIPCHK(c, hipMemcpyAsync(c->st_lits.p, lits.data(), nl * sizeof(PlaceDescH), hipMemcpyHostToDevice, st));
    if (np) HIPCHK(c, hipMemcpyAsync(c->st_pieces.p, pieces.data(), np * sizeof(StorePiece), hipMemcpyHostToDevice, st));
    if (nf) HIPCHK(c, hipMemcpyAsync(c->fr_desc.p, fds.data(), nf * sizeof(FrameDesc), hipMemcpyHostToDevice, st));
    launch_gather(c->st_lits.p, (uint32_t)nl, (const uint8_t *)c->fr_blob.p, sb.d_dst, st);
    launch_store(c->st_pieces.p, (uint32_t)np, sb.d_src, sb.d_dst, (const CrcTabs *)c->crc_tabs.p, nullptr, false, st);
    if (fj->cipher) { rc = cipher_stage(sb, L); if (rc) return rc; }
    std::vector<uint32_t> states(nf);
    launch_frame_pieces((const FrameDesc *)c->fr_desc.p, (uint32_t)nf, (const CrcTabs *)c->crc_tabs.p, sb.d_dst, (uint64_t)sb.dst_cap & ~(uint64_t)15, "SDAT", (uint32_t *)c->st_states.p, st);
    HIPCHK(c, hipGetLastError());
    if (nf) HIPCHK(c, hipMemcpyAsync(states.data(), c->st_states.p, nf * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    std::vector<CrcPatchH> patches;
    for (size_t q = 0; q < nf; q++) {                        // (only the window's first part can continue a chunk, only its last can leave one open)
        sr->state = sr->started ? (crc_gf2_mulmod(crc_gf2_xpow(8 * parts[q].len), sr->state) ^ states[q]) : states[q];
        sr->started = !parts[q].ends;
        if (parts[q].ends) patches.push_back(CrcPatchH{(int64_t)parts[q].crc_at, ~sr->state, 15u});
    }
    if (!patches.empty()) {
        HIPCHK(c, hipMemcpyAsync(c->st_chunks.p, patches.data(), patches.size() * sizeof(CrcPatchH), hipMemcpyHostToDevice, st));
        launch_crc_patch(c->st_chunks.p, (uint32_t)patches.size(), sb.d_dst, st);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipStreamSynchronize(st));
    }
    sr->pos = w1;
    sb.dst_off[sb.e1] = pos;
    c->st_copy_only += np;
    return PNA_OK;
}
static int store_subbatch(const SubBatch &sb) {
    pna_gpu_ctx *c = sb.c; const FrameJob *fj = sb.fj; const hipStream_t st = sb.st; const size_t e0 = sb.e0, e1 = sb.e1;
    if (fj && fj->solid && fj->srun) return store_solid_window(sb);
    if (!fj || fj->solid) return fail(c, PNA_E_UNSUPPORTED, "algorithm not implemented on the device path");
    if (!launch_store || !launch_store_fold) return fail(c, PNA_E_UNSUPPORTED, "algorithm not implemented on the device path");
    const EntryRecords *recs = fj->recs;
    const uint64_t CH = chunk_limit(fj->max_chunk);
    const int mode = fj->cipher ? fj->cipher->cipher_mode : -1;
    const bool cbc = mode == PNA_MODE_CBC, gcm = mode == PNA_MODE_GCM, ctr = mode == PNA_MODE_CTR;
    const uint64_t G = gcm ? gcm_seg_size(fj->cipher) : 0;
    // the form of an unencrypted sub-batch (option store_unfused; -1: by its longest data chunk, as measured -- profiles/store_rate.txt): chunks of one piece
    // (10 000 x 1 MiB) are faster through the copy-only form and k_frame, 8.6 against 12.2 ms; a chunk of several pieces must not be CRC'd by one workgroup
    // (one entry of 4 GiB: 4.6 against 839 ms), and at 4 KiB the fused form is ahead again (27.9 against 28.4 ms).  Sizes between 4 KiB and 1 MiB were not measured.
    uint64_t longest = 0;
    if (!fj->cipher && c->tun.store_unfused < 0)
        for (size_t e = e0; e < e1; e++) if (!(recs && recs->len(e))) longest = std::max<uint64_t>(longest, std::min<uint64_t>(sb.src_len[e], CH));
    const bool fused = !fj->cipher && (c->tun.store_unfused < 0 ? (longest > STORE_PIECE || longest <= 4096) : c->tun.store_unfused == 0);
    GcmCallKeys gkeys{};
    if (gcm) gkeys = gcm_call_keys(fj->cipher->key, fj->cipher->phsf, strlen(fj->cipher->phsf));
    std::vector<uint8_t> blob, tmp;                          // the framing bytes; lits: where they go (src_off: in the blob)
    std::vector<PlaceDescH> lits;
    std::vector<StorePiece> pieces; std::vector<StoreChunk> chunks; std::vector<FrameDesc> units;
    SubLayout L; GcmMaterial gm;
    uint64_t pos = sb.out_base;
    uint8_t fend[12] = {0, 0, 0, 0, 'F', 'E', 'N', 'D', 0, 0, 0, 0};
    put_be32(fend + 8, frame_fend_crc());
    auto lit = [&](const uint8_t *p, size_t n) {             // n framing bytes at `pos` (in pieces that fit a descriptor's 32-bit length)
        for (size_t o = 0; o < n; o += 0x40000000u) lits.push_back(PlaceDescH{blob.size() + o, pos + o, (uint32_t)std::min<size_t>(0x40000000u, n - o), 0});
        blob.insert(blob.end(), p, p + n); pos += n;
    };
    auto payload = [&](uint64_t src, uint64_t dst, uint64_t n) { for (uint64_t o = 0; o < n; o += STORE_PIECE) pieces.push_back(StorePiece{src + o, dst + o, (uint32_t)std::min<uint64_t>(STORE_PIECE, n - o), 0}); };
    for (size_t e = e0; e < e1; e++) {
        sb.dst_off[e] = pos;
        if (recs && recs->len(e)) { lit(recs->at(e), (size_t)recs->len(e)); continue; }
        const uint64_t len = sb.src_len[e], so = sb.src_off[e];
        tmp.clear();
        if (gcm) { gcm_entry_material(fj->cipher, gkeys, fj->ivs + 39 * e, (uint32_t)G, fj->names[e], PNA_ALGO_STORE, gm);
                   frame_entry_prefix_enc(tmp, fj->names[e], PNA_ALGO_STORE, len, fj->cipher->encryption, PNA_MODE_GCM, fj->cipher->phsf, gm.header, 75); }
        else if (fj->cipher) frame_entry_prefix_enc(tmp, fj->names[e], PNA_ALGO_STORE, len, fj->cipher->encryption, mode, fj->cipher->phsf, fj->ivs + 16 * e, 16);
        else frame_entry_prefix(tmp, fj->names[e], PNA_ALGO_STORE, len, 0);
        splice_meta(tmp, fj->meta, e);                       // (tmp ends in the first payload chunk's length and type)
        if (len == 0 && !cbc && !gcm) { tmp.resize(tmp.size() - 8); tmp.insert(tmp.end(), fend, fend + 12); lit(tmp.data(), tmp.size()); continue; }
        const uint64_t KG = gcm ? (len ? (len + G - 1) / G : 1) : 0;
        const uint64_t plen = cbc ? (len / 16 + 1) * 16 : gcm ? len + 16 * KG : len;      // what the cipher makes of the payload
        if (cbc && plen > CH) return fail(c, PNA_E_UNSUPPORTED, "CBC entry beyond one FDAT chunk");
        if (gcm && KG > 0xFFFFFFFFull) return fail(c, PNA_E_INVAL, "GCM segment counter overflow");
        if (gcm && plen > CH) return fail(c, PNA_E_UNSUPPORTED, "GCM entry beyond one FDAT chunk");
        const uint64_t K = (plen + CH - 1) / CH;
        if (chunks.size() + units.size() + K > 0x7FFFFFF0ull || pieces.size() + plen / STORE_PIECE + K > 0x7FFFFFF0ull) return fail(c, PNA_E_INVAL, "too many data chunks");
        for (uint64_t k = 0; k < K; k++) {
            const uint64_t cl = std::min<uint64_t>(CH, plen - k * CH);
            if (k == 0) { put_be32(tmp.data() + tmp.size() - 8, (uint32_t)cl); lit(tmp.data(), tmp.size()); }
            else { uint8_t h[8]; put_be32(h, (uint32_t)cl); memcpy(h + 4, "FDAT", 4); lit(h, 8); }
            if (blob.size() > 0xFFFFFF00ull) return fail(c, PNA_E_INVAL, "the framing bytes of a sub-batch exceed 4 GiB");      // (FrameDesc::prefix_off; before the descriptor below takes the offset)
            const uint64_t cstart = pos;                     // the chunk's data in the archive
            if (fused) chunks.push_back(StoreChunk{cstart + cl, cl, (uint32_t)pieces.size(), (uint32_t)((cl + STORE_PIECE - 1) / STORE_PIECE), k + 1 == K ? 1u : 0u, 0});
            else units.push_back(FrameDesc{cstart - 8, (uint32_t)cl, (uint32_t)(blob.size() - 8), 8u, k + 1 < K ? 2u : 0u});      // (k_frame puts the header down once more: the same bytes)
            if (gcm) {
                for (uint64_t q = 0; q < KG; q++) {          // segment q at cstart + q (G + 16), its tag behind it; the last one carries the final flag
                    const uint64_t sl = std::min<uint64_t>(G, len - q * G), at = cstart + q * (G + 16);
                    const uint32_t si = (uint32_t)(L.giv.size() / 16);
                    GcmEntry ge{at, (uint32_t)sl, 0, {0, 0, 0, 0}, {0, 0, 0, 0}};
                    uint8_t iv[16];
                    gcm_segment(gm, (uint32_t)q, q + 1 == KG, ge, iv);
                    L.giv.insert(L.giv.end(), iv, iv + 16);
                    L.gkeys.push(si, gm.key);
                    for (uint64_t o = 0; o < sl; o += CTR_UNIT) L.cunits.push_back(CipherUnit{at + o, o, (uint32_t)std::min<uint64_t>(CTR_UNIT, sl - o), si});
                    L.gents.push_back(ge);
                    payload(so + q * G, at, sl);
                }
            } else if (cbc) { L.cunits.push_back(CipherUnit{cstart, 0, (uint32_t)len, (uint32_t)(e - e0)}); payload(so, cstart, len); }
            else {
                payload(so + k * CH, cstart, cl);
                if (ctr) for (uint64_t o = 0; o < cl; o += CTR_UNIT) L.cunits.push_back(CipherUnit{cstart + o, k * CH + o, (uint32_t)std::min<uint64_t>(CTR_UNIT, cl - o), (uint32_t)(e - e0)});
            }
            pos += cl + 4;
        }
        pos += 12;                                           // FEND
        if (blob.size() > 0xFFFFFF00ull) return fail(c, PNA_E_INVAL, "the framing bytes of a sub-batch exceed 4 GiB");      // (FrameDesc::prefix_off)
    }
    sb.dst_off[e1] = pos;
    // the destination holds the sub-batch: nothing has been launched yet.  (k_frame reads whole 16-byte words below the capacity: the cipher forms keep the
    // compressed paths' 16 bytes of room; the fused form touches its own bytes only and takes a destination of exactly the archive's size)
    if (pos + (fused ? 0 : 16) > sb.dst_cap) return fail(c, PNA_E_DSTSIZE, "device destination too small");
    const size_t np = pieces.size(), nl = lits.size(), nc = chunks.size(), nu = units.size();
    if (c->fr_blob.ensure(blob.size() + 16) || c->st_lits.ensure(nl * sizeof(PlaceDescH) + 16) || c->st_pieces.ensure(np * sizeof(StorePiece) + 16) ||
        c->st_chunks.ensure(nc * sizeof(StoreChunk) + 16) || c->st_states.ensure(np * 4 + 16) || c->fr_desc.ensure(nu * sizeof(FrameDesc) + 16))
        return fail(c, PNA_E_NOMEM, "stored workspace");
    int rc = ensure_crc(c); if (rc) return rc;
    for (auto &ev : c->st_ev) if (!ev) HIPCHK(c, hipEventCreate(&ev));
    if (!blob.empty()) HIPCHK(c, hipMemcpyAsync(c->fr_blob.p, blob.data(), blob.size(), hipMemcpyHostToDevice, st));
    if (nl) HIPCHK(c, hipMemcpyAsync(c->st_lits.p, lits.data(), nl * sizeof(PlaceDescH), hipMemcpyHostToDevice, st));
    if (np) HIPCHK(c, hipMemcpyAsync(c->st_pieces.p, pieces.data(), np * sizeof(StorePiece), hipMemcpyHostToDevice, st));
    if (nc) HIPCHK(c, hipMemcpyAsync(c->st_chunks.p, chunks.data(), nc * sizeof(StoreChunk), hipMemcpyHostToDevice, st));
    if (nu) HIPCHK(c, hipMemcpyAsync(c->fr_desc.p, units.data(), nu * sizeof(FrameDesc), hipMemcpyHostToDevice, st));
    launch_gather(c->st_lits.p, (uint32_t)nl, (const uint8_t *)c->fr_blob.p, sb.d_dst, st);
    HIPCHK(c, hipEventRecord(c->st_ev[0], st));
    launch_store(c->st_pieces.p, (uint32_t)np, sb.d_src, sb.d_dst, (const CrcTabs *)c->crc_tabs.p, (uint32_t *)c->st_states.p, fused, st);
    HIPCHK(c, hipEventRecord(c->st_ev[1], st));
    if (fused) launch_store_fold(c->st_chunks.p, (uint32_t)nc, (const uint32_t *)c->st_states.p, c->st_pieces.p, "FDAT", frame_fend_crc(), sb.d_dst, st);
    else {
        if (fj->cipher) { rc = cipher_stage(sb, L); if (rc) return rc; }      // (no unit at all -- every entry empty -- is fine: GCM still writes its tags)
        launch_frame((const FrameDesc *)c->fr_desc.p, (uint32_t)nu, (const uint8_t *)c->fr_blob.p, (const CrcTabs *)c->crc_tabs.p, sb.d_dst,
                     (uint64_t)sb.dst_cap & ~(uint64_t)15, frame_fend_crc(), "FDAT", true, st, 0);
    }
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(st));                      // (the staging vectors are read by the copies; the caller's next sub-batch reuses the workspace)
    float ms = 0; (void)hipEventElapsedTime(&ms, c->st_ev[0], c->st_ev[1]);
    c->st_ms += ms; (fused ? c->st_fused : c->st_copy_only) += np; c->st_folded += nc;
    return PNA_OK;
}
extern "C" int pna_gpu_debug_store_stats(pna_gpu_ctx *c, uint64_t *pieces_fused, uint64_t *pieces_copy_only, uint64_t *chunks_folded, double *ms_k_store) {
    if (!c) return PNA_E_INVAL;
    if (pieces_fused) *pieces_fused = c->st_fused;
    if (pieces_copy_only) *pieces_copy_only = c->st_copy_only;
    if (chunks_folded) *chunks_folded = c->st_folded;
    if (ms_k_store) *ms_k_store = c->st_ms;
    return PNA_OK;
}
// One sub-batch: entries [e0, e1) -> segments -> kernels; output appended at d_dst + out_base.
int run_subbatch(pna_gpu_ctx *c, int algo, const uint8_t *d_src, const uint64_t *src_off, const uint64_t *src_len,
                 size_t e0, size_t e1, uint8_t *d_dst, size_t dst_cap, uint64_t out_base, uint64_t *dst_off,
                 hipStream_t st, bool timed, const FrameJob *fj) {
    const SubBatch sb{c, algo, d_src, src_off, src_len, e0, e1, d_dst, dst_cap, out_base, dst_off, st, timed, fj};
    HostMarks hm{c->tun.trace != 0};
    if (algo == PNA_ALGO_STORE) return store_subbatch(sb);      // no codec: no plan, no LZ stage, no entropy stage
    SubPlan p;
    int rc = plan_subbatch(sb, hm, p);
    if (rc == PNA_OK && p.nseg == 0 && fj && fj->recs) return records_subbatch(sb);
    if (rc || p.nseg == 0) return rc;
    hm.mark("plan queued");
    rc = compress_subbatch(sb, p); if (rc) return rc;
    hm.mark("kernels queued");
    SubLayout L;
    if (fj) { rc = frame_prefixes(sb, p, L); if (rc) return rc; }
    hm.mark("prefixes built");
    if (fj && !fj->solid && !fj->cipher && c->tun.dev_layout != 0 && !L.layout_over && out_base + L.layout_need + 16 <= dst_cap) return layout_device(sb, p, L, hm);
    // the output offsets are needed on the host before the write pass can be bounds-checked
    if (c->h_segoff.ensure((size_t)(p.nseg + 1) * 8)) return fail(c, PNA_E_NOMEM, "offset staging");
    const uint64_t *seg_off = (const uint64_t *)c->h_segoff.p;
    // (plain batches whose destination holds the worst case of every entry need no check against the sizes found: the write kernels go out
    // at once, the offsets travel behind them and the one wait is the call's last -- a wait in the middle of a small batch is a tenth of it)
    bool early_write = !fj;
    if (early_write) { uint64_t need = out_base; for (size_t e = e0; e < e1; e++) need += pna_gpu_bound(algo, (size_t)src_len[e]); early_write = need <= dst_cap; }
    if (!early_write) {
        HIPCHK(c, hipMemcpyAsync(c->h_segoff.p, c->seg_off.p, (size_t)(p.nseg + 1) * 8, hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipStreamSynchronize(st));
        L.total = seg_off[p.nseg];
    }
    const uint64_t *d_segdst = (const uint64_t *)c->seg_off.p;
    uint8_t *wbase = d_dst + out_base;
    if (fj) {
        // the host layout, checked against the destination; its descriptors, prefixes and segment destinations to the device
        uint64_t pos = out_base;
        rc = fj->solid ? layout_solid(sb, p, seg_off, L, pos) : layout_entries(sb, p, seg_off, L, pos); if (rc) return rc;
        L.segdst[p.nseg] = pos;
        L.total = pos - out_base;
        if (pos + 16 > dst_cap) return fail(c, PNA_E_DSTSIZE, "device destination too small");
        if (c->fr_desc.ensure(L.nunit * sizeof(FrameDesc)) || c->fr_blob.ensure(L.blob_len + 16) || c->fr_segdst.ensure((size_t)(p.nseg + 1) * 8))
            return fail(c, PNA_E_NOMEM, "framing workspace");
        rc = ensure_crc(c); if (rc) return rc;
        HIPCHK(c, hipMemcpyAsync(c->fr_desc.p, L.fds, L.nunit * sizeof(FrameDesc), hipMemcpyHostToDevice, st));
        HIPCHK(c, hipMemcpyAsync(c->fr_blob.p, L.blob, L.blob_len, hipMemcpyHostToDevice, st));
        HIPCHK(c, hipMemcpyAsync(c->fr_segdst.p, L.segdst, (size_t)(p.nseg + 1) * 8, hipMemcpyHostToDevice, st));
        d_segdst = (const uint64_t *)c->fr_segdst.p; wbase = d_dst;
    } else if (!early_write && out_base + L.total > dst_cap) return fail(c, PNA_E_DSTSIZE, "device destination too small");
    rc = write_stage(sb, p, L, d_segdst, wbase); if (rc) return rc;
    if (fj && fj->cipher) { rc = cipher_stage(sb, L); if (rc) return rc; }
    // k_frame over the framed units; the offsets (early_write: the segment offsets travel back behind the kernels) and, timed, the stage times.  The call
    // waits here: the staging buffers are reused by the next sub-batch.
    if (timed) HIPCHK(c, hipEventRecord(c->ev[6], st));
    if (fj) launch_frame((const FrameDesc *)c->fr_desc.p, (uint32_t)L.nunit, (const uint8_t *)c->fr_blob.p, (const CrcTabs *)c->crc_tabs.p,
                         d_dst, (uint64_t)dst_cap & ~(uint64_t)15, frame_fend_crc(), fj->solid ? "SDAT" : "FDAT", !fj->solid, st, p.frame_max_payload);
    if (timed) HIPCHK(c, hipEventRecord(c->ev[7], st));
    HIPCHK(c, hipGetLastError());
    if (early_write) {
        HIPCHK(c, hipMemcpyAsync(c->h_segoff.p, c->seg_off.p, (size_t)(p.nseg + 1) * 8, hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipStreamSynchronize(st));
        L.total = seg_off[p.nseg];
    }
    if (!fj) for (size_t e = e0; e < e1; e++) dst_off[e] = out_base + seg_off[p.entry_first_seg[e - e0]];
    dst_off[e1] = out_base + L.total;
    c->last_nblk = p.nblk;
    if (fj || timed) HIPCHK(c, hipStreamSynchronize(st));
    return timed ? collect_timing(c, algo == PNA_ALGO_DEFLATE, p.nseg, p.nblk, fj && fj->cipher) : PNA_OK;
}

extern "C" int pna_gpu_compress_batch_device(pna_gpu_ctx *c, int algo, int level, size_t n, const void *d_src,
                                             const uint64_t *src_off, const uint64_t *src_len, void *d_dst, size_t dst_cap,
                                             uint64_t *dst_off, void *hip_stream) {
    if (!c || !src_off || !src_len || !dst_off || (!d_src && n) || (!d_dst && n)) return fail(c, PNA_E_INVAL, "null argument");
    if (!encode_algo_ok(c, algo)) return fail(c, PNA_E_UNSUPPORTED, "algorithm not implemented on the device path");
    set_call_level(c, algo, level);
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : c->stream;
    c->timing = pna_gpu_timing{};
    dst_off[0] = 0;
    uint64_t out_base = 0, in_total = 0;
    size_t e = 0;
    plan_call(c, src_len, n);
    const CallTotalScope call_total(c, src_len, n);                                              // (the block size follows the call, not its sub-batches)
    while (e < n) {
        size_t e1 = e; size_t blocks = 0;
        while (e1 < n) {
            size_t nb = plan_blocks(c, src_len[e1]);
            if (e1 > e && blocks + nb > c->max_blocks) break;
            blocks += nb; in_total += src_len[e1]; e1++;
        }
        int rc = run_subbatch(c, algo, (const uint8_t *)d_src, src_off, src_len, e, e1, (uint8_t *)d_dst, dst_cap, out_base, dst_off, st, true);
        if (rc) return rc;
        out_base = dst_off[e1];
        e = e1;
    }
    HIPCHK(c, hipStreamSynchronize(st));
    c->timing.in_bytes = in_total; c->timing.out_bytes = out_base;
    return PNA_OK;
}

extern "C" size_t pna_gpu_archive_bound(int algo, size_t n, const char *const *names, const uint64_t *src_len) {
    size_t b = 28 + 12 + 64;                                    // signature + AHED, AEND, alignment slack of the CRC reads
    for (size_t i = 0; i < n; i++) {
        const size_t pb = pna_gpu_bound(algo, (size_t)src_len[i]);
        b += frame_entry_prefix_bound(names ? names[i] : nullptr) + pb + 16 + 12 * (src_len[i] >> 20);    // + one FDAT header / CRC per possible cut
    }
    return b;
}

// Non-solid `pna create` with the archive assembled in HBM: create_archive_file (cli/src/command/create.rs:575-635) +
// Archive::write_header / add_entry / finalize (lib/src/archive/write.rs) for file entries carrying FHED, fSIZ, FDAT, FEND.
extern "C" int pna_gpu_create_archive_device(pna_gpu_ctx *c, int algo, int level, size_t n, const char *const *names,
                                             const void *d_src, const uint64_t *src_off, const uint64_t *src_len,
                                             void *d_dst, size_t dst_cap, uint64_t *entry_off, uint64_t *archive_len,
                                             void *hip_stream) {
    return pna_gpu_create_archive_part_device(c, algo, level, n, names, d_src, src_off, src_len, d_dst, dst_cap, entry_off, archive_len,
                                              PNA_PART_HEAD | PNA_PART_TAIL, hip_stream);
}

// One shard of an archive whose entries are split over several producers (ranks): only the first shard carries the signature +
// AHED, only the last one AEND; the shards' outputs concatenated in entry order are the archive.
extern "C" int pna_gpu_create_archive_part_device(pna_gpu_ctx *c, int algo, int level, size_t n, const char *const *names,
                                                  const void *d_src, const uint64_t *src_off, const uint64_t *src_len,
                                                  void *d_dst, size_t dst_cap, uint64_t *entry_off, uint64_t *archive_len,
                                                  uint32_t part_flags, void *hip_stream) {
    return pna_gpu_create_archive_enc_device(c, algo, level, n, names, d_src, src_off, src_len, nullptr, d_dst, dst_cap, entry_off, archive_len,
                                             part_flags, hip_stream);
}

extern "C" size_t pna_gpu_archive_enc_bound(int algo, size_t n, const char *const *names, const uint64_t *src_len, const pna_gpu_cipher *cipher) {
    size_t b = pna_gpu_archive_bound(algo, n, names, src_len);
    if (cipher && cipher->encryption != PNA_ENC_NONE && cipher->phsf) {
        b += n * (12 + strlen(cipher->phsf) + 12 + 75 + 16);   // PHSF, FDAT(iv | stream header), CBC padding / the final GCM tag
        if (cipher->cipher_mode == PNA_MODE_GCM) {               // one more tag per full stream segment of the (bounded) payload
            const uint64_t seg = gcm_seg_size(cipher);
            for (size_t i = 0; i < n; i++) b += 16 * (pna_gpu_bound(algo, (size_t)src_len[i]) / seg);
        }
    }
    return b;
}

// The same with the cipher stage between the write kernels and the chunk CRC (get_writer: compress -> cipher -> sink,
// lib/src/entry/write.rs:268-274): entry record FHED | fSIZ | PHSF | FDAT(iv) | FDAT(ciphertext) | FEND.
extern "C" int pna_gpu_create_archive_enc_device(pna_gpu_ctx *c, int algo, int level, size_t n, const char *const *names,
                                                 const void *d_src, const uint64_t *src_off, const uint64_t *src_len,
                                                 const pna_gpu_cipher *cipher, void *d_dst, size_t dst_cap, uint64_t *entry_off,
                                                 uint64_t *archive_len, uint32_t part_flags, void *hip_stream) {
    return pna_gpu_create_archive_meta_device(c, algo, level, n, names, d_src, src_off, src_len, cipher, nullptr, d_dst, dst_cap, entry_off, archive_len,
                                              part_flags, hip_stream);
}

int check_meta(pna_gpu_ctx *c, const pna_gpu_entry_meta *meta, size_t n) {
    if (!meta) return PNA_OK;
    if ((meta->extra && !meta->extra_len) || (meta->facets && !meta->facets_len)) return fail(c, PNA_E_INVAL, "metadata blobs without lengths");
    for (size_t e = 0; e < n; e++) {
        if (meta->extra && meta->extra_len[e] && (!meta->extra[e] || !meta_blob_ok((const uint8_t *)meta->extra[e], meta->extra_len[e]))) return fail(c, PNA_E_INVAL, "extra chunks of an entry are not well-formed chunks");
        if (meta->facets && meta->facets_len[e] && (!meta->facets[e] || !meta_blob_ok((const uint8_t *)meta->facets[e], meta->facets_len[e]))) return fail(c, PNA_E_INVAL, "metadata chunks of an entry are not well-formed chunks");
    }
    return PNA_OK;
}

// The entry kinds of a tree call (pna_gpu_entry_kinds; create_entry's four arms, cli/src/command/core.rs:915-977): every kind known, a non-file without source
// bytes, a link with a target.  Needs no context.
extern "C" int pna_gpu_entry_kinds_check(size_t n, const uint64_t *src_len, const pna_gpu_entry_kinds *kinds) {
    if (!kinds || !kinds->kind) return PNA_OK;
    if (n && !src_len) return PNA_E_INVAL;
    for (size_t e = 0; e < n; e++) {
        const uint8_t k = kinds->kind[e];
        if (k == PNA_KIND_FILE) continue;
        if (k > PNA_KIND_HARDLINK || src_len[e] != 0) return PNA_E_INVAL;
        if (k != PNA_KIND_DIRECTORY && (!kinds->link || !kinds->link_len || !kinds->link[e] || !kinds->link_len[e])) return PNA_E_INVAL;
    }
    return PNA_OK;
}
int build_entry_records(pna_gpu_ctx *c, size_t n, const char *const *names, const uint64_t *src_len, const pna_gpu_entry_kinds *kinds,
                        const pna_gpu_entry_meta *meta, uint32_t max_chunk, EntryRecords &out) {
    out = EntryRecords{};
    if (!kinds || !kinds->kind) return PNA_OK;
    if (pna_gpu_entry_kinds_check(n, src_len, kinds)) return fail(c, PNA_E_INVAL, "entry kinds: an unknown kind, a non-file with source bytes, or a link without a target");
    out.off.resize(n + 1);
    for (size_t e = 0; e < n; e++) {
        out.off[e] = out.blob.size();
        const int k = kinds->kind[e];
        if (k == PNA_KIND_FILE) continue;
        const bool ex = meta && meta->extra && meta->extra_len && meta->extra_len[e], fa = meta && meta->facets && meta->facets_len && meta->facets_len[e];
        frame_nonfile_record(out.blob, k, names[e], ex ? meta->extra[e] : nullptr, ex ? meta->extra_len[e] : 0, fa ? meta->facets[e] : nullptr, fa ? meta->facets_len[e] : 0,
                             k == PNA_KIND_DIRECTORY ? nullptr : kinds->link[e], k == PNA_KIND_DIRECTORY ? 0 : kinds->link_len[e], max_chunk);
        if (out.blob.size() - out.off[e] > 0x7FFFFFFFull) return fail(c, PNA_E_INVAL, "a link's record exceeds 2 GiB");
        out.count++;
    }
    out.off[n] = out.blob.size();
    if (!out.count) out = EntryRecords{};                      // every entry a file: the counterpart's path
    return PNA_OK;
}

// ... and with per-entry metadata: chunks the host has already framed (timestamps, permissions, owner, xattr: try_for_each_metadata_facet,
// lib/src/entry.rs:124-180; user-defined extra chunks) are placed where NormalEntry::write_chunks_to puts them.
int create_archive_device_impl(pna_gpu_ctx *c, int algo, int level, size_t n, const char *const *names,
                                      const void *d_src, const uint64_t *src_off, const uint64_t *src_len,
                                      const pna_gpu_cipher *cipher, const pna_gpu_entry_meta *meta, uint32_t max_chunk, void *d_dst, size_t dst_cap,
                                      uint64_t *entry_off, uint64_t *archive_len, uint32_t part_flags, void *hip_stream, const pna_gpu_entry_kinds *kinds = nullptr);
extern "C" int pna_gpu_create_archive_meta_device(pna_gpu_ctx *c, int algo, int level, size_t n, const char *const *names,
                                                  const void *d_src, const uint64_t *src_off, const uint64_t *src_len,
                                                  const pna_gpu_cipher *cipher, const pna_gpu_entry_meta *meta, void *d_dst, size_t dst_cap,
                                                  uint64_t *entry_off, uint64_t *archive_len, uint32_t part_flags, void *hip_stream) {
    return create_archive_device_impl(c, algo, level, n, names, d_src, src_off, src_len, cipher, meta, c ? (uint32_t)c->tun.max_chunk_size : 0u, d_dst, dst_cap, entry_off, archive_len, part_flags, hip_stream);
}
extern "C" int pna_gpu_create_archive_chunked_device(pna_gpu_ctx *c, int algo, int level, size_t n, const char *const *names,
                                                     const void *d_src, const uint64_t *src_off, const uint64_t *src_len,
                                                     const pna_gpu_cipher *cipher, const pna_gpu_entry_meta *meta, uint32_t max_chunk_size, void *d_dst, size_t dst_cap,
                                                     uint64_t *entry_off, uint64_t *archive_len, uint32_t part_flags, void *hip_stream) {
    return create_archive_device_impl(c, algo, level, n, names, d_src, src_off, src_len, cipher, meta, max_chunk_size, d_dst, dst_cap, entry_off, archive_len, part_flags, hip_stream);
}
extern "C" size_t pna_gpu_archive_chunked_bound(int algo, size_t n, const char *const *names, const uint64_t *src_len, const pna_gpu_cipher *cipher, uint32_t max_chunk_size) {
    size_t b = cipher && cipher->encryption != PNA_ENC_NONE ? pna_gpu_archive_enc_bound(algo, n, names, src_len, cipher) : pna_gpu_archive_bound(algo, n, names, src_len);
    const uint64_t CH = chunk_limit(max_chunk_size);
    for (size_t i = 0; i < n; i++) b += 12 * (size_t)((pna_gpu_bound(algo, (size_t)src_len[i]) + 64 + 16 * (src_len[i] >> 12)) / CH + 1);   // a CRC + a header per further chunk
    return b;
}
int create_archive_device_impl(pna_gpu_ctx *c, int algo, int level, size_t n, const char *const *names,
                                      const void *d_src, const uint64_t *src_off, const uint64_t *src_len,
                                      const pna_gpu_cipher *cipher, const pna_gpu_entry_meta *meta, uint32_t max_chunk, void *d_dst, size_t dst_cap,
                                      uint64_t *entry_off, uint64_t *archive_len, uint32_t part_flags, void *hip_stream, const pna_gpu_entry_kinds *kinds) {
    { int rcm = check_meta(c, meta, n); if (rcm) return rcm; }
    if (!c || !archive_len || (n && (!names || !src_off || !src_len)) || !d_dst) return fail(c, PNA_E_INVAL, "null argument");
    EntryRecords recs;                                          // the tree form: the records of the entries that are not files
    { int rck = build_entry_records(c, n, names, src_len, kinds, meta, max_chunk, recs); if (rck) return rck; }
    if (!d_src && recs.count < n) return fail(c, PNA_E_INVAL, "null argument");
    if (!encode_algo_ok(c, algo, true)) return fail(c, PNA_E_UNSUPPORTED, "algorithm not implemented on the device path");
    if ((uintptr_t)d_dst & 15) return fail(c, PNA_E_INVAL, "archive buffer must be 16-byte aligned");
    if (cipher && cipher->encryption == PNA_ENC_NONE) cipher = nullptr;
    const auto t_call0 = std::chrono::steady_clock::now();
    auto call_ms = [&]() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_call0).count(); };
    std::vector<uint8_t> own_ivs;
    const uint8_t *ivs = nullptr;
    if (cipher) { int rc = resolve_ivs(c, cipher, n, own_ivs, &ivs); if (rc) return rc; }
    set_call_level(c, algo, level);
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : c->stream;
    c->timing = pna_gpu_timing{};
    c->st_fused = c->st_copy_only = c->st_folded = 0; c->st_ms = 0;
    std::vector<uint8_t> head, tail;
    if (part_flags & PNA_PART_HEAD) frame_archive_head(head, 0);
    if (part_flags & PNA_PART_TAIL) frame_archive_tail(tail);
    if (head.size() + tail.size() + 16 > dst_cap) return fail(c, PNA_E_DSTSIZE, "device destination too small");
    if (!head.empty()) HIPCHK(c, hipMemcpyAsync(d_dst, head.data(), head.size(), hipMemcpyHostToDevice, st));
    // (10^6 entries: the call's own loops over them -- the total, the longest, the sub-batch cut -- ran one after the other on one thread, ~2 ms in front of the first
    // kernel and a zero-filled vector of offsets behind it; round 5: one pass on several threads, the cut by arithmetic where every entry is one block)
    std::unique_ptr<uint64_t[]> offs_mem(new uint64_t[n + 1]);
    uint64_t *offs = offs_mem.get();
    uint64_t pos = head.size(), in_total = 0, longest = 0;
    {
        const unsigned nt = host_loop_threads(n);
        std::vector<uint64_t> part_sum(nt, 0), part_max(nt, 0);
        par_ranges(n, nt, [&](unsigned t, size_t a, size_t b) { uint64_t sm = 0, mx = 0; for (size_t i = a; i < b; i++) { sm += src_len[i]; mx = std::max<uint64_t>(mx, src_len[i]); } part_sum[t] = sm; part_max[t] = mx; });
        for (unsigned t = 0; t < nt; t++) { in_total += part_sum[t]; longest = std::max(longest, part_max[t]); }
    }
    const CallTotalScope call_total(c, in_total);                                                // (the block size follows the call, not its sub-batches)
    FrameJob fj{names, 0, cipher, ivs, meta, max_chunk, entry_off != nullptr};
    if (recs.count) fj.recs = &recs;
    size_t e = 0;
    plan_call_longest(c, longest);
    const bool one_block_each = longest <= ((uint64_t)1 << c->plan_log);
    while (e < n) {
        size_t e1 = e, blocks = 0;
        if (one_block_each) e1 = std::min(n, e + std::max<size_t>(1, c->max_blocks));           // (an empty entry counts as a block of its own here: the cut only has to respect the budget)
        else while (e1 < n) {
            size_t nb = plan_blocks(c, src_len[e1]);
            if (e1 > e && blocks + nb > c->max_blocks) break;
            blocks += nb; e1++;
        }
        if (c->tun.trace) fprintf(stderr, "[pna create_archive_device] sub-batch of %zu entries starts at %.2f ms of the call\n", e1 - e, call_ms());
        int rc = run_subbatch(c, algo, (const uint8_t *)d_src, src_off, src_len, e, e1, (uint8_t *)d_dst, dst_cap - tail.size(), pos, offs, st, true, &fj);
        if (rc) return rc;
        if (c->tun.trace) fprintf(stderr, "[pna create_archive_device] sub-batch back at %.2f ms\n", call_ms());
        pos = offs[e1];
        e = e1;
    }
    offs[n] = pos;
    if (!tail.empty()) HIPCHK(c, hipMemcpyAsync((uint8_t *)d_dst + pos, tail.data(), tail.size(), hipMemcpyHostToDevice, st));
    HIPCHK(c, hipStreamSynchronize(st));
    pos += tail.size();
    if (entry_off) memcpy(entry_off, offs, (n + 1) * 8);
    *archive_len = pos;
    c->timing.in_bytes = in_total; c->timing.out_bytes = pos;
    if (c->tun.trace) fprintf(stderr, "[pna create_archive_device] call ends at %.2f ms\n", call_ms());
    return PNA_OK;
}

// ---------------------------------------------------------------------------------------------------------
// `pna create --solid` with the archive assembled in HBM (create_archive_file's solid branch, cli/src/command/create.rs:594-598,
// 603-617; SolidArchive / SolidEntryBuilder, lib/src/archive/write.rs:443-470,575-580,716-727):
//   1. the inner entries are serialised as STORE records FHED | fSIZ | FDAT | FEND (their FDAT CRC-32 computed by k_frame) into
//      one stream in HBM,
//   2. that stream is compressed as ONE entry (independent 1 MiB frames / zlib blocks inside the kernels),
//   3. every segment's output becomes one SDAT chunk between SHED and SEND.

// the bound of a solid archive whose inner stream holds `plain` bytes, then what a cipher adds to it
static size_t solid_bound_of(int algo, uint64_t plain) {
    const uint64_t segs = (plain + SEG_SIZE - 1) / SEG_SIZE + 1;
    return 28 + 17 + pna_gpu_bound(algo, (size_t)plain) + 12 * segs + 12 + 12 + 64;
}
static uint64_t solid_plain_bound(size_t n, const char *const *names, const uint64_t *src_len) {
    uint64_t plain = 0;
    for (size_t i = 0; i < n; i++) plain += frame_entry_prefix_bound(names ? names[i] : nullptr) + src_len[i] + 16;
    return plain;
}
extern "C" size_t pna_gpu_solid_archive_bound(int algo, size_t n, const char *const *names, const uint64_t *src_len) {
    return solid_bound_of(algo, solid_plain_bound(n, names, src_len));
}

static size_t solid_enc_bound_of(size_t b, const pna_gpu_cipher *cipher);
extern "C" size_t pna_gpu_solid_archive_enc_bound(int algo, size_t n, const char *const *names, const uint64_t *src_len, const pna_gpu_cipher *cipher) {
    return solid_enc_bound_of(pna_gpu_solid_archive_bound(algo, n, names, src_len), cipher);
}
// What the entries that are not files, the metadata chunks and the chunk cut add to a bound whose per-entry terms treat every entry as a file (those
// terms cover FHED and FEND): the blobs, a link's target, a chunk frame per FDAT chunk of it
static size_t tree_bound_terms(size_t n, const pna_gpu_entry_meta *meta, uint32_t max_chunk_size, const pna_gpu_entry_kinds *kinds) {
    size_t b = 0; const uint64_t CH = chunk_limit(max_chunk_size);
    for (size_t i = 0; i < n; i++) {
        b += meta_len(meta, i);
        if (kinds && kinds->kind && kinds->kind[i] != PNA_KIND_FILE && kinds->kind[i] != PNA_KIND_DIRECTORY && kinds->link_len) b += kinds->link_len[i] + 12 * (size_t)(kinds->link_len[i] / CH + 1);
    }
    return b;
}
extern "C" size_t pna_gpu_archive_tree_bound(int algo, size_t n, const char *const *names, const uint64_t *src_len, const pna_gpu_cipher *cipher,
                                             const pna_gpu_entry_meta *meta, uint32_t max_chunk_size, const pna_gpu_entry_kinds *kinds) {
    return pna_gpu_archive_chunked_bound(algo, n, names, src_len, cipher, max_chunk_size) + tree_bound_terms(n, meta, max_chunk_size, kinds);
}
extern "C" size_t pna_gpu_solid_archive_tree_bound(int algo, size_t n, const char *const *names, const uint64_t *src_len, const pna_gpu_cipher *cipher,
                                                   const pna_gpu_entry_meta *meta, uint32_t max_chunk_size, const pna_gpu_entry_kinds *kinds) {
    uint64_t plain = solid_plain_bound(n, names, src_len) + tree_bound_terms(n, meta, max_chunk_size, kinds);
    if (max_chunk_size) for (size_t i = 0; i < n; i++) plain += 12 * (src_len[i] / chunk_limit(max_chunk_size) + 1);      // a file's further FDAT chunks
    size_t b = solid_bound_of(algo, plain);
    if (algo == PNA_ALGO_STORE) b += 12 * (size_t)(plain / chunk_limit(max_chunk_size) + 1);      // the stored stream itself is cut into SDAT chunks of max_chunk_size bytes
    return solid_enc_bound_of(b, cipher);
}
extern "C" int pna_gpu_create_archive_tree_device(pna_gpu_ctx *c, int algo, int level, size_t n, const char *const *names,
                                                  const void *d_src, const uint64_t *src_off, const uint64_t *src_len,
                                                  const pna_gpu_cipher *cipher, const pna_gpu_entry_meta *meta, uint32_t max_chunk_size, const pna_gpu_entry_kinds *kinds,
                                                  void *d_dst, size_t dst_cap, uint64_t *entry_off, uint64_t *archive_len, uint32_t part_flags, void *hip_stream) {
    return create_archive_device_impl(c, algo, level, n, names, d_src, src_off, src_len, cipher, meta, max_chunk_size, d_dst, dst_cap, entry_off, archive_len, part_flags, hip_stream, kinds);
}
extern "C" int pna_gpu_create_solid_archive_tree_device(pna_gpu_ctx *c, int algo, int level, size_t n, const char *const *names,
                                                        const void *d_src, const uint64_t *src_off, const uint64_t *src_len,
                                                        const pna_gpu_cipher *cipher, const pna_gpu_entry_meta *meta, uint32_t max_chunk_size, const pna_gpu_entry_kinds *kinds,
                                                        void *d_dst, size_t dst_cap, uint64_t *archive_len, void *hip_stream) {
    return create_solid_device_impl(c, algo, level, n, names, d_src, src_off, src_len, cipher, meta, max_chunk_size, kinds, d_dst, dst_cap, archive_len, hip_stream);
}
static size_t solid_enc_bound_of(size_t b, const pna_gpu_cipher *cipher) {
    if (!cipher || cipher->encryption == PNA_ENC_NONE) return b;
    b += 12 + (cipher->phsf ? strlen(cipher->phsf) : 0) + 12 + 75 + 64;          // PHSF chunk, the chunk of the IV / stream header
    if (cipher->cipher_mode == PNA_MODE_GCM) {
        const uint64_t seg = gcm_seg_size(cipher);
        b += 28 * (size_t)(b / seg + 2);                                            // tag + chunk framing per GCM segment
    }
    return b;
}

extern "C" int pna_gpu_create_solid_archive_device(pna_gpu_ctx *c, int algo, int level, size_t n, const char *const *names,
                                                   const void *d_src, const uint64_t *src_off, const uint64_t *src_len,
                                                   void *d_dst, size_t dst_cap, uint64_t *archive_len, void *hip_stream) {
    return pna_gpu_create_solid_archive_enc_device(c, algo, level, n, names, d_src, src_off, src_len, nullptr, d_dst, dst_cap, archive_len, hip_stream);
}

// With a cipher (CTR): SHED(encryption, cipher_mode) | PHSF | SDAT(iv) | SDAT(ciphertext)* | SEND -- into_solid_archive writes the PHSF
// chunk behind SHED and the IV as the first write of the SDAT stream (lib/src/archive/write.rs:443-470); one cipher stream runs over
// all SDAT bodies.  cipher->ivs: ONE 16-byte IV (or NULL).
extern "C" int pna_gpu_create_solid_archive_enc_device(pna_gpu_ctx *c, int algo, int level, size_t n, const char *const *names,
                                                       const void *d_src, const uint64_t *src_off, const uint64_t *src_len,
                                                       const pna_gpu_cipher *cipher, void *d_dst, size_t dst_cap, uint64_t *archive_len,
                                                       void *hip_stream) {
    return create_solid_device_impl(c, algo, level, n, names, d_src, src_off, src_len, cipher, nullptr, 0, nullptr, d_dst, dst_cap, archive_len, hip_stream);
}
// The stored solid stream (SHED compression 0): the serialised inner records ARE the stream, so nothing is compressed and nothing is copied twice -- the
// framing bytes go from one blob to their places in the destination's SDAT bodies (k_gather), k_store puts every inner payload at its place there and
// leaves its pieces' CRC registers, k_store_fold writes the inner FDAT CRCs and FEND.  The stream is cut into SDAT chunks of chunk_limit(max_chunk) bytes
// (the default: one chunk up to 2^32 - 5 bytes); stream position p stands at base + p + 12 (p / SCH), and a cut may fall anywhere -- into a payload (its
// pieces end there: the chunk folds by the piece list's lengths) or into a CRC field (the fold maps every byte).  With a cipher the stream is encrypted
// where it stands -- CTR: one keystream over the SDAT bodies; GCM STREAM: one SDAT chunk per segment, its tag behind it (28 bytes between two segments) --,
// and the SDAT CRCs are k_frame's over what stands there then.  For a stream of one chunk without a cipher the bytes are pna_create_archive's.
static int create_solid_store(pna_gpu_ctx *c, size_t n, const char *const *names, const void *d_src, const uint64_t *src_off, const uint64_t *src_len,
                              const pna_gpu_cipher *cipher, const uint8_t *ivs, const pna_gpu_entry_meta *meta, uint32_t max_chunk, const EntryRecords &recs,
                              void *d_dst, size_t dst_cap, uint64_t *archive_len, hipStream_t st) {
    const bool gcm = cipher && cipher->cipher_mode == PNA_MODE_GCM;
    const uint64_t G = gcm ? gcm_seg_size(cipher) : 0, CHI = chunk_limit(max_chunk);
    const uint64_t SCH = gcm ? G : chunk_limit(max_chunk), OVH = gcm ? 28 : 12;     // data bytes of an SDAT chunk, what stands between two chunks' data
    std::vector<uint8_t> head, tail, blob, tmp;
    solid_archive_head(head, PNA_ALGO_STORE, cipher, ivs);
    frame_solid_tail(tail); frame_archive_tail(tail);
    const uint64_t base = head.size() + 8;
    auto at = [&](uint64_t p) { return base + p + OVH * (p / SCH); };
    std::vector<PlaceDescH> lits; std::vector<StorePiece> pieces; std::vector<StoreChunk> chunks; std::vector<FrameDesc> units;
    uint64_t pos = 0;
    uint8_t fend[12] = {0, 0, 0, 0, 'F', 'E', 'N', 'D', 0, 0, 0, 0};
    put_be32(fend + 8, frame_fend_crc());
    auto lit = [&](const uint8_t *p, size_t nb) {            // framing bytes of the stream, cut where an SDAT chunk ends
        const size_t b0 = blob.size();
        blob.insert(blob.end(), p, p + nb);
        for (size_t o = 0; o < nb;) {
            const size_t k = (size_t)std::min<uint64_t>(std::min<uint64_t>(nb - o, SCH - pos % SCH), 0x40000000u);
            lits.push_back(PlaceDescH{b0 + o, at(pos), (uint32_t)k, 0}); pos += k; o += k;
        }
    };
    for (size_t i = 0; i < n; i++) {
        if (recs.count && recs.len(i)) { lit(recs.at(i), (size_t)recs.len(i)); continue; }
        const uint64_t len = src_len[i];
        tmp.clear();
        if (len == 0) { frame_inner_entry_empty(tmp, names[i]); splice_meta(tmp, meta, i); lit(tmp.data(), tmp.size()); continue; }
        for (uint64_t o = 0; o < len; o += CHI) {
            const uint64_t cl = std::min<uint64_t>(CHI, len - o);
            const bool last = o + cl == len;
            if (o == 0) { frame_entry_prefix(tmp, names[i], PNA_ALGO_STORE, len, (uint32_t)cl); splice_meta(tmp, meta, i); lit(tmp.data(), tmp.size()); }
            else { uint8_t h[8]; put_be32(h, (uint32_t)cl); memcpy(h + 4, "FDAT", 4); lit(h, 8); }
            if (pieces.size() + cl / STORE_PIECE + 2 > 0x7FFFFFF0ull || chunks.size() > 0x7FFFFFF0ull) return fail(c, PNA_E_INVAL, "too many data chunks");
            StoreChunk ch{0, cl, (uint32_t)pieces.size(), 0, last ? 1u : 0u, 0};
            bool regular = true;
            for (uint64_t q = 0; q < cl;) {
                const uint64_t k = std::min<uint64_t>(std::min<uint64_t>(cl - q, STORE_PIECE), SCH - pos % SCH);
                if (k != STORE_PIECE && q + k != cl) regular = false;      // an SDAT cut inside the chunk
                pieces.push_back(StorePiece{src_off[i] + o + q, at(pos), (uint32_t)k, 0}); pos += k; q += k;
            }
            ch.npieces = (uint32_t)pieces.size() - ch.first; ch.crc_off = pos; if (!regular) ch.flags |= 2u;
            chunks.push_back(ch);
            pos += last ? 16 : 4;                            // the CRC [and FEND]: k_store_fold's bytes
        }
    }
    const uint64_t plain_len = pos;
    const uint64_t K = gcm ? (plain_len ? (plain_len + G - 1) / G : 1) : (plain_len + SCH - 1) / SCH;
    if (K > 0x7FFFFFF0ull) return fail(c, PNA_E_INVAL, gcm ? "GCM segment counter overflow" : "too many data chunks");
    SubLayout L;
    if (gcm) { L.gmat.resize(1); gcm_solid_material(cipher, ivs, PNA_ALGO_STORE, L.gmat[0]); }
    for (uint64_t k = 0; k < K; k++) {                       // the SDAT chunks: header, cipher units, k_frame's descriptor
        const uint64_t sl = std::min<uint64_t>(SCH, plain_len - k * SCH), hdr = base - 8 + k * (SCH + OVH), dl = sl + (gcm ? 16 : 0);
        uint8_t h[8]; put_be32(h, (uint32_t)dl); memcpy(h + 4, "SDAT", 4);
        lits.push_back(PlaceDescH{blob.size(), hdr, 8u, 0});
        units.push_back(FrameDesc{hdr, (uint32_t)dl, (uint32_t)blob.size(), 8u, 0});
        blob.insert(blob.end(), h, h + 8);
        if (gcm) {
            const uint32_t si = (uint32_t)(L.giv.size() / 16);
            GcmEntry ge{hdr + 8, (uint32_t)sl, 0, {0, 0, 0, 0}, {0, 0, 0, 0}};
            uint8_t iv[16];
            gcm_segment(L.gmat[0], (uint32_t)k, k + 1 == K, ge, iv);
            L.giv.insert(L.giv.end(), iv, iv + 16);
            L.gkeys.push(si, L.gmat[0].key);
            for (uint64_t o = 0; o < sl; o += CTR_UNIT) L.cunits.push_back(CipherUnit{hdr + 8 + o, o, (uint32_t)std::min<uint64_t>(CTR_UNIT, sl - o), si});
            L.gents.push_back(ge);
        } else if (cipher)
            for (uint64_t o = 0; o < sl; o += CTR_UNIT) L.cunits.push_back(CipherUnit{hdr + 8 + o, k * SCH + o, (uint32_t)std::min<uint64_t>(CTR_UNIT, sl - o), 0u});
    }
    if (blob.size() > 0xFFFFFF00ull) return fail(c, PNA_E_INVAL, "the inner entries' framing exceeds 4 GiB");
    const uint64_t end = head.size() + plain_len + OVH * K;
    if (end + tail.size() + 16 > dst_cap) return fail(c, PNA_E_DSTSIZE, "device destination too small");
    const size_t np = pieces.size(), nl = lits.size(), nc = chunks.size(), nu = units.size();
    if (c->fr_blob.ensure(blob.size() + 16) || c->st_lits.ensure(nl * sizeof(PlaceDescH) + 16) || c->st_pieces.ensure(np * sizeof(StorePiece) + 16) ||
        c->st_chunks.ensure(nc * sizeof(StoreChunk) + 16) || c->st_states.ensure(np * 4 + 16) || c->fr_desc.ensure(nu * sizeof(FrameDesc) + 16))
        return fail(c, PNA_E_NOMEM, "stored workspace");
    int rc = ensure_crc(c); if (rc) return rc;
    for (auto &ev : c->st_ev) if (!ev) HIPCHK(c, hipEventCreate(&ev));
    uint8_t *dst = (uint8_t *)d_dst;
    c->timing = pna_gpu_timing{};
    c->st_fused = c->st_copy_only = c->st_folded = 0; c->st_ms = 0;
    HIPCHK(c, hipMemcpyAsync(dst, head.data(), head.size(), hipMemcpyHostToDevice, st));
    if (!blob.empty()) HIPCHK(c, hipMemcpyAsync(c->fr_blob.p, blob.data(), blob.size(), hipMemcpyHostToDevice, st));
    if (nl) HIPCHK(c, hipMemcpyAsync(c->st_lits.p, lits.data(), nl * sizeof(PlaceDescH), hipMemcpyHostToDevice, st));
    if (np) HIPCHK(c, hipMemcpyAsync(c->st_pieces.p, pieces.data(), np * sizeof(StorePiece), hipMemcpyHostToDevice, st));
    if (nc) HIPCHK(c, hipMemcpyAsync(c->st_chunks.p, chunks.data(), nc * sizeof(StoreChunk), hipMemcpyHostToDevice, st));
    if (nu) HIPCHK(c, hipMemcpyAsync(c->fr_desc.p, units.data(), nu * sizeof(FrameDesc), hipMemcpyHostToDevice, st));
    launch_gather(c->st_lits.p, (uint32_t)nl, (const uint8_t *)c->fr_blob.p, dst, st);
    HIPCHK(c, hipEventRecord(c->st_ev[0], st));
    launch_store(c->st_pieces.p, (uint32_t)np, (const uint8_t *)d_src, dst, (const CrcTabs *)c->crc_tabs.p, (uint32_t *)c->st_states.p, true, st);
    HIPCHK(c, hipEventRecord(c->st_ev[1], st));
    launch_store_fold(c->st_chunks.p, (uint32_t)nc, (const uint32_t *)c->st_states.p, c->st_pieces.p, "FDAT", frame_fend_crc(), dst, st, base, SCH, OVH);
    if (cipher) {
        const uint64_t zero = 0; uint64_t offs[2] = {0, 0};
        const FrameJob fj{nullptr, 1, cipher, ivs};
        const SubBatch sb{c, PNA_ALGO_STORE, (const uint8_t *)d_src, &zero, &plain_len, 0, 1, dst, dst_cap, head.size(), offs, st, false, &fj};
        rc = cipher_stage(sb, L); if (rc) return rc;
    }
    launch_frame((const FrameDesc *)c->fr_desc.p, (uint32_t)nu, (const uint8_t *)c->fr_blob.p, (const CrcTabs *)c->crc_tabs.p, dst,
                 (uint64_t)(dst_cap - tail.size()) & ~(uint64_t)15, frame_fend_crc(), "SDAT", false, st, 0);
    HIPCHK(c, hipMemcpyAsync(dst + end, tail.data(), tail.size(), hipMemcpyHostToDevice, st));
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(st));
    float ms = 0; (void)hipEventElapsedTime(&ms, c->st_ev[0], c->st_ev[1]);
    c->st_ms = ms; c->st_fused = np; c->st_folded = nc;
    *archive_len = end + tail.size();
    uint64_t in_total = 0; for (size_t i = 0; i < n; i++) in_total += src_len[i];
    c->timing.in_bytes = in_total; c->timing.out_bytes = *archive_len;
    return PNA_OK;
}
// (the tree form: inner entries that are not files are finished records between the file records -- blob spans, "without a data chunk" for k_frame --, files carry
// their metadata chunks and are cut into FDAT chunks of max_chunk bytes: every inner entry of a solid stream is a stored record)
int create_solid_device_impl(pna_gpu_ctx *c, int algo, int level, size_t n, const char *const *names,
                             const void *d_src, const uint64_t *src_off, const uint64_t *src_len,
                             const pna_gpu_cipher *cipher, const pna_gpu_entry_meta *meta, uint32_t max_chunk, const pna_gpu_entry_kinds *kinds,
                             void *d_dst, size_t dst_cap, uint64_t *archive_len, void *hip_stream) {
    { int rcm = check_meta(c, meta, n); if (rcm) return rcm; }
    if (cipher && cipher->encryption == PNA_ENC_NONE) cipher = nullptr;
    std::vector<uint8_t> own_ivs;
    const uint8_t *ivs = nullptr;
    if (cipher) { int rc0 = resolve_ivs(c, cipher, 1, own_ivs, &ivs); if (rc0) return rc0; }
    if (cipher && cipher->cipher_mode == PNA_MODE_CBC) return fail(c, PNA_E_UNSUPPORTED, "solid archives: CTR and GCM on the device path (CBC encryption is one serial chain over the whole stream)");
    if (!c || !archive_len || (n && (!names || !src_off || !src_len)) || !d_dst) return fail(c, PNA_E_INVAL, "null argument");
    EntryRecords recs;
    { int rck = build_entry_records(c, n, names, src_len, kinds, meta, max_chunk, recs); if (rck) return rck; }
    if (!d_src && recs.count < n) return fail(c, PNA_E_INVAL, "null argument");
    const bool stored = algo == PNA_ALGO_STORE && launch_store && launch_store_fold;
    if (algo != PNA_ALGO_ZSTD && algo != PNA_ALGO_DEFLATE && !stored) return fail(c, PNA_E_UNSUPPORTED, algo == PNA_ALGO_XZ ? "xz is written by the batch and the non-solid archive entry points only (option xz_encode)" : "algorithm not implemented on the device path");
    if ((uintptr_t)d_dst & 15) return fail(c, PNA_E_INVAL, "archive buffer must be 16-byte aligned");
    set_call_level(c, algo, level);
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : c->stream;
    if (stored) {
        for (size_t i = 0; i < n; i++) if (!(recs.count && recs.len(i)) && (src_off[i] & 15)) return fail(c, PNA_E_INVAL, "entry offset not 16-byte aligned");
        return create_solid_store(c, n, names, d_src, src_off, src_len, cipher, ivs, meta, max_chunk, recs, d_dst, dst_cap, archive_len, st);
    }
    // ---- 1. layout of the serialised inner entries (all sizes are known up front)
    std::vector<FrameDesc> fds; std::vector<uint8_t> blob, tmp; std::vector<PlaceDescH> places;
    fds.reserve(n);
    // (without max_chunk an inner entry is ONE data chunk, below 2 GiB; with it, FlattenWriter's chunks -- lib/src/util/io.rs:60-77 --, a descriptor each)
    const uint64_t CH = max_chunk ? chunk_limit(max_chunk) : 0x7FFF0000ull;
    const bool cut = max_chunk != 0;
    uint64_t pos = 0, max_piece = 0;
    for (size_t i = 0; i < n; i++) if (!(recs.count && recs.len(i))) max_piece = std::max<uint64_t>(max_piece, std::min<uint64_t>(src_len[i], CH));
    const uint32_t solid_max_inner = max_piece <= 16380 ? (uint32_t)std::max<uint64_t>(max_piece, 1) : 0u;      // (stored inner entries: the FDAT payload is the entry; small ones take k_frame's wave-per-entry form)
    for (size_t i = 0; i < n; i++) {
        const size_t po = blob.size();
        if (recs.count && recs.len(i)) {
            blob.insert(blob.end(), recs.at(i), recs.at(i) + recs.len(i));
            fds.push_back(FrameDesc{pos, 0, (uint32_t)po, (uint32_t)recs.len(i), 1});
            pos += recs.len(i);
            continue;
        }
        if (src_off[i] & 15) return fail(c, PNA_E_INVAL, "entry offset not 16-byte aligned");
        if (!cut && src_len[i] >= CH) return fail(c, PNA_E_INVAL, "inner entry too large for one FDAT chunk");
        if (src_len[i] == 0) {
            if (!meta_len(meta, i)) frame_inner_entry_empty(blob, names[i]);
            else { tmp.clear(); frame_inner_entry_empty(tmp, names[i]); splice_meta(tmp, meta, i); blob.insert(blob.end(), tmp.begin(), tmp.end()); }
            fds.push_back(FrameDesc{pos, 0, (uint32_t)po, (uint32_t)(blob.size() - po), 1});
            pos += blob.size() - po;
            continue;
        }
        for (uint64_t o = 0; o < src_len[i]; o += CH) {
            const uint64_t cl = std::min<uint64_t>(CH, src_len[i] - o);
            const bool last = o + cl == src_len[i];
            const size_t pk = blob.size();
            if (o == 0 && !meta_len(meta, i)) frame_entry_prefix(blob, names[i], PNA_ALGO_STORE, src_len[i], (uint32_t)cl);
            else if (o == 0) { tmp.clear(); frame_entry_prefix(tmp, names[i], PNA_ALGO_STORE, src_len[i], (uint32_t)cl); splice_meta(tmp, meta, i); blob.insert(blob.end(), tmp.begin(), tmp.end()); }
            else { const uint8_t h[8] = {(uint8_t)(cl >> 24), (uint8_t)(cl >> 16), (uint8_t)(cl >> 8), (uint8_t)cl, 'F', 'D', 'A', 'T'}; blob.insert(blob.end(), h, h + 8); }
            const uint32_t pl = (uint32_t)(blob.size() - pk);
            fds.push_back(FrameDesc{pos, (uint32_t)cl, (uint32_t)pk, pl, last ? 0u : 2u});
            for (uint64_t k = 0; k < cl; k += SEG_SIZE)
                places.push_back(PlaceDescH{src_off[i] + o + k, pos + pl + k, (uint32_t)std::min<uint64_t>(SEG_SIZE, cl - k), 0});
            pos += pl + cl + (last ? 16 : 4);
        }
    }
    if (blob.size() > 0xFFFFFFFFull) return fail(c, PNA_E_INVAL, "the inner entries' framing exceeds 4 GiB");
    const size_t nfd = fds.size();
    const uint64_t plain_len = pos;
    if (c->solid_plain.ensure(plain_len + 8192) || c->solid_desc.ensure(nfd * sizeof(FrameDesc) + 16) || c->solid_blob.ensure(blob.size() + 16) ||
        c->solid_place.ensure(places.size() * sizeof(PlaceDescH) + 16)) return fail(c, PNA_E_NOMEM, "solid workspace");
    int rc = ensure_crc(c); if (rc) return rc;
    if (n) {
        HIPCHK(c, hipMemcpyAsync(c->solid_desc.p, fds.data(), nfd * sizeof(FrameDesc), hipMemcpyHostToDevice, st));
        HIPCHK(c, hipMemcpyAsync(c->solid_blob.p, blob.data(), blob.size(), hipMemcpyHostToDevice, st));
        if (!places.empty()) HIPCHK(c, hipMemcpyAsync(c->solid_place.p, places.data(), places.size() * sizeof(PlaceDescH), hipMemcpyHostToDevice, st));
        // (chunks cut by max_chunk start at any byte of their entry: k_gather takes any alignment on both sides, k_place wants 16-byte aligned sources)
        if (cut) launch_gather(c->solid_place.p, (uint32_t)places.size(), (const uint8_t *)d_src, (uint8_t *)c->solid_plain.p, st);
        else launch_place(c->solid_place.p, (uint32_t)places.size(), (const uint8_t *)d_src, (uint8_t *)c->solid_plain.p, st);
        launch_frame((const FrameDesc *)c->solid_desc.p, (uint32_t)nfd, (const uint8_t *)c->solid_blob.p, (const CrcTabs *)c->crc_tabs.p,
                     (uint8_t *)c->solid_plain.p, (uint64_t)c->solid_plain.cap & ~(uint64_t)15, frame_fend_crc(), "FDAT", true, st, solid_max_inner);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipStreamSynchronize(st));                     // the host vectors above are read by the async copies
    }
    // ---- 2 + 3. one entry -> SDAT chunks, between the fixed chunks
    c->timing = pna_gpu_timing{};
    std::vector<uint8_t> head, tail;
    solid_archive_head(head, algo, cipher, ivs);
    frame_solid_tail(tail); frame_archive_tail(tail);
    if (head.size() + tail.size() + 64 > dst_cap) return fail(c, PNA_E_DSTSIZE, "device destination too small");
    HIPCHK(c, hipMemcpyAsync(d_dst, head.data(), head.size(), hipMemcpyHostToDevice, st));
    const uint64_t off0 = 0, len0 = plain_len; uint64_t offs[2] = {0, 0};
    FrameJob fj{nullptr, 1, cipher, ivs};
    rc = run_subbatch(c, algo, (const uint8_t *)c->solid_plain.p, &off0, &len0, 0, 1, (uint8_t *)d_dst, dst_cap - tail.size(), head.size(), offs, st, true, &fj);
    if (rc) return rc;
    HIPCHK(c, hipMemcpyAsync((uint8_t *)d_dst + offs[1], tail.data(), tail.size(), hipMemcpyHostToDevice, st));
    HIPCHK(c, hipStreamSynchronize(st));
    *archive_len = offs[1] + tail.size();
    uint64_t in_total = 0; for (size_t i = 0; i < n; i++) in_total += src_len[i];
    c->timing.in_bytes = in_total; c->timing.out_bytes = *archive_len;
    return PNA_OK;
}

extern "C" int pna_gpu_debug_block(pna_gpu_ctx *c, uint32_t block, uint64_t *seqs, uint32_t cap_seqs, uint32_t *nseq,
                                   uint8_t *lits, uint32_t cap_lits, uint32_t *nlit) {
    if (!c || block >= c->last_nblk) return PNA_E_INVAL;
    HIPCHK(c, hipSetDevice(c->device));
    BlkInfo bi;
    HIPCHK(c, hipMemcpy(&bi, (BlkInfo *)c->blk.p + block, sizeof(bi), hipMemcpyDeviceToHost));
    if (nseq) *nseq = bi.nseq;
    if (nlit) *nlit = bi.nlit;
    if (seqs) HIPCHK(c, hipMemcpy(seqs, (uint64_t *)c->seqs.p + (size_t)block * seq_cap_of(c->last_blk_log), (size_t)std::min(cap_seqs, bi.nseq) * 8, hipMemcpyDeviceToHost));
    if (lits) HIPCHK(c, hipMemcpy(lits, (uint8_t *)c->lits.p + ((size_t)block << c->last_blk_log), std::min(cap_lits, bi.nlit), hipMemcpyDeviceToHost));
    return PNA_OK;
}

// ---------------------------------------------------------------------------------------------------------
// corpus tables (integer-only; same construction as the checker's corpus model, written independently here)
static uint64_t splitmix(uint64_t &s) {
    uint64_t z = (s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
static int ensure_corpus(pna_gpu_ctx *c) {
    if (c->corpus_ready) return PNA_OK;
    const int VOCAB = 50000, SLOT = 16, NPHRASE = 8192;
    static const uint16_t LCUM[26] = {817, 966, 1244, 1669, 2939, 3162, 3364, 3973, 4670, 4685, 4762, 5165, 5406,
                                      6081, 6832, 7025, 7035, 7634, 8267, 9173, 9449, 9547, 9783, 9798, 9995, 10000};
    std::vector<uint8_t> vocab((size_t)VOCAB * SLOT, 0); std::vector<uint64_t> cum(VOCAB); std::vector<uint32_t> phr((size_t)NPHRASE * 4, 0);
    uint64_t s = 0x504E41ull;
    for (int w = 0; w < VOCAB; w++) {
        uint64_t r = splitmix(s);
        int len = 2 + (int)((r & 0xFFFF) * 11 >> 16);
        if (w < 64) len = 2 + (int)((r & 0xFFFF) * 3 >> 16);
        else if (w < 1024) len = 3 + (int)((r & 0xFFFF) * 5 >> 16);
        uint8_t *slot = &vocab[(size_t)w * SLOT];
        slot[0] = (uint8_t)len;
        for (int i = 0; i < len; i++) { uint32_t x = (uint32_t)(splitmix(s) >> 33) % 10000u; int ch = 0; while (LCUM[ch] <= x) ch++; slot[1 + i] = (uint8_t)('a' + ch); }
    }
    uint64_t acc = 0;
    for (int k = 0; k < VOCAB; k++) { acc += (1ull << 40) / (uint64_t)(k + 1); cum[k] = acc; }
    auto draw = [&](uint64_t r, int n) {
        unsigned __int128 m = (unsigned __int128)r * cum[n - 1]; uint64_t x = (uint64_t)(m >> 64);
        int lo = 0, hi = n - 1; while (lo < hi) { int mid = (lo + hi) >> 1; if (cum[mid] > x) hi = mid; else lo = mid + 1; } return lo;
    };
    for (int p = 0; p < NPHRASE; p++) {
        uint64_t r = splitmix(s);
        phr[4 * p] = (uint32_t)(2 + (int)(r & 1));
        for (int i = 0; i < 3; i++) phr[4 * p + 1 + i] = (uint32_t)draw(splitmix(s), VOCAB);
    }
    if (c->c_vocab.ensure(vocab.size()) || c->c_cum.ensure(cum.size() * 8) || c->c_phr.ensure(phr.size() * 4)) return fail(c, PNA_E_NOMEM, "corpus tables");
    HIPCHK(c, hipMemcpy(c->c_vocab.p, vocab.data(), vocab.size(), hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(c->c_cum.p, cum.data(), cum.size() * 8, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(c->c_phr.p, phr.data(), phr.size() * 4, hipMemcpyHostToDevice));
    c->corpus_ready = true;
    return PNA_OK;
}

extern "C" int pna_bench_corpus_fill_device(pna_gpu_ctx *c, int kind, uint64_t first_file, uint64_t n_files, uint64_t file_len,
                                            uint64_t stride, void *d_dst, void *hip_stream) {
    if (!c || !d_dst || kind < 0 || kind > 4 || stride < file_len) return fail(c, PNA_E_INVAL, "bad corpus argument");
    HIPCHK(c, hipSetDevice(c->device));
    int rc = ensure_corpus(c); if (rc) return rc;
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : c->stream;
    launch_corpus(kind, first_file, n_files, file_len, stride, (const uint8_t *)c->c_vocab.p, (const uint64_t *)c->c_cum.p,
                  (const uint32_t *)c->c_phr.p, (uint8_t *)d_dst, st);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(st));
    return PNA_OK;
}

extern "C" int pna_gpu_debug_lz_stamps(pna_gpu_ctx *c, unsigned long long *out8) {
    if (!c || !out8) return PNA_E_INVAL;
    HIPCHK(c, hipSetDevice(c->device));
    lz_read_stamps(out8);
    return PNA_OK;
}

// The cipher stage's host side is a file of its own in this translation unit: whatever builds pna_host.cpp -- the library, the sanitizer build of the
// host code -- has it, under one list of sources.
#include "pna_cipher.cpp"
