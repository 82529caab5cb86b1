// pna_pipeline.cpp -- the host-memory create pipelines of libpna_gpu.so: bounded staging || H2D || kernels || D2H (pna_gpu_create_archive_host and its
// forms, solid, multi-context, append, zero-staging host slots) and pna_gpu_compress_batch from host buffers.  Each pipeline is a row of stages over a
// call struct (what the stages share) and a plan; thread counts, parallel copies, copy streams, sink calls and slot reservation come from pna_ctx.h.
//   solid_stream (pna_gpu_create_solid_archive[_enc]_host in windows): solid_layout -> solid_sizes (window sizes, slots) -> per window: SolidAssembler::assemble
//     (on a thread beside the window before) -> solid_window_in (H2D, the pieces' CRC registers, chaining, patches) -> solid_window_compress (kernels, D2H, sink).
//   create_archive_host_impl (pna_gpu_create_archive_host and its forms): create_check -> capacity_terms -> cut_subbatches -> reserve_create_slots ->
//     Stager (lend_subbatch / stage_subbatch on its thread) || drain_subbatches (kernels, copy_out, hand_over of the sub-batch before) -> create_finish.
//   pna_gpu_compress_batch: cut_pieces -> BatchRun::stage(k + 1) || BatchRun::compress(k) || BatchRun::scatter(k - 1); BatchRun::drain on an error exit.
#include "pna_ctx.h"
#include <memory>

// `pna create --solid` from host memory (SolidArchive::add_entry streams the entries into ONE encoder, lib/src/archive/write.rs:575-580), zstd and deflate:
// the serialised inner entries -- FHED | fSIZ | FDAT(data, crc) | FEND per entry, stored -- reach the device in WINDOWS of solid_win_mib MiB of that stream
// (whole 1 MiB segments, every segment an SDAT chunk of its own), through two page-locked slots each way: ~4 windows of page-locked memory whatever the
// archive's size (round 4: the whole stream was staged, copied and held at once).  A window is planned as the whole stream (FrameJob::stream_len: the
// stream's block size and forms), so it is compressed exactly as it is inside the one-shot stream.  zstd: every segment is a frame.  deflate: the segments
// are runs of blocks that end in a sync flush, and only three things tie the zlib stream together -- the 78 9C header in front of the stream's first
// segment, BFINAL and the Adler-32 trailer on its last one, one Adler-32 over everything: the windows carry the segment flags of their place in the stream
// (FrameJob::run) and fold their blocks into the stream's Adler-32, which stays in device memory from window to window (k_dfold).  The host writes the
// chunk framing and the entries' bytes where they stand in the stream while the device compresses the window before; the data chunks' CRC-32 are the
// device's -- the raw CRC register of every piece of a chunk inside the window (k_frame's piece mode), chained by the host with CRC(A || B) =
// x^(8|B|) CRC(A) + CRC(B) for a chunk that spans windows, written into the window (k_crc_patch) before it is compressed.  An inner entry is cut into
// FDAT chunks of at most 2^32 - 5 bytes like FlattenWriter's (lib/src/util/io.rs:60-77): any size goes through (the one-shot device path: below 2 GiB).
// The archive equals pna_gpu_create_solid_archive_device's byte for byte.  No entries, and zstd's single_frame option, keep the one-shot form below.
namespace {
struct SolidSpan { uint64_t pos, len; uint32_t kind; uint32_t chunk; uint64_t a, b; };     // kind 0: blob[a ..), 1: entry a from byte b on, 2: the CRC of chunk `chunk`
struct SolidChunk { uint32_t state = 0, crc = 0; uint64_t end = 0; bool started = false, done = false; };   // end: stream position behind the chunk's data
struct SolidLayout { std::vector<uint8_t> blob; std::vector<SolidSpan> spans; std::vector<SolidChunk> chunks; uint64_t plain_len = 0; };
// what a window's stages share: its pieces of data chunks, the CRC spans that are not known yet, its place [w0, w1) in the stream
struct SolidWin { std::vector<FrameDesc> pieces; std::vector<uint32_t> piece_chunk; std::vector<uint64_t> piece_len; std::vector<uint32_t> crc_spans; uint64_t w0 = 0, w1 = 0; };
struct SolidRun {
    pna_gpu_ctx *c; int algo; const pna_gpu_cipher *cipher; const uint8_t *ivs; pna_sink_fn sink; void *user;
    SolidLayout L; SolidCipherRun crun;
    uint32_t max_chunk = 0; SolidStoreRun srun;                                               // PNA_ALGO_STORE: the stream's SDAT cut, the window's place and the open chunk's CRC register
    uint64_t W = 0, nwin = 0, wcap_in = 0, wcap_out = 0, slot_in = 0, slot_out = 0;          // window bytes, windows, a window's room each way, the device slots' stride
    uint8_t *d_in(uint64_t k) const { return (uint8_t *)c->stage_in.p + (k & 1) * slot_in; }
    uint8_t *d_out(uint64_t k) const { return (uint8_t *)c->stage_out.p + (k & 1) * slot_out; }
};
// ---- assemble window k in its page-locked slot: framing bytes, entry bytes, the CRCs that are known; the pieces of data chunks inside it
struct SolidAssembler {
    const SolidRun &r; const void *const *src; unsigned threads;
    size_t cursor = 0;                                                                         // first span that reaches into the window
    void assemble(uint64_t k, SolidWin &w) {
        const SolidLayout &L = r.L;
        w.pieces.clear(); w.piece_chunk.clear(); w.piece_len.clear(); w.crc_spans.clear();
        w.w0 = k * r.W; w.w1 = std::min(L.plain_len, w.w0 + r.W);
        uint8_t *slot = (uint8_t *)r.c->hp_in[k & 1].p;
        std::vector<CopyJob> jobs;
        while (cursor < L.spans.size() && L.spans[cursor].pos + L.spans[cursor].len <= w.w0) cursor++;
        for (size_t j = cursor; j < L.spans.size() && L.spans[j].pos < w.w1; j++) {
            const SolidSpan &sp = L.spans[j];
            const uint64_t a = std::max(sp.pos, w.w0), b = std::min(sp.pos + sp.len, w.w1);
            if (a >= b) continue;
            uint8_t *d = slot + (a - w.w0);
            if (sp.kind == 0) memcpy(d, L.blob.data() + sp.a + (a - sp.pos), b - a);
            else if (sp.kind == 1) {
                const uint8_t *sbase = (const uint8_t *)src[sp.a] + sp.b + (a - sp.pos);
                for (uint64_t o = 0; o < b - a; o += (8u << 20)) jobs.push_back(CopyJob{d + o, sbase + o, std::min<uint64_t>(8u << 20, b - a - o)});
                w.pieces.push_back(FrameDesc{a - w.w0, (uint32_t)(b - a), 0u, 0u, 4u | (a == sp.pos ? 0u : 8u)});
                w.piece_chunk.push_back(sp.chunk); w.piece_len.push_back(b - a);
            } else {
                const SolidChunk &cc = L.chunks[sp.chunk];
                if (cc.done) for (uint64_t q = a; q < b; q++) slot[q - w.w0] = (uint8_t)(cc.crc >> (24 - 8 * (q - sp.pos)));
                else { memset(d, 0, b - a); w.crc_spans.push_back((uint32_t)j); }
            }
        }
        if (w.w1 - w.w0 < r.wcap_in) memset(slot + (w.w1 - w.w0), 0, std::min<uint64_t>(64, r.wcap_in - (w.w1 - w.w0)));
        // entry bytes in jobs of at most 8 MiB, taken one by one by the threads: parallel_copy's fixed ranges measured 1.5 % slower on this path
        // (2 048 x 1 MiB: 87.6 against 86.2 ms, profiles/host_pipeline_stages_rate.txt), so the window keeps its own pool
        if (jobs.size() <= 1 || threads <= 1) { for (const CopyJob &jb : jobs) memcpy(jb.dst, jb.src, jb.len); return; }
        std::atomic<size_t> next{0};
        std::vector<std::thread> th;
        for (unsigned t = 0; t < std::min<size_t>(threads, jobs.size()); t++)
            th.emplace_back([&]() { for (size_t q; (q = next.fetch_add(1)) < jobs.size();) memcpy(jobs[q].dst, jobs[q].src, jobs[q].len); });
        for (auto &x : th) x.join();
    }
};
}
// ---- the stream's layout
// (the tree form: `recs` holds the finished records of the inner entries that are not files -- blob spans like any framing bytes, which a window edge may cut
// anywhere --, `meta` the files' metadata chunks, max_chunk FlattenWriter's cut of their data)
static SolidLayout solid_layout(size_t n, const char *const *names, const size_t *src_len, const EntryRecords *recs = nullptr, const pna_gpu_entry_meta *meta = nullptr, uint32_t max_chunk = 0) {
    SolidLayout L;
    std::vector<uint8_t> &blob = L.blob;
    std::vector<uint8_t> tmp;
    const uint64_t CH = chunk_limit(max_chunk);
    uint64_t pos = 0;
    uint8_t fend[12] = {0, 0, 0, 0, 'F', 'E', 'N', 'D', 0, 0, 0, 0};
    { const uint32_t fc = frame_fend_crc(); fend[8] = (uint8_t)(fc >> 24); fend[9] = (uint8_t)(fc >> 16); fend[10] = (uint8_t)(fc >> 8); fend[11] = (uint8_t)fc; }
    auto lit = [&](size_t from) { const uint64_t l = blob.size() - from; L.spans.push_back(SolidSpan{pos, l, 0u, 0u, (uint64_t)from, 0}); pos += l; };
    for (size_t i = 0; i < n && L.chunks.size() <= 0x7FFFFFF0u; i++) {                         // (more chunks than that: refused by the caller)
        const size_t b0 = blob.size();
        if (recs && recs->len(i)) { blob.insert(blob.end(), recs->at(i), recs->at(i) + recs->len(i)); lit(b0); continue; }
        const bool with_meta = meta_len(meta, i) != 0;
        if (src_len[i] == 0 && !with_meta) { frame_inner_entry_empty(blob, names[i]); lit(b0); continue; }
        if (src_len[i] == 0) { tmp.clear(); frame_inner_entry_empty(tmp, names[i]); splice_meta(tmp, meta, i); blob.insert(blob.end(), tmp.begin(), tmp.end()); lit(b0); continue; }
        const uint64_t len = src_len[i];
        for (uint64_t o = 0; o < len; o += CH) {
            const uint64_t cl = std::min<uint64_t>(CH, len - o);
            const size_t b1 = blob.size();
            if (o == 0 && !with_meta) frame_entry_prefix(blob, names[i], PNA_ALGO_STORE, len, (uint32_t)cl);
            else if (o == 0) { tmp.clear(); frame_entry_prefix(tmp, names[i], PNA_ALGO_STORE, len, (uint32_t)cl); splice_meta(tmp, meta, i); blob.insert(blob.end(), tmp.begin(), tmp.end()); }
            else { const uint8_t h[8] = {(uint8_t)(cl >> 24), (uint8_t)(cl >> 16), (uint8_t)(cl >> 8), (uint8_t)cl, 'F', 'D', 'A', 'T'}; blob.insert(blob.end(), h, h + 8); }
            lit(b1);
            const uint32_t ci = (uint32_t)L.chunks.size();
            L.chunks.emplace_back();
            L.spans.push_back(SolidSpan{pos, cl, 1u, ci, (uint64_t)i, o}); pos += cl;
            L.chunks[ci].end = pos;
            L.spans.push_back(SolidSpan{pos, 4, 2u, ci, 0, 0}); pos += 4;
        }
        const size_t b2 = blob.size();
        blob.insert(blob.end(), fend, fend + 12); lit(b2);
    }
    L.plain_len = pos;
    return L;
}
// ---- window sizes, the two slots each way (page-locked and device), the workspaces that live from window to window
static int solid_sizes(SolidRun &r) {
    pna_gpu_ctx *c = r.c;
    const bool gcm = r.cipher && r.cipher->cipher_mode == PNA_MODE_GCM;
    const uint64_t G = gcm ? gcm_seg_size(r.cipher) : 0, plain_len = r.L.plain_len;
    r.W = std::max<uint64_t>(1, (uint64_t)c->tun.solid_win_mib) << 20;                        // a multiple of SEG_SIZE
    const bool stored = r.algo == PNA_ALGO_STORE;
    if (stored && gcm) r.W = std::max<uint64_t>(G, r.W - r.W % G);                            // stored GCM STREAM: windows of whole segments (the stream's length is known: no carry)
    r.nwin = (plain_len + r.W - 1) / r.W;
    r.wcap_in = std::min<uint64_t>(r.W, plain_len) + 8192;
    r.wcap_out = pna_gpu_bound(r.algo, (size_t)std::min<uint64_t>(r.W, plain_len)) + (std::min<uint64_t>(r.W, plain_len) / SEG_SIZE + 2) * 16 + 4096;
    if (gcm) r.wcap_out += G + 28 * ((r.wcap_out + G) / G + 2);    // GCM: the carry in front, a tag and SDAT framing per segment
    if (stored && !gcm) r.wcap_out += 12 * (std::min<uint64_t>(r.W, plain_len) / chunk_limit(r.max_chunk) + 2);   // stored: SDAT framing per max_chunk bytes of the window
    int rc = ensure_crc(c); if (rc) return rc;
    r.slot_in = (r.wcap_in + 255) & ~(uint64_t)255; r.slot_out = (r.wcap_out + 255) & ~(uint64_t)255;   // the two device slots each way
    rc = Reserve{c}.add(c->stage_in, 2 * r.slot_in + 64).add(c->stage_out, 2 * r.slot_out + 64).add(c->hp_in, 2, r.wcap_in).add(c->hp_out, 2, r.wcap_out).done();
    if (rc) return rc;
    if (r.algo == PNA_ALGO_DEFLATE && c->solid_adler.ensure(64)) return fail(c, PNA_E_NOMEM, "solid workspace");   // the stream's Adler-32 (A, B) between windows
    if (gcm && c->solid_carry.ensure(G + 64)) return fail(c, PNA_E_NOMEM, "solid workspace");              // the GCM carry between windows
    r.crun.carry = (uint8_t *)c->solid_carry.p;
    return PNA_OK;
}
// ---- window k to the device and its CRC step: the raw CRC registers of its pieces to the host, chained into their chunks' (crc_gf2_mulmod / crc_gf2_xpow),
// the CRCs that are complete now patched into the window.  An error exit leaves the window's H2D copy and kernels on the stream: solid_stream waits for them.
static int solid_window_in(SolidRun &r, uint64_t k, const SolidWin &w) {
    pna_gpu_ctx *c = r.c; hipStream_t st = c->stream;
    DevBuf &dp = c->solid_place, &dd = c->solid_desc;                                          // patches, piece descriptors + states
    const uint64_t wl = w.w1 - w.w0;
    uint8_t *d_in = r.d_in(k);
    HIPCHK(c, hipMemcpyAsync(d_in, c->hp_in[k & 1].p, wl + std::min<uint64_t>(64, r.wcap_in - wl), hipMemcpyHostToDevice, st));
    const size_t np = w.pieces.size();
    std::vector<uint32_t> states(np);
    if (np) {
        if (dd.ensure(np * (sizeof(FrameDesc) + 4) + 64)) return fail(c, PNA_E_NOMEM, "solid workspace");
        uint32_t *d_states = (uint32_t *)((uint8_t *)dd.p + np * sizeof(FrameDesc));
        HIPCHK(c, hipMemcpyAsync(dd.p, w.pieces.data(), np * sizeof(FrameDesc), hipMemcpyHostToDevice, st));
        launch_frame_pieces((const FrameDesc *)dd.p, (uint32_t)np, (const CrcTabs *)c->crc_tabs.p, d_in, r.wcap_in & ~(uint64_t)15, "FDAT", d_states, st);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipMemcpyAsync(states.data(), d_states, np * 4, hipMemcpyDeviceToHost, st));
    }
    HIPCHK(c, hipStreamSynchronize(st));
    for (size_t q = 0; q < np; q++) {
        SolidChunk &cc = r.L.chunks[w.piece_chunk[q]];
        cc.state = cc.started ? (crc_gf2_mulmod(crc_gf2_xpow(8 * w.piece_len[q]), cc.state) ^ states[q]) : states[q];
        cc.started = true;
        if (w.w0 + w.pieces[q].arc_off + w.piece_len[q] == cc.end) { cc.crc = ~cc.state; cc.done = true; }
    }
    std::vector<CrcPatchH> patches;
    for (uint32_t j : w.crc_spans) {
        const SolidSpan &sp = r.L.spans[j];
        const SolidChunk &cc = r.L.chunks[sp.chunk];
        if (!cc.done) return fail(c, PNA_E_INVAL, "internal: a chunk's CRC is due before its data is through");
        uint32_t mask = 0;
        for (int q = 0; q < 4; q++) if (sp.pos + q >= w.w0 && sp.pos + q < w.w1) mask |= 1u << q;
        patches.push_back(CrcPatchH{(int64_t)sp.pos - (int64_t)w.w0, cc.crc, mask});
    }
    if (!patches.empty()) {
        if (dp.ensure(patches.size() * sizeof(CrcPatchH) + 64)) return fail(c, PNA_E_NOMEM, "solid workspace");
        HIPCHK(c, hipMemcpyAsync(dp.p, patches.data(), patches.size() * sizeof(CrcPatchH), hipMemcpyHostToDevice, st));
        launch_crc_patch(dp.p, (uint32_t)patches.size(), d_in, st);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipStreamSynchronize(st));                                                   // (`patches` is read by the copy)
    }
    return PNA_OK;
}
// ---- compress window k and hand it back; the next window is assembled on a thread of its own while the device compresses this one.  Every exit has joined
// that thread; an error exit may leave kernels or the D2H copy on the stream: solid_stream waits for them.
static int solid_window_compress(SolidRun &r, uint64_t k, const SolidWin &w, SolidAssembler &as, SolidWin &next_win) {
    pna_gpu_ctx *c = r.c; hipStream_t st = c->stream;
    struct Joined { std::thread t; ~Joined() { if (t.joinable()) t.join(); } } next;
    if (k + 1 < r.nwin) next.t = std::thread([&, k]() { as.assemble(k + 1, next_win); });
    const uint64_t off0 = 0, len0 = w.w1 - w.w0; uint64_t offs[2] = {0, 0};
    FrameJob fj{nullptr, 1, r.cipher, r.ivs};
    fj.stream_len = r.L.plain_len;
    if (r.cipher) { r.crun.final_win = k + 1 == r.nwin; fj.crun = &r.crun; }
    if (r.algo == PNA_ALGO_STORE) { fj.max_chunk = r.max_chunk; fj.srun = &r.srun; }
    if (r.algo == PNA_ALGO_DEFLATE) { fj.run = (k > 0 ? DRUN_CONT : 0u) | (k + 1 < r.nwin ? DRUN_OPEN : 0u); fj.adler_carry = (uint32_t *)c->solid_adler.p; }
    int rc = run_subbatch(c, r.algo, r.d_in(k), &off0, &len0, 0, 1, r.d_out(k), r.wcap_out, 0, offs, st, false, &fj);
    if (rc == PNA_OK && hipMemcpyAsync(c->hp_out[k & 1].p, r.d_out(k), offs[1], hipMemcpyDeviceToHost, st) != hipSuccess) rc = fail(c, PNA_E_HIP, "D2H copy failed");
    if (rc == PNA_OK && hipStreamSynchronize(st) != hipSuccess) rc = fail(c, PNA_E_HIP, "D2H copy failed");
    if (next.t.joinable()) next.t.join();
    return rc ? rc : sink_put(c, r.sink, r.user, c->hp_out[k & 1].p, (size_t)offs[1]);
}
// the tree arguments of the solid host forms (all NULL / 0: the plain forms)
struct SolidTree { const pna_gpu_entry_meta *meta = nullptr; uint32_t max_chunk = 0; const pna_gpu_entry_kinds *kinds = nullptr; const EntryRecords *recs = nullptr; };
static int solid_stream(pna_gpu_ctx *c, int algo, int level, size_t n, const char *const *names, const void *const *src, const size_t *src_len,
                        const pna_gpu_cipher *cipher, const uint8_t *ivs, pna_sink_fn sink, void *user, const SolidTree &tree = SolidTree{}) {
    set_call_level(c, algo, level);
    SolidRun r{c, algo, cipher, ivs, sink, user, solid_layout(n, names, src_len, tree.recs, tree.meta, tree.max_chunk), {}};
    if (r.L.chunks.size() > 0x7FFFFFF0u) return fail(c, PNA_E_INVAL, "too many data chunks");
    r.max_chunk = tree.max_chunk;
    c->st_fused = c->st_copy_only = c->st_folded = 0; c->st_ms = 0;
    // the fixed chunks around the stream (GCM: the stream header is the stream's first SDAT chunk, as in the device form)
    std::vector<uint8_t> head, tail;
    solid_archive_head(head, algo, cipher, ivs);
    frame_solid_tail(tail); frame_archive_tail(tail);
    int rc = sink_put(c, sink, user, head.data(), head.size()); if (rc) return rc;
    if ((rc = solid_sizes(r))) return rc;
    const CallTotalScope call_total(c, r.L.plain_len);                                        // every window picks the block size of the whole stream
    SolidAssembler as{r, src, staging_threads(c)};
    SolidWin win[2];
    if (r.nwin) as.assemble(0, win[0]);
    for (uint64_t k = 0; k < r.nwin && rc == PNA_OK; k++) {
        rc = solid_window_in(r, k, win[k & 1]);
        if (rc == PNA_OK) rc = solid_window_compress(r, k, win[k & 1], as, win[(k + 1) & 1]);
    }
    if (rc) { (void)hipStreamSynchronize(c->stream); return rc; }                             // (no thread is left; what the window left on the stream is waited for: its slots are the next call's)
    return sink_put(c, sink, user, tail.data(), tail.size());                                 // (nothing in flight)
}

// Page-locked staging memory the context holds right now (the slots of the host pipelines; plan blobs and tables excluded): what tests/ pin the
// bounded-memory claims with.  Not a product path.
extern "C" uint64_t pna_gpu_debug_pinned_bytes(pna_gpu_ctx *c) {
    if (!c) return 0;
    uint64_t t = 0;
    for (auto &b : c->hp_in) t += b.cap;
    for (auto &b : c->hp_out) t += b.cap;
    for (auto &b : c->df_pin) t += b.cap;                       // pna diff's two slots
    return t;
}

// the entries of [e0, e1) into a page-locked buffer at off[e], on the staging threads (below 8 MiB: on the calling thread)
static void parallel_stage(uint8_t *dst, const void *const *src, const size_t *src_len, const uint64_t *off, size_t e0, size_t e1, unsigned threads) {
    parallel_copy(e1 - e0, threads, 8u << 20, [=](size_t i) { return CopyJob{dst + off[e0 + i], (const uint8_t *)src[e0 + i], src_len[e0 + i]}; });
}
// no entries, or zstd's single_frame option (an entry's segments form ONE frame): one H2D of the entries, the device path, one D2H of the archive, handed
// to the sink in pieces of at most 16 MiB
static int solid_one_shot(pna_gpu_ctx *c, int algo, int level, size_t n, const char *const *names, const void *const *src, const size_t *src_len,
                          const pna_gpu_cipher *cipher, pna_sink_fn sink, void *user, const SolidTree &tree = SolidTree{}) {
    std::vector<uint64_t> off(n + 1), len(n);
    uint64_t pos = 0;
    for (size_t i = 0; i < n; i++) { off[i] = pos; len[i] = src_len[i]; pos = (pos + src_len[i] + 15) & ~(uint64_t)15; }
    off[n] = pos;
    const size_t cap = pna_gpu_solid_archive_tree_bound(algo, n, names, len.data(), cipher, tree.meta, tree.max_chunk, tree.kinds);
    int rc = Reserve{c}.add(c->stage_in, pos + 8192).add(c->stage_out, cap + 64).add(c->hp_in[0], pos + 64).add(c->hp_out[0], cap + 64).done();
    if (rc) return rc;
    parallel_stage((uint8_t *)c->hp_in[0].p, src, src_len, off.data(), 0, n, staging_threads(c));
    if (pos) HIPCHK(c, hipMemcpyAsync(c->stage_in.p, c->hp_in[0].p, pos, hipMemcpyHostToDevice, c->stream));
    uint64_t total = 0;
    rc = create_solid_device_impl(c, algo, level, n, names, c->stage_in.p, off.data(), len.data(), cipher, tree.meta, tree.max_chunk, tree.kinds, c->stage_out.p, cap + 64, &total, nullptr);
    if (rc) return rc;
    HIPCHK(c, hipMemcpyAsync(c->hp_out[0].p, c->stage_out.p, total, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (uint64_t p = 0; p < total && rc == PNA_OK; p += (16u << 20))
        rc = sink_put(c, sink, user, (const uint8_t *)c->hp_out[0].p + p, (size_t)std::min<uint64_t>(16u << 20, total - p));
    return rc;
}
// PNA_ALGO_STORE on the solid host forms: the stored stream travels in windows like the compressed ones (store_solid_window, pna_host.cpp); no entries: the one-shot form
static bool solid_store_ok(int algo) { return algo == PNA_ALGO_STORE && launch_store && launch_store_fold; }
static bool solid_windowed(const pna_gpu_ctx *c, int algo, size_t n) {
    return n && c->tun.solid_win_mib > 0 && (algo == PNA_ALGO_DEFLATE || solid_store_ok(algo) || (algo == PNA_ALGO_ZSTD && !c->tun.single_frame));
}
extern "C" int pna_gpu_create_solid_archive_host(pna_gpu_ctx *c, int algo, int level, size_t n, const char *const *names,
                                                 const void *const *src, const size_t *src_len, pna_sink_fn sink, void *user) {
    if (!c || !sink || (n && (!names || !src || !src_len))) return fail(c, PNA_E_INVAL, "null argument");
    HIPCHK(c, hipSetDevice(c->device));
    if (solid_windowed(c, algo, n)) return solid_stream(c, algo, level, n, names, src, src_len, nullptr, nullptr, sink, user);
    return solid_one_shot(c, algo, level, n, names, src, src_len, nullptr, sink, user);
}
// The same with a cipher (into_solid_archive, lib/src/archive/write.rs:443-470): CTR -- one keystream over all SDAT bodies, continued from window to
// window at the stream offset of the window's first compressed byte; GCM STREAM -- segments cut from the whole compressed stream, each window holding
// back in device memory the tail that is not yet known to be a non-final segment (SolidCipherRun).  The archive equals
// pna_gpu_create_solid_archive_enc_device's for the same IV / salt.
extern "C" int pna_gpu_create_solid_archive_enc_host(pna_gpu_ctx *c, int algo, int level, size_t n, const char *const *names,
                                                     const void *const *src, const size_t *src_len, const pna_gpu_cipher *cipher,
                                                     pna_sink_fn sink, void *user) {
    if (!cipher || cipher->encryption == PNA_ENC_NONE) return pna_gpu_create_solid_archive_host(c, algo, level, n, names, src, src_len, sink, user);
    if (!c || !sink || (n && (!names || !src || !src_len))) return fail(c, PNA_E_INVAL, "null argument");
    std::vector<uint8_t> own_ivs;
    const uint8_t *ivs = nullptr;
    int rc = resolve_ivs(c, cipher, 1, own_ivs, &ivs); if (rc) return rc;
    if (cipher->cipher_mode == PNA_MODE_CBC) return fail(c, PNA_E_UNSUPPORTED, "solid archives: CTR and GCM on the device path (CBC encryption is one serial chain over the whole stream)");
    if (algo != PNA_ALGO_ZSTD && algo != PNA_ALGO_DEFLATE && !solid_store_ok(algo)) return fail(c, PNA_E_UNSUPPORTED, algo == PNA_ALGO_XZ ? "xz is written by the batch and the non-solid archive entry points only (option xz_encode)" : "algorithm not implemented on the device path");
    HIPCHK(c, hipSetDevice(c->device));
    pna_gpu_cipher ci = *cipher; ci.ivs = ivs;                  // (IVs drawn here: the one-shot form must not draw others)
    if (solid_windowed(c, algo, n)) return solid_stream(c, algo, level, n, names, src, src_len, &ci, ivs, sink, user);
    return solid_one_shot(c, algo, level, n, names, src, src_len, &ci, sink, user);
}

// The tree form (pna_gpu.h "ENTRY KINDS"): directories and links stand between the file records of the inner stream
extern "C" int pna_gpu_create_solid_archive_tree_host(pna_gpu_ctx *c, int algo, int level, size_t n, const char *const *names,
                                                      const void *const *src, const size_t *src_len, const pna_gpu_cipher *cipher,
                                                      const pna_gpu_entry_meta *meta, uint32_t max_chunk_size, const pna_gpu_entry_kinds *kinds,
                                                      pna_sink_fn sink, void *user) {
    { int rcm = check_meta(c, meta, n); if (rcm) return rcm; }
    if (!c || !sink || (n && (!names || !src || !src_len))) return fail(c, PNA_E_INVAL, "null argument");
    if (cipher && cipher->encryption == PNA_ENC_NONE) cipher = nullptr;
    EntryRecords recs;
    { int rck = build_entry_records(c, n, names, (const uint64_t *)src_len, kinds, meta, max_chunk_size, recs); if (rck) return rck; }
    std::vector<uint8_t> own_ivs;
    const uint8_t *ivs = nullptr;
    pna_gpu_cipher ci{};
    if (cipher) {
        int rc = resolve_ivs(c, cipher, 1, own_ivs, &ivs); if (rc) return rc;
        if (cipher->cipher_mode == PNA_MODE_CBC) return fail(c, PNA_E_UNSUPPORTED, "solid archives: CTR and GCM on the device path (CBC encryption is one serial chain over the whole stream)");
        ci = *cipher; ci.ivs = ivs; cipher = &ci;               // (IVs drawn here: the one-shot form must not draw others)
    }
    if (algo != PNA_ALGO_ZSTD && algo != PNA_ALGO_DEFLATE && !solid_store_ok(algo)) return fail(c, PNA_E_UNSUPPORTED, algo == PNA_ALGO_XZ ? "xz is written by the batch and the non-solid archive entry points only (option xz_encode)" : "algorithm not implemented on the device path");
    HIPCHK(c, hipSetDevice(c->device));
    const SolidTree tree{meta, max_chunk_size, kinds, recs.count ? &recs : nullptr};
    if (solid_windowed(c, algo, n)) return solid_stream(c, algo, level, n, names, src, src_len, cipher, ivs, sink, user, tree);
    return solid_one_shot(c, algo, level, n, names, src, src_len, cipher, sink, user, tree);
}

// ---------------------------------------------------------------------------------------------------------
// Host-memory `pna create` (non-solid), bounded memory: the entries stream through two staging slots of at most
// ~1 GiB of input each.  While the GPU compresses and frames sub-batch k, helper threads stage sub-batch k+1 into
// page-locked memory and its H2D copy runs on a second stream; the archive bytes of sub-batch k-1 travel back on a
// third stream and are handed to the sink in one piece.  Replaces the reference's "every compressed entry in RAM until
// the scope ends" (cli/src/command/core.rs:496-537, create.rs:575-635) with a fixed in-flight window.
// ---- zero-staging input (round 4).  cli/src/command/core.rs:889-913 write_from_path reads every file into memory the library could own: with
// pna_gpu_host_alloc the host gets PAGE-LOCKED buffers to read its files into (read_exact into the slot instead of fs::read into a Vec), and the create
// entry points send entries that lie in such a buffer to the device straight from there -- the pageable -> page-locked copy on eight host threads is gone,
// one thread issues the copies.  Any mix works: a batch with an entry elsewhere is staged as before.
extern "C" int pna_gpu_host_alloc(pna_gpu_ctx *c, size_t bytes, void **out) {
    if (!c || !out || !bytes) return fail(c, PNA_E_INVAL, "null argument");
    *out = nullptr;
    HIPCHK(c, hipSetDevice(c->device));
    void *p = nullptr;
    if (hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess) return fail(c, PNA_E_NOMEM, "page-locked allocation failed");
    { std::lock_guard<std::mutex> lk(c->lent_mu); c->lent.emplace_back((const uint8_t *)p, bytes); }
    *out = p;
    return PNA_OK;
}
extern "C" int pna_gpu_host_free(pna_gpu_ctx *c, void *p) {
    if (!c || !p) return fail(c, PNA_E_INVAL, "null argument");
    {
        std::lock_guard<std::mutex> lk(c->lent_mu);
        auto it = std::find_if(c->lent.begin(), c->lent.end(), [&](const std::pair<const uint8_t *, size_t> &b) { return b.first == (const uint8_t *)p; });
        if (it == c->lent.end()) return fail(c, PNA_E_INVAL, "not a buffer of pna_gpu_host_alloc");
        c->lent.erase(it);
    }
    (void)hipSetDevice(c->device);
    (void)hipHostFree(p);
    return PNA_OK;
}
static bool entries_all_lent(pna_gpu_ctx *c, const void *const *src, const size_t *src_len, size_t n) {
    std::lock_guard<std::mutex> lk(c->lent_mu);
    if (c->lent.empty() || !n) return false;
    // (on the host-loop threads: 10^6 entries against the registry were 4 ms on one; the registry does not change while the lock is held)
    const unsigned nt = host_loop_threads(n);
    std::vector<char> ok(nt, 1);
    par_ranges(n, nt, [&](unsigned t, size_t a, size_t b) {
        size_t hint = 0;
        for (size_t i = a; i < b; i++) {
            if (!src_len[i]) continue;
            const uint8_t *p = (const uint8_t *)src[i];
            bool in = false;
            for (size_t k = 0; k < c->lent.size() && !in; k++) {                        // (entries of one call mostly share a buffer: start with the last hit)
                const auto &bf = c->lent[(hint + k) % c->lent.size()];
                if (p >= bf.first && p + src_len[i] <= bf.first + bf.second) { in = true; hint = (hint + k) % c->lent.size(); }
            }
            if (!in) { ok[t] = 0; return; }
        }
    });
    for (char v : ok) if (!v) return false;
    return true;
}

namespace {
// ---- pna_gpu_create_archive_host in stages.  CreateCall: what the stages share; CreatePlan: the sub-batches and the per-entry arrays they are cut over
struct CreateCall {
    pna_gpu_ctx *c; int algo; size_t n; const char *const *names; const void *const *src; const size_t *src_len;
    const pna_gpu_cipher *cipher; const uint8_t *ivs; const pna_gpu_entry_meta *meta; uint32_t part_flags, max_chunk; pna_sink_fn sink; void *user;
    std::chrono::steady_clock::time_point t_entry, t0;          // PNA_TRACE: the call's start, the pipeline's start
    const pna_gpu_entry_kinds *kinds = nullptr; EntryRecords recs;      // the tree form: the records of the entries that are not files (built by create_check)
    void trace(const char *what, size_t k) const {
        if (c->tun.trace) fprintf(stderr, "[pna create] %8.3f ms  %s %zu\n", std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(), what, k);
    }
};
struct Sub { size_t e0, e1; uint64_t in_bytes, out_cap; };
struct CreatePlan {
    std::vector<Sub> subs; uint64_t *off, *len64, *ecap, *eoff;   // staging offsets, lengths, capacity terms, archive offsets of the entries (the context's arrays)
    uint64_t in_total = 0; bool all_lent = false;                // (then no page-locked staging of the library's own is needed, and no staging copy)
    uint64_t out_len[2] = {0, 0}, out_total = 0;                 // archive bytes in the two output slots, bytes handed to the sink
};
constexpr int NS = 4;                                            // input slots (page-locked staging + device buffer)
// ---- the stager: sub-batch i into slot i % NS as soon as sub-batch i - NS has left the device.  It owns its thread: the destructor stops and joins it, so no
// exit of the pipeline leaves it running (what it has issued on cp_in by then is the caller's to wait for).
struct Stager {
    const CreateCall &k; const CreatePlan &p;
    std::mutex mu; std::condition_variable cv;
    size_t staged = 0, freed = 0; int rc = PNA_OK; bool stop = false;      // sub-batches staged (copies issued) / sub-batches whose kernels are done
    const unsigned threads;
    std::thread th;
    Stager(const CreateCall &call, const CreatePlan &plan) : k(call), p(plan), threads(staging_threads(call.c)), th([this] { run(); }) {}
    ~Stager() { { std::lock_guard<std::mutex> lk(mu); stop = true; cv.notify_all(); } th.join(); }
    int wait_staged(size_t i) { std::unique_lock<std::mutex> lk(mu); cv.wait(lk, [&] { return staged > i; }); return rc; }
    void release(size_t i) { std::lock_guard<std::mutex> lk(mu); freed = i + 1; cv.notify_all(); }        // sub-batch i's kernels are done: its input slot is free
  private:
    void give_up(int r) { std::lock_guard<std::mutex> lk(mu); rc = r; staged = p.subs.size(); cv.notify_all(); }
    // every entry lies in page-locked memory the library lent out (pna_gpu_host_alloc): no staging copy, the copy engine reads the host's
    // buffers themselves -- runs of entries that are contiguous there and here (16-byte stride) travel as ONE copy
    int lend_subbatch(const Sub &sb, uint8_t *db) const {
        const uint64_t *off = p.off;
        for (size_t g0 = sb.e0, g1; g0 < sb.e1; g0 = g1) {
            g1 = g0 + 1;
            while (g1 < sb.e1 && (const uint8_t *)k.src[g1] == (const uint8_t *)k.src[g0] + (off[g1] - off[g0])) g1++;
            const uint64_t bytes = (g1 < sb.e1 ? off[g1] : off[g1 - 1] + k.src_len[g1 - 1]) - off[g0];
            const uint64_t nb = std::min<uint64_t>(bytes, (const uint8_t *)k.src[g1 - 1] + k.src_len[g1 - 1] - (const uint8_t *)k.src[g0]);
            if (nb && hipMemcpyAsync(db + off[g0], k.src[g0], nb, hipMemcpyHostToDevice, k.c->cp_in) != hipSuccess) return PNA_E_HIP;
        }
        return PNA_OK;
    }
    // entries in pageable memory: groups of ~128 MiB into the slot's page-locked buffer on the staging threads, each group's H2D copy right behind it
    int stage_subbatch(const Sub &sb, uint8_t *hb, uint8_t *db) const {
        for (size_t g0 = sb.e0, g1; g0 < sb.e1; g0 = g1) {
            uint64_t acc = 0;
            for (g1 = g0; g1 < sb.e1 && acc < (128ull << 20);) acc += k.src_len[g1++];
            parallel_stage(hb, k.src, k.src_len, p.off, g0, g1, threads);
            const uint64_t b0 = p.off[g0], b1 = g1 < sb.e1 ? p.off[g1] : sb.in_bytes;
            if (b1 > b0 && hipMemcpyAsync(db + b0, hb + b0, b1 - b0, hipMemcpyHostToDevice, k.c->cp_in) != hipSuccess) return PNA_E_HIP;
        }
        return PNA_OK;
    }
    void run() {
        pna_gpu_ctx *c = k.c;
        try {
            if (hipSetDevice(c->device) != hipSuccess) { give_up(PNA_E_HIP); return; }
            for (size_t i = 0; i < p.subs.size(); i++) {
                {
                    std::unique_lock<std::mutex> lk(mu);
                    cv.wait(lk, [&] { return stop || i < freed + NS; });
                    if (stop) return;
                }
                const int sl = (int)(i % NS);
                int r = p.all_lent ? lend_subbatch(p.subs[i], (uint8_t *)c->dp_in[sl].p) : stage_subbatch(p.subs[i], (uint8_t *)c->hp_in[sl].p, (uint8_t *)c->dp_in[sl].p);
                if (r == PNA_OK && hipEventRecord(c->ev_in[sl], c->cp_in) != hipSuccess) r = PNA_E_HIP;
                k.trace("staged + H2D issued", i);
                if (r != PNA_OK) { give_up(r); return; }
                std::lock_guard<std::mutex> lk(mu);
                staged = i + 1; cv.notify_all();
            }
        } catch (...) { give_up(PNA_E_NOMEM); }
    }
};
}
// ---- check and resolve: arguments, metadata, algorithm, level, IVs; the device, the copy streams
static int create_check(CreateCall &k, int level, std::vector<uint8_t> &own_ivs) {
    pna_gpu_ctx *c = k.c;
    { int rcm = check_meta(c, k.meta, k.n); if (rcm) return rcm; }
    if (!c || !k.sink || (k.n && (!k.names || !k.src || !k.src_len))) return fail(c, PNA_E_INVAL, "null argument");
    { int rck = build_entry_records(c, k.n, k.names, (const uint64_t *)k.src_len, k.kinds, k.meta, k.max_chunk, k.recs); if (rck) return rck; }
    if (!encode_algo_ok(c, k.algo, true)) return fail(c, PNA_E_UNSUPPORTED, "algorithm not implemented on the device path");
    set_call_level(c, k.algo, level);
    if (k.cipher && k.cipher->encryption == PNA_ENC_NONE) k.cipher = nullptr;
    if (k.cipher) { int rc0 = resolve_ivs(c, k.cipher, k.n, own_ivs, &k.ivs); if (rc0) return rc0; }
    HIPCHK(c, hipSetDevice(c->device));
    return ensure_copy_lanes(c);
}
// ---- capacity terms: every entry's share of its sub-batch's output capacity (name length, worst-case payload, chunk framing): on the host-loop threads -- for
// 10^5 .. 10^6 small entries this loop, on one thread, was 8 .. 40 ms in front of the pipeline (a third of the end-to-end time of 10^6 x 4 KiB)
static void capacity_terms(const CreateCall &k, CreatePlan &p) {
    pna_gpu_ctx *c = k.c; const size_t n = k.n;
    // (the context keeps these arrays between calls: 10^6 entries are 24 MB, and fresh memory costs a page fault per 4 KiB -- milliseconds in front of the pipeline)
    if (c->pl_off.size() < n + 1) { c->pl_off.resize(n + 1); c->pl_len.resize(n + 1); c->pl_cap.resize(n + 1); }
    if (c->pl_eoff.size() < n + 1) c->pl_eoff.resize(n + 1);
    p.off = c->pl_off.data(); p.len64 = c->pl_len.data(); p.ecap = c->pl_cap.data(); p.eoff = c->pl_eoff.data();
    const unsigned plan_nt = host_loop_threads(n);
    std::vector<std::pair<uint64_t, uint64_t>> psum(plan_nt, {0, 0});         // (bytes, longest entry) per thread
    par_ranges(n, plan_nt, [&](unsigned t, size_t a, size_t b) {
        uint64_t tot = 0, mx = 0;
        for (size_t i = a; i < b; i++) {
            if (k.recs.count && k.recs.len(i)) { p.ecap[i] = k.recs.len(i); continue; }       // not a file: its record and nothing else
            const uint64_t l = k.src_len[i], wb = pna_gpu_bound(k.algo, (size_t)l);
            tot += l; mx = std::max(mx, l);
            uint64_t cap = (k.cipher ? frame_entry_prefix_enc_bound(k.names[i], k.cipher->phsf) + 16 : frame_entry_prefix_bound(k.names[i])) + meta_len(k.meta, i) + wb + 16;
            if (k.cipher && k.cipher->cipher_mode == PNA_MODE_GCM) cap += 16 * (wb / gcm_seg_size(k.cipher));   // a tag per full stream segment
            // a CRC + a header per further FDAT chunk once max_chunk_size cuts the payload (the term of pna_gpu_archive_chunked_bound: without it data
            // that does not compress overran the sub-batch's device buffer by 12 bytes per chunk -- PNA_E_DSTSIZE for a 2 MiB random entry at mcs = 1000)
            cap += 12 * (uint64_t)((wb + 64 + 16 * (l >> 12)) / chunk_limit(k.max_chunk) + 1);
            p.ecap[i] = cap;
        }
        psum[t] = {tot, mx};
    });
    uint64_t longest = 0;
    for (auto &q : psum) { p.in_total += q.first; longest = std::max(longest, q.second); }
    plan_call_longest(c, longest);
}
// ---- Sub-batches.  What bounds this path is the host link in the H2D direction (page-locked memory -> HBM: 56.8 GB/s on the MI355X boxes;
// experiments/link_duplex.hip, profiles/r03_c_link_duplex.txt) -- the kernels take a sixth of that time, the archive bytes going back a third of the
// volume and the link is full duplex.  So the pipeline is built around ONE rule: the H2D copy engine never waits.
//   * a stager thread runs ahead through all sub-batches over a ring of four input slots (page-locked staging + device buffer): it copies
//     the entries of a sub-batch into the slot's page-locked buffer (several threads, groups of ~128 MiB) and issues each group's H2D copy
//     right behind it; it blocks only while all four slots are in use (a slot is free again when its sub-batch's kernels are done);
//   * the main thread takes the sub-batches in order: kernels on the context's stream, then the archive bytes of the sub-batch travel to
//     the host next to the following sub-batch's kernels and copies -- by a small copy KERNEL that stores into the page-locked buffer
//     (d2h_wgs workgroups: ~30 GB/s, which leaves the H2D engine its full rate; the runtime's own D2H copy ran as a blit kernel at 51 GB/s
//     and took 30 % off the H2D copies next to it) --, and are handed to the sink one sub-batch later;
//   * sub-batch sizes grow from 64 MiB to `sub_mib` (default 256 MiB) at the start: the first kernels start after 2 ms instead of 20, and
//     what is left to do when the last input byte has arrived is the work of one sub-batch.  256 MiB is the smallest size whose kernels
//     (1.2 ms of fixed costs + 1 ms per 85 MiB) keep up with its H2D copy (1 ms per 53 MiB); shrinking sizes at the end only makes the
//     kernels fall behind the copies (measured, LAB_LOG.md).
static void cut_subbatches(const CreateCall &k, CreatePlan &p) {
    pna_gpu_ctx *c = k.c;
    const uint64_t SUBMAX = (uint64_t)c->tun.sub_mib << 20, SUBMIN = std::min<uint64_t>(64ull << 20, SUBMAX);
    uint64_t target = SUBMIN;
    for (size_t e = 0; e < k.n;) {
        const uint64_t want = std::min(target, SUBMAX);
        Sub sb{e, e, 0, 64}; uint64_t pos = 0; size_t blocks = 0;
        while (sb.e1 < k.n) {
            const size_t i = sb.e1; const uint64_t l = k.src_len[i];
            const size_t nb = plan_blocks(c, l);
            if (i > sb.e0 && (pos + l > want || blocks + nb > c->max_blocks)) break;
            p.off[i] = pos; p.len64[i] = l; pos = (pos + l + 15) & ~(uint64_t)15; blocks += nb;
            sb.out_cap += p.ecap[i];
            sb.e1++;
        }
        sb.in_bytes = pos; p.subs.push_back(sb); e = sb.e1;
        target = std::min(SUBMAX, target * 2);
    }
}
// ---- slots sized once for the largest sub-batch (allocation of page-locked memory is slow: not inside the pipeline)
static int reserve_create_slots(const CreateCall &k, const CreatePlan &p) {
    pna_gpu_ctx *c = k.c;
    uint64_t max_in = 0, max_out = 0;
    for (const Sub &sb : p.subs) { max_in = std::max(max_in, sb.in_bytes); max_out = std::max(max_out, sb.out_cap); }
    const size_t ns_in = std::min<size_t>(NS, p.subs.size()), ns_out = std::min<size_t>(2, p.subs.size());
    return Reserve{c}.add(c->hp_in, p.all_lent ? 0 : ns_in, max_in + 8192).add(c->dp_in, ns_in, max_in + 8192).add(c->dp_out, ns_out, max_out + 64).add(c->hp_out, ns_out, max_out + 64).done();
}
// sub-batch `so`'s archive bytes from its device slot to its page-locked one on cp_out: by k_link_copy (option d2h_wgs) or the runtime's copy
static int copy_out(const CreateCall &k, const CreatePlan &p, int so, uint8_t *(&dev_view)[2]) {
    pna_gpu_ctx *c = k.c;
    const uint32_t d2h_wgs = (uint32_t)c->tun.d2h_wgs;
    bool ok = true;
    if (d2h_wgs && !dev_view[so]) ok = hipHostGetDevicePointer((void **)&dev_view[so], c->hp_out[so].p, 0) == hipSuccess;
    if (ok && d2h_wgs) { launch_link_copy((const uint8_t *)c->dp_out[so].p, dev_view[so], p.out_len[so], d2h_wgs, c->cp_out); ok = hipGetLastError() == hipSuccess; }
    else if (ok) ok = hipMemcpyAsync(c->hp_out[so].p, c->dp_out[so].p, p.out_len[so], hipMemcpyDeviceToHost, c->cp_out) == hipSuccess;
    if (!ok || hipEventRecord(c->ev_out[so], c->cp_out) != hipSuccess) return fail(c, PNA_E_HIP, "D2H copy failed");
    return PNA_OK;
}
// the archive bytes in output slot `so` (their copy has been waited for) -> sink
static int hand_over(const CreateCall &k, CreatePlan &p, int so) {
    const int rc = sink_put(k.c, k.sink, k.user, k.c->hp_out[so].p, p.out_len[so]);
    p.out_total += p.out_len[so];
    return rc;
}
// ---- the drain loop: the sub-batches in order -- kernels on the context's stream, the archive bytes on their way to the host (copy_out), the sub-batch
// before handed to the sink.  An error exit leaves copies and kernels in flight: the caller stops the stager, then waits for the device.
static int drain_subbatches(const CreateCall &k, CreatePlan &p, Stager &stager) {
    pna_gpu_ctx *c = k.c;
    FrameJob fj{k.names, 0, k.cipher, k.ivs, k.meta, k.max_chunk, false};
    if (k.recs.count) fj.recs = &k.recs;
    const CallTotalScope call_total(c, p.len64, k.n);                                               // (the block size follows the archive, not its sub-batches)
    uint8_t *dev_view[2] = {nullptr, nullptr};                   // device views of the page-locked output slots (the copy kernel's destination)
    for (size_t i = 0; i < p.subs.size(); i++) {
        const Sub &sb = p.subs[i]; const int sl = (int)(i % NS), so = (int)(i & 1);
        if (const int r = stager.wait_staged(i)) return fail(c, r, "staging / H2D copy failed");
        if (hipEventSynchronize(c->ev_in[sl]) != hipSuccess) return fail(c, PNA_E_HIP, "H2D copy failed");
        k.trace("H2D done, kernels start", i);
        int rc = run_subbatch(c, k.algo, (const uint8_t *)c->dp_in[sl].p, p.off, p.len64, sb.e0, sb.e1, (uint8_t *)c->dp_out[so].p, sb.out_cap + 64, 0, p.eoff, c->stream, true, &fj);
        stager.release(i);                                       // (run_subbatch has waited for its kernels: the input slot is free)
        k.trace("kernels done", i);
        if (rc == PNA_OK) { p.out_len[so] = p.eoff[sb.e1]; rc = copy_out(k, p, so, dev_view); }
        if (rc == PNA_OK && i > 0) {                             // archive bytes of the previous sub-batch -> sink
            if (hipEventSynchronize(c->ev_out[so ^ 1]) != hipSuccess) return fail(c, PNA_E_HIP, "D2H copy failed");
            rc = hand_over(k, p, so ^ 1);
        }
        if (rc) return rc;
    }
    return PNA_OK;
}
// ---- finish: the last sub-batch, the tail, the call's totals.  Its copy has been waited for when the sink is called: nothing is in flight at these exits
static int create_finish(const CreateCall &k, CreatePlan &p, const std::vector<uint8_t> &tail) {
    pna_gpu_ctx *c = k.c;
    int rc = PNA_OK;
    if (!p.subs.empty()) {
        const int so = (int)((p.subs.size() - 1) & 1);
        HIPCHK(c, hipEventSynchronize(c->ev_out[so]));
        if ((rc = hand_over(k, p, so))) return rc;
    }
    if ((rc = sink_put(c, k.sink, k.user, tail.data(), tail.size()))) return rc;
    p.out_total += tail.size();
    k.trace("all bytes handed to the sink", 0);
    c->timing.in_bytes = p.in_total; c->timing.out_bytes = p.out_total;
    return PNA_OK;
}
static int create_archive_host_impl(pna_gpu_ctx *c, int algo, int level, size_t n, const char *const *names,
                                    const void *const *src, const size_t *src_len, const pna_gpu_cipher *cipher,
                                    const pna_gpu_entry_meta *meta, uint32_t part_flags, pna_sink_fn sink, void *user, uint32_t max_chunk,
                                    const pna_gpu_entry_kinds *kinds = nullptr) {
    using clk = std::chrono::steady_clock;
    auto ms = [](clk::time_point a, clk::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
    CreateCall k{c, algo, n, names, src, src_len, cipher, nullptr, meta, part_flags, max_chunk, sink, user, clk::now(), {}};
    k.kinds = kinds;
    std::vector<uint8_t> own_ivs;
    int rc = create_check(k, level, own_ivs); if (rc) return rc;
    c->timing = pna_gpu_timing{};
    c->st_fused = c->st_copy_only = c->st_folded = 0; c->st_ms = 0;
    std::vector<uint8_t> head, tail;
    if (part_flags & PNA_PART_HEAD) frame_archive_head(head, 0);
    if (part_flags & PNA_PART_TAIL) frame_archive_tail(tail);
    if ((rc = sink_put(c, sink, user, head.data(), head.size()))) return rc;
    CreatePlan p;
    p.out_total = head.size();
    capacity_terms(k, p);
    const auto t_caps = clk::now();
    cut_subbatches(k, p);
    const auto t_cut = clk::now();
    p.all_lent = entries_all_lent(c, src, src_len, n);
    if ((rc = reserve_create_slots(k, p))) return rc;
    k.t0 = clk::now();
    if (c->tun.trace) fprintf(stderr, "[pna create] planning took %.3f ms (capacity terms at %.3f, sub-batches cut at %.3f)\n", ms(k.t_entry, k.t0), ms(k.t_entry, t_caps), ms(k.t_entry, t_cut));
    k.trace("planned, slots ready; sub-batches:", p.subs.size());
    { Stager stager(k, p); rc = drain_subbatches(k, p, stager); }                             // (the stager is stopped and joined behind this line)
    k.trace("loop done", 0);
    if (rc != PNA_OK) { (void)hipDeviceSynchronize(); return rc; }                            // (nothing of this call is in flight when the error is returned)
    return create_finish(k, p, tail);
}

extern "C" int pna_gpu_create_archive_host(pna_gpu_ctx *c, int algo, int level, size_t n, const char *const *names,
                                           const void *const *src, const size_t *src_len, pna_sink_fn sink, void *user) {
    return pna_gpu_create_archive_enc_host(c, algo, level, n, names, src, src_len, nullptr, sink, user);
}
extern "C" int pna_gpu_create_archive_enc_host(pna_gpu_ctx *c, int algo, int level, size_t n, const char *const *names,
                                               const void *const *src, const size_t *src_len, const pna_gpu_cipher *cipher,
                                               pna_sink_fn sink, void *user) {
    return pna_gpu_create_archive_meta_host(c, algo, level, n, names, src, src_len, cipher, nullptr, sink, user);
}
extern "C" int pna_gpu_create_archive_meta_host(pna_gpu_ctx *c, int algo, int level, size_t n, const char *const *names,
                                                const void *const *src, const size_t *src_len, const pna_gpu_cipher *cipher,
                                                const pna_gpu_entry_meta *meta, pna_sink_fn sink, void *user) {
    return create_archive_host_impl(c, algo, level, n, names, src, src_len, cipher, meta, PNA_PART_HEAD | PNA_PART_TAIL, sink, user, c ? (uint32_t)c->tun.max_chunk_size : 0u);
}
extern "C" int pna_gpu_create_archive_chunked_host(pna_gpu_ctx *c, int algo, int level, size_t n, const char *const *names,
                                                   const void *const *src, const size_t *src_len, const pna_gpu_cipher *cipher,
                                                   const pna_gpu_entry_meta *meta, uint32_t max_chunk_size, uint32_t part_flags, pna_sink_fn sink, void *user) {
    return create_archive_host_impl(c, algo, level, n, names, src, src_len, cipher, meta, part_flags, sink, user, max_chunk_size);
}
extern "C" int pna_gpu_create_archive_tree_host(pna_gpu_ctx *c, int algo, int level, size_t n, const char *const *names,
                                                const void *const *src, const size_t *src_len, const pna_gpu_cipher *cipher,
                                                const pna_gpu_entry_meta *meta, uint32_t max_chunk_size, const pna_gpu_entry_kinds *kinds, uint32_t part_flags, pna_sink_fn sink, void *user) {
    return create_archive_host_impl(c, algo, level, n, names, src, src_len, cipher, meta, part_flags, sink, user, max_chunk_size, kinds);
}
extern "C" int pna_gpu_create_archive_part_host(pna_gpu_ctx *c, int algo, int level, size_t n, const char *const *names,
                                                const void *const *src, const size_t *src_len, uint32_t part_flags, pna_sink_fn sink, void *user) {
    return create_archive_host_impl(c, algo, level, n, names, src, src_len, nullptr, nullptr, part_flags, sink, user, c ? (uint32_t)c->tun.max_chunk_size : 0u);
}
// `pna append`: Archive::seek_to_end, then the new entries and AEND where the old AEND stood (cli/src/command/append.rs:504-560)
extern "C" int pna_gpu_append_archive_host(pna_gpu_ctx *c, int algo, int level, const void *archive, size_t archive_len, size_t n,
                                           const char *const *names, const void *const *src, const size_t *src_len, uint64_t *write_at,
                                           pna_sink_fn sink, void *user) {
    if (!c || !archive || !write_at || !sink) return fail(c, PNA_E_INVAL, "null argument");
    int has_next = 0;
    if (pna_archive_seek_to_end(archive, archive_len, write_at, &has_next) != PNA_OK) return fail(c, PNA_E_INVAL, "not a PNA archive, or truncated before its AEND chunk");
    if (has_next) return fail(c, PNA_E_INVAL, "the archive continues in another part (ANXT): append to its last part");
    return create_archive_host_impl(c, algo, level, n, names, src, src_len, nullptr, nullptr, PNA_PART_TAIL, sink, user, (uint32_t)c->tun.max_chunk_size);
}
// One process, several GPUs (SURVEY §8(b)'s `device_ids, n_devices`; §8(e)'s comparison path in C): the entries are cut into contiguous
// index ranges balanced by bytes, one per context (= per device), every context runs the bounded host pipeline on its range on a thread of
// its own (part flags: the first range carries the archive header, the last AEND) into host memory, and the parts reach the sink in index
// order -- the reference's fan-out + ordered drain (cli/src/command/core.rs:496-537,471-493) with devices in place of rayon workers and no
// device-to-device traffic at all.  Contexts may share a device (that is how the one-GPU boxes test it).
extern "C" int pna_gpu_create_archive_multi_host(pna_gpu_ctx *const *ctxs, size_t n_ctx, int algo, int level, size_t n, const char *const *names,
                                                 const void *const *src, const size_t *src_len, pna_sink_fn sink, void *user) {
    if (!ctxs || !n_ctx || !sink || (n && (!names || !src || !src_len))) return PNA_E_INVAL;
    for (size_t r = 0; r < n_ctx; r++) if (!ctxs[r]) return PNA_E_INVAL;
    if (algo == PNA_ALGO_STORE) return fail(ctxs[0], PNA_E_UNSUPPORTED, "algorithm not implemented on the device path");   // (stored entries: the one-context entry points)
    if (n_ctx == 1) return pna_gpu_create_archive_host(ctxs[0], algo, level, n, names, src, src_len, sink, user);
    // contiguous ranges balanced by input bytes (shard.partition_entries)
    uint64_t total = 0; for (size_t i = 0; i < n; i++) total += src_len[i];
    std::vector<size_t> lo(n_ctx + 1, n);
    {   // range r ends where the running byte count passes r + 1 shares of the total (a range may be empty when there are few entries)
        size_t i = 0; uint64_t acc = 0;
        for (size_t r = 0; r < n_ctx; r++) {
            lo[r] = i;
            const uint64_t target = (uint64_t)((__uint128_t)total * (r + 1) / n_ctx);
            while (i < n && (r + 1 == n_ctx || acc + src_len[i] <= target)) { acc += src_len[i]; i++; }
        }
        lo[n_ctx] = n;
    }
    // Every range runs the bounded pipeline on a thread of its own; range 0 hands its pieces to the caller's sink as they come, the ranges behind it keep
    // theirs in memory until every range before them has finished (the sink sees the archive in index order, on the calling thread only).  An exception
    // inside a worker (allocation) is that range's PNA_E_NOMEM, not a terminate; the first failing range's code is returned and its message copied to
    // ctxs[0] (what pna_gpu_last_error of the first context reports).  Every exit lies behind the join of the range threads.
    struct Part { std::vector<uint8_t> buf; int rc = PNA_OK; bool done = false; };
    std::vector<Part> parts(n_ctx);
    // every range picks the block size of the WHOLE call (pna_ctx.h CallTotalScope): the archive equals pna_gpu_create_archive_host's on one context
    std::vector<std::unique_ptr<CallTotalScope>> whole;
    for (size_t r = 0; r < n_ctx; r++) whole.emplace_back(new CallTotalScope(ctxs[r], total));
    std::mutex mu; std::condition_variable cv;
    auto vec_sink = [](void *u, const void *b, size_t k) -> int { auto *v = (std::vector<uint8_t> *)u; try { v->insert(v->end(), (const uint8_t *)b, (const uint8_t *)b + k); } catch (...) { return 1; } return 0; };
    std::vector<std::thread> th;
    for (size_t r = 1; r < n_ctx; r++)
        th.emplace_back([&, r]() {
            int rc;
            try {
                const uint32_t pf = r + 1 == n_ctx ? PNA_PART_TAIL : 0u;
                rc = pna_gpu_create_archive_part_host(ctxs[r], algo, level, lo[r + 1] - lo[r], names + lo[r], src + lo[r], src_len + lo[r], pf, vec_sink, &parts[r].buf);
            } catch (...) { rc = PNA_E_NOMEM; }
            std::lock_guard<std::mutex> lk(mu);
            parts[r].rc = rc; parts[r].done = true; cv.notify_all();
        });
    int rc;
    try { rc = pna_gpu_create_archive_part_host(ctxs[0], algo, level, lo[1] - lo[0], names + lo[0], src + lo[0], src_len + lo[0], PNA_PART_HEAD, sink, user); }
    catch (...) { rc = fail(ctxs[0], PNA_E_NOMEM, "out of memory"); }
    for (size_t r = 1; r < n_ctx; r++) {
        { std::unique_lock<std::mutex> lk(mu); cv.wait(lk, [&] { return parts[r].done; }); }
        if (rc == PNA_OK && parts[r].rc != PNA_OK) { rc = parts[r].rc; const std::string msg = std::string("range ") + std::to_string(r) + ": " + pna_gpu_last_error(ctxs[r]); (void)fail(ctxs[0], rc, msg.c_str()); }
        if (rc == PNA_OK) rc = sink_put(ctxs[0], sink, user, parts[r].buf.data(), parts[r].buf.size());
        std::vector<uint8_t>().swap(parts[r].buf);                // handed on (or abandoned): the memory goes back at once
    }
    for (auto &t : th) t.join();
    return rc;
}

namespace {
// ---- pna_gpu_compress_batch in stages.  Inputs are staged into page-locked memory by several threads and copied H2D, outputs copied D2H and scattered by
// several threads (per-entry copies from pageable memory ran at ~1 GiB/s).  A large batch goes through in PIECES of >= 256 MiB (a round of the CUs:
// the kernels' fixed latencies stay amortised): piece k + 1 is staged and copied while piece k is on the device, piece k - 1's results
// travel back meanwhile -- 512 x 1 MiB: 27.5 -> see profiles/ (PNA_BATCH_PIECE_MIB; 0 = one piece).
struct BatchPlan {
    std::vector<uint64_t> off, len, obase, pbase;                // staging offsets, lengths, running sum of the entries' bounds; where piece k's output starts in stage_out (256-byte aligned)
    std::vector<size_t> pe{0};                                   // piece k = entries [pe[k], pe[k + 1])
    uint64_t max_in = 0, max_out = 0; size_t K = 0;
};
struct BatchRun {
    pna_gpu_ctx *c; int algo, level; const void *const *src; const size_t *src_len; void *const *dst; size_t *dst_len;
    const BatchPlan &p; const unsigned threads; const bool lanes;                     // lanes: several pieces -- copies on cp_in / cp_out, slots guarded by events
    std::vector<uint64_t> doff, ptotal; pna_gpu_timing tsum{};   // output offsets of the entries (running, all pieces), compressed bytes per piece
    hipStream_t s_in() const { return lanes ? c->cp_in : c->stream; }
    hipStream_t s_out() const { return lanes ? c->cp_out : c->stream; }
    int stage(size_t k) {                                        // entries of piece k -> pinned slot -> their place in stage_in
        const int sl = (int)(k & 1);
        const size_t e0 = p.pe[k], e1 = p.pe[k + 1];
        const uint64_t b0 = p.off[e0], nb = p.off[e1] - b0;
        uint8_t *hb = (uint8_t *)c->hp_in[sl].p;
        parallel_copy(e1 - e0, threads, 8u << 20, [&](size_t i) { return CopyJob{hb + (p.off[e0 + i] - b0), (const uint8_t *)src[e0 + i], src_len[e0 + i]}; });
        if (nb) HIPCHK(c, hipMemcpyAsync((uint8_t *)c->stage_in.p + b0, hb, nb, hipMemcpyHostToDevice, s_in()));
        if (lanes) HIPCHK(c, hipEventRecord(c->ev_in[sl], s_in()));
        return PNA_OK;
    }
    int compress(size_t k) {                                     // the device call on piece k, its compressed entries on their way to the pinned slot
        const int sl = (int)(k & 1);
        if (lanes) HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_in[sl], 0));
        const size_t e0 = p.pe[k], nk = p.pe[k + 1] - e0;
        std::vector<uint64_t> d(nk + 1);
        uint8_t *ob = (uint8_t *)c->stage_out.p + p.pbase[k];
        const int rc = pna_gpu_compress_batch_device(c, algo, level, nk, c->stage_in.p, p.off.data() + e0, p.len.data() + e0, ob, p.obase[p.pe[k + 1]] - p.obase[e0] + 64, d.data(), nullptr);
        if (rc) return rc;
        { const pna_gpu_timing &t = c->timing; tsum.ms_lz += t.ms_lz; tsum.ms_stats += t.ms_stats; tsum.ms_lit += t.ms_lit; tsum.ms_seq += t.ms_seq; tsum.ms_pack += t.ms_pack;
          tsum.in_bytes += t.in_bytes; tsum.out_bytes += t.out_bytes; tsum.n_segments += t.n_segments; tsum.n_blocks += t.n_blocks; tsum.ms_lz_match += t.ms_lz_match; tsum.lz_match_launches += t.lz_match_launches; }
        for (size_t i = 0; i < nk; i++) { doff[e0 + i + 1] = doff[e0] + d[i + 1]; dst_len[e0 + i] = (size_t)(d[i + 1] - d[i]); }
        ptotal[k] = d[nk];
        if (ptotal[k]) HIPCHK(c, hipMemcpyAsync(c->hp_out[sl].p, ob, ptotal[k], hipMemcpyDeviceToHost, s_out()));   // (the kernels are done: compress_batch_device returns synchronised)
        if (lanes) HIPCHK(c, hipEventRecord(c->ev_out[sl], s_out()));
        return PNA_OK;
    }
    int scatter(size_t k) {                                      // piece k's compressed entries: pinned slot -> the caller's buffers (below 8 MiB: on the calling thread)
        const int sl = (int)(k & 1);
        if (lanes) HIPCHK(c, hipEventSynchronize(c->ev_out[sl])); else HIPCHK(c, hipStreamSynchronize(c->stream));
        const uint8_t *hb = (const uint8_t *)c->hp_out[sl].p;
        const size_t e0 = p.pe[k], e1 = p.pe[k + 1];
        parallel_copy(e1 - e0, threads, 8u << 20, [&](size_t i) { return CopyJob{(uint8_t *)dst[e0 + i], hb + (doff[e0 + i] - doff[e0]), dst_len[e0 + i]}; });
        return PNA_OK;
    }
    // an error exit: the copies issued so far read or write the pinned slots, which the next call on the context reuses -- wait for the streams they are on
    int drain(int rc) { (void)hipStreamSynchronize(s_in()); (void)hipStreamSynchronize(c->stream); (void)hipStreamSynchronize(s_out()); return rc; }
};
}
// ---- the piece cut
static BatchPlan cut_pieces(const pna_gpu_ctx *c, int algo, size_t n, const size_t *src_len) {
    BatchPlan p;
    p.off.resize(n + 1); p.len.resize(n); p.obase.resize(n + 1);
    uint64_t pos = 0, bound = 0;
    for (size_t i = 0; i < n; i++) {
        p.off[i] = pos; p.len[i] = src_len[i]; pos = (pos + src_len[i] + 15) & ~(uint64_t)15;
        p.obase[i] = bound; bound += pna_gpu_bound(algo, src_len[i]);
    }
    p.off[n] = pos; p.obase[n] = bound;
    const uint64_t piece_bytes = c->tun.batch_piece_mib <= 0 ? ~0ull >> 1 : (uint64_t)c->tun.batch_piece_mib << 20;
    for (size_t i = 0; i < n;) {
        size_t j = i; uint64_t acc = 0;
        while (j < n && (j == i || acc + src_len[j] <= piece_bytes)) acc += src_len[j++];
        p.pe.push_back(j); i = j;
    }
    if (p.pe.size() > 2 && p.off[n] - p.off[p.pe[p.pe.size() - 2]] < piece_bytes / 2) p.pe.erase(p.pe.end() - 2);   // a short last piece joins its neighbour
    p.K = p.pe.size() - 1;
    p.pbase.assign(p.K + 1, 0);
    for (size_t k = 0; k < p.K; k++) {
        p.max_in = std::max(p.max_in, p.off[p.pe[k + 1]] - p.off[p.pe[k]]); p.max_out = std::max(p.max_out, p.obase[p.pe[k + 1]] - p.obase[p.pe[k]]);
        p.pbase[k + 1] = (p.pbase[k] + (p.obase[p.pe[k + 1]] - p.obase[p.pe[k]]) + 64 + 255) & ~(uint64_t)255;
    }
    return p;
}
extern "C" int pna_gpu_compress_batch(pna_gpu_ctx *c, int algo, int level, size_t n, const void *const *src,
                                      const size_t *src_len, void *const *dst, const size_t *dst_cap, size_t *dst_len) {
    if (!c || (n && (!src || !src_len || !dst || !dst_cap || !dst_len))) return fail(c, PNA_E_INVAL, "null argument");
    if (!encode_algo_ok(c, algo)) return fail(c, PNA_E_UNSUPPORTED, "algorithm not implemented");
    HIPCHK(c, hipSetDevice(c->device));
    for (size_t i = 0; i < n; i++) if (dst_cap[i] < pna_gpu_bound(algo, src_len[i])) return fail(c, PNA_E_DSTSIZE, "dst_cap below pna_gpu_bound");
    const CallTotalScope call_total(c, src_len, n);              // (the pieces below pick the block size of the whole call: the bytes equal pna_gpu_compress_batch_device's)
    const BatchPlan p = cut_pieces(c, algo, n, src_len);
    const size_t K = p.K, slots = K > 1 ? 2 : 1;
    int rc = Reserve{c}.add(c->stage_in, p.off[n] + 8192).add(c->stage_out, p.pbase[K] + 64).add(c->hp_in, slots, p.max_in + 64).add(c->hp_out, slots, p.max_out + 64).done();
    if (rc) return rc;
    if (K > 1 && (rc = ensure_copy_lanes(c))) return rc;
    BatchRun r{c, algo, level, src, src_len, dst, dst_len, p, staging_threads(c), K > 1, std::vector<uint64_t>(n + 1), std::vector<uint64_t>(K)};
    if (K && (rc = r.stage(0))) return r.drain(rc);
    for (size_t k = 0; k < K; k++) {
        if (k + 1 < K && (rc = r.stage(k + 1))) return r.drain(rc);          // (its slot's previous copy, piece k - 1, was waited for by that piece's kernels)
        if ((rc = r.compress(k))) return r.drain(rc);
        if (k >= 1 && (rc = r.scatter(k - 1))) return r.drain(rc);
    }
    if (K && (rc = r.scatter(K - 1))) return r.drain(rc);
    c->timing = r.tsum;
    return PNA_OK;
}
