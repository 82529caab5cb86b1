// pna_decode.cpp -- the decoders' host side: DecodeBatch (pna_ctx.h) to its codec's decoder (decode_batch), the zstd and zlib decoders as stages, open-size measurement, the exports.
#include "pna_ctx.h"
#include "xz_core.h"

// The parallel executor (k_zexec_par.hip) runs a frame / stream in WINDOWS of whole blocks, at most zexec_win_mib (1 024) MiB of output each (its words count 31 bits from the
// window's start): the cuts, from the blocks' output offsets (k_zoff / the chunk decoder's count pass have set them).  One window for everything up to 1 GiB.
static int zx_windows(pna_gpu_ctx *c, const ZxFrame &h, hipStream_t st, std::vector<uint32_t> &win_blk, std::vector<uint64_t> &win_off, uint64_t *max_win) {
    win_blk.assign(1, 0u); win_off.assign(1, 0ull);
    uint64_t mx = h.dst_len;
    const uint64_t WMAX = (uint64_t)c->tun.zexec_win_mib << 20;
    if (h.dst_len > WMAX) {
        std::vector<ZBlock> hb(h.nblk);
        HIPCHK(c, hipMemcpyAsync(hb.data(), (const ZBlock *)c->z_blocks.p + h.blk_base, (size_t)h.nblk * sizeof(ZBlock), hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipStreamSynchronize(st));
        mx = 0;
        uint64_t start = 0;
        for (uint32_t k = 0; k < h.nblk; k++) {
            const uint64_t rel = hb[k].out_off - h.dst_off, end = rel + hb[k].out_len;
            if (end - start > WMAX && rel > start) { mx = std::max(mx, rel - start); win_blk.push_back(k); win_off.push_back(rel); start = rel; }
        }
        mx = std::max(mx, h.dst_len - start);
    }
    win_blk.push_back(h.nblk); win_off.push_back(h.dst_len);
    *max_win = mx;
    return PNA_OK;
}

// the zstd and zlib decoders' workspace, typed
static ZFrame *zframes(pna_gpu_ctx *c) { return (ZFrame *)c->z_frames.p; }
static ZFrameX *zfx(pna_gpu_ctx *c) { return (ZFrameX *)c->z_fx.p; }
static ZBlock *zblocks(pna_gpu_ctx *c) { return (ZBlock *)c->z_blocks.p; }
static uint8_t *zlit(pna_gpu_ctx *c) { return (uint8_t *)c->z_lit.p; }
static uint64_t *zseqs(pna_gpu_ctx *c) { return (uint64_t *)c->z_seqs.p; }
// One frame / stream through the parallel executor: its windows, the workspace, the descriptor, the launch.  *zst: the executor's status (0: executed), the caller reacts to it
static int exec_par_frame(pna_gpu_ctx *c, ZxFrame h, const void *d_src, void *d_dst, hipStream_t st, uint32_t *zst, const char *failed) {
    std::vector<uint32_t> wblk; std::vector<uint64_t> woff; uint64_t wmax = 0;
    { const int rw = zx_windows(c, h, st, wblk, woff, &wmax); if (rw) return rw; }
    if (c->z_words.ensure(wmax * 4 + 4096) || c->z_rep.ensure((size_t)h.nblk * 24 + 64) || c->z_zxf.ensure(64)) return fail(c, PNA_E_NOMEM, "decoder workspace");
    HIPCHK(c, hipMemcpyAsync(c->z_zxf.p, &h, sizeof h, hipMemcpyHostToDevice, st));
    if (launch_zexec_par((ZxFrame *)c->z_zxf.p, h, zblocks(c), (const uint8_t *)d_src, zlit(c), zseqs(c), (uint32_t *)c->z_rep.p, (uint32_t *)c->z_words.p, (uint8_t *)d_dst, zst, &c->zexec_par_rounds, st,
                         (uint32_t)wblk.size() - 1, wblk.data(), woff.data()) != 0)
        return fail(c, PNA_E_HIP, failed);
    return PNA_OK;
}
// v (0 .. 3) into one 32-bit word of device memory, on the stream: the copy is asynchronous, its source is this table, which outlives every copy
static const uint32_t WORD_VALUE[4] = {0u, 1u, 2u, 3u};
static hipError_t poke32(void *d_word, uint32_t v, hipStream_t st) { return hipMemcpyAsync(d_word, &WORD_VALUE[v], 4, hipMemcpyHostToDevice, st); }
// The first bad stream of a call as the call's failure: "<who>: <what> (produced x of y bytes)" -- who: "entry i" or "entry i frame f", size3: what status 3 is called
static int fail_status(pna_gpu_ctx *c, const std::string &who, const ZFrame &fr, const char *size3) {
    char msg[160];
    snprintf(msg, sizeof msg, "%s: %s (produced %u of %llu bytes)", who.c_str(), fr.status == 2 ? "unsupported stream" : (fr.status == 3 ? size3 : "corrupt stream"), fr.out_len, (unsigned long long)fr.dst_len);
    return fail(c, fr.status == 2 ? PNA_E_UNSUPPORTED : PNA_E_INVAL, msg);
}

// ---------------------------------------------------------------------------------------------------------
// Read side, Compression::Deflate: one zlib stream per entry (flate2::read::ZlibDecoder, lib/src/entry/read.rs:178-179).
// k_inflate turns each stream into literals + (run, length, distance) records, k_zoff / k_zexec execute them, k_iadler_* check
// the Adler-32 trailer.
static constexpr uint32_t SPEC_CHUNK = 16384;
// One walk of k_inflate's chunk mode over the chunks ch[idx[0 ..]] (idx empty: all of them) of stream f (its ZFrame / ZFrameX on the device): count pass
// (emit = 0: only the chunk descriptors are written) or emit pass.
static int run_chunks(pna_gpu_ctx *c, uint32_t f, std::vector<ISChunkH> &ch, const std::vector<uint32_t> &idx, uint32_t emit, ISChunkH *d_chunks, const void *d_src,
                      ZBlock *blocks, uint8_t *lit, uint64_t *seqs, hipStream_t st) {
    const uint32_t cnt = idx.empty() ? (uint32_t)ch.size() : (uint32_t)idx.size();
    std::vector<ISChunkH> sub;
    if (!idx.empty()) { sub.resize(cnt); for (uint32_t i = 0; i < cnt; i++) sub[i] = ch[idx[i]]; }
    ISChunkH *hp = idx.empty() ? ch.data() : sub.data();
    HIPCHK(c, hipMemcpyAsync(d_chunks, hp, (size_t)cnt * sizeof(ISChunkH), hipMemcpyHostToDevice, st));
    launch_inflate_chunks((ZFrame *)c->z_frames.p, (ZFrameX *)c->z_fx.p, f, d_chunks, cnt, emit, (const uint8_t *)d_src, blocks, lit, seqs, st);
    HIPCHK(c, hipMemcpyAsync(hp, d_chunks, (size_t)cnt * sizeof(ISChunkH), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    if (!idx.empty()) for (uint32_t i = 0; i < cnt; i++) ch[idx[i]] = sub[i];
    return PNA_OK;
}
// The count pass over the chunks `ch` of stream f, false block starts repaired; *ok = false: a chunk's walk failed, the chain is broken or there were too many
// false starts (`why` says which).
// A walk that runs past its chunk's end says the NEXT chunk's start was not a block start (a well-formed header by chance: one in a few 10^9 bit positions --
// seen in a 445 MB stream, five of them in a 2 GB one): that chunk is dropped, its predecessor runs on to the start behind it and is counted again -- only it:
// the other chunks' counts stand (second half of round 4; before, every repair was a walk over the whole stream, one false start at a time).  A dropped chunk's
// own walk says nothing about the chunk behind it, which is judged in the next round by its new predecessor.
static int count_chunks(pna_gpu_ctx *c, uint32_t f, std::vector<ISChunkH> &ch, ISChunkH *d_chunks, const void *d_src, ZBlock *blocks, uint8_t *lit, uint64_t *seqs,
                        hipStream_t st, const std::function<void(const char *, uint64_t, uint64_t)> &why, bool *ok) {
    *ok = false;
    uint32_t m = (uint32_t)ch.size();
    std::vector<uint32_t> todo;                                      // (empty: everything)
    for (int round = 0;; round++) {
        const int rc = run_chunks(c, f, ch, todo, 0, d_chunks, d_src, blocks, lit, seqs, st); if (rc) return rc;
        std::vector<ISChunkH> keep; keep.reserve(m);
        todo.clear();
        bool prev_dropped = false;
        for (uint32_t k = 0; k < m; k++) {
            if (k > 0 && !prev_dropped && ch[k - 1].status == 4u /* IF_CHAIN */) {           // the predecessor (kept, its walk valid) ran past this chunk's start
                if (todo.empty() || todo.back() != (uint32_t)keep.size() - 1) todo.push_back((uint32_t)keep.size() - 1);
                prev_dropped = true;
                continue;
            }
            prev_dropped = false;
            keep.push_back(ch[k]);
        }
        if (todo.empty()) break;
        if (round >= 16) { why("too many false block starts", m, round); return PNA_OK; }
        ch.swap(keep); m = (uint32_t)ch.size();
        for (uint32_t i : todo) { ISChunkH &h = ch[i]; const uint64_t sb = h.start_bit; h = ISChunkH{}; h.start_bit = sb; h.end_bit = i + 1 < m ? ch[i + 1].start_bit : ~0ull; }
    }
    for (uint32_t k = 0; k < m; k++) {
        const ISChunkH &h = ch[k];
        if (h.status) { why("a chunk's walk failed: chunk, status", k, h.status); return PNA_OK; }
        if (k + 1 < m && h.end_found != ch[k + 1].start_bit) { why("the chain is broken behind chunk: end found, next start", h.end_found, ch[k + 1].start_bit); return PNA_OK; }   // a false start, or a stream this scheme does not fit
    }
    *ok = true;
    return PNA_OK;
}
// Why a stream was not decoded in chunks; corrupt: a chunk's walk found damage (and no false start explains it).  A stream of 4 GiB and more has no other way:
// it is refused with this (a stream of fixed-Huffman blocks only has no block start the trial can find: PNA_E_UNSUPPORTED).
struct SpecWhy { std::string text = "too few block starts found"; bool corrupt = false; };
static int big_unsplit(pna_gpu_ctx *c, uint64_t src_len, const SpecWhy &w) {
    char msg[384];
    if (w.corrupt) { snprintf(msg, sizeof msg, "corrupt zlib stream of %llu compressed bytes (decoding it in chunks: %s)", (unsigned long long)src_len, w.text.c_str()); return fail(c, PNA_E_INVAL, msg); }
    snprintf(msg, sizeof msg, "zlib stream of %llu compressed bytes not decoded: a stream of 4 GiB and more is decoded in chunks between dynamic or stored block starts, and this one "
             "does not split (%s) -- a stream of fixed-Huffman blocks only has no start to split at", (unsigned long long)src_len, w.text.c_str());
    return fail(c, PNA_E_UNSUPPORTED, msg);
}
// block starts of a stream by trial (k_ispec): one chunk per start found, each running up to the next (nch chunks of SPEC_CHUNK bytes searched)
static int find_chunks(pna_gpu_ctx *c, const void *d_src, uint64_t src_off, uint64_t src_len, uint32_t nch, uint64_t *d_start, std::vector<ISChunkH> &ch, hipStream_t st) {
    std::vector<uint64_t> start(nch);
    launch_ispec((const uint8_t *)d_src, src_off, src_len, SPEC_CHUNK, nch, d_start, st);
    HIPCHK(c, hipMemcpyAsync(start.data(), d_start, (size_t)nch * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    ch.clear();
    for (uint32_t k = 0; k < nch; k++)
        if (start[k] != ~0ull) { ISChunkH h{}; h.start_bit = start[k]; h.end_bit = ~0ull; if (!ch.empty()) ch.back().end_bit = start[k]; ch.push_back(h); }
    return PNA_OK;
}

// A LARGE stream the lane-per-piece decoder cannot take (a foreign encoder's: no sync flush behind every 128 KiB -- what the reference itself writes for a large
// deflate entry): block starts found by trial (k_ispec), one wave per chunk between two of them (k_inflate's chunk mode: COUNT, prefix sums here, EMIT), one ZBlock per
// chunk.  *ok = false: something did not fit (no chunk starts found, a chunk's walk did not end where the next begins, sizes that do not add up) -- the serial walk
// takes the stream, nothing is lost but time; a stream of 4 GiB and more is refused then (big_unsplit).  The records are executed by k_zexec_par afterwards (the caller).
static int inflate_spec_stream(pna_gpu_ctx *c, uint32_t f, const ZFrame &fr, const ZFrameX &x, const void *d_src, hipStream_t st, uint32_t *nblk_out, bool *ok,
                               bool open, uint64_t *out_len, SpecWhy *reason) {
    *ok = false;
    const uint32_t nch = (uint32_t)((fr.src_len + SPEC_CHUNK - 1) / SPEC_CHUNK);
    if (nch < 4 || nch > x.blk_cap) return PNA_OK;
    if (c->z_spec.ensure((size_t)nch * (8 + sizeof(ISChunkH)) + 64)) return fail(c, PNA_E_NOMEM, "decoder workspace");
    uint64_t *d_start = (uint64_t *)c->z_spec.p;
    ISChunkH *d_chunks = (ISChunkH *)((uint8_t *)c->z_spec.p + (size_t)nch * 8);
    std::vector<ISChunkH> ch;
    int rc = find_chunks(c, d_src, fr.src_off, fr.src_len, nch, d_start, ch, st); if (rc) return rc;
    uint32_t m = (uint32_t)ch.size();
    auto why = [&](const char *what, uint64_t a, uint64_t b) {
        char t[192]; snprintf(t, sizeof t, "%s (%llu, %llu)", what, (unsigned long long)a, (unsigned long long)b); reason->text = t;
        if (c->tun.trace) fprintf(stderr, "[pna inflate] stream %u of %llu B not decoded in chunks: %s\n", f, (unsigned long long)fr.src_len, t);
    };
    if (m < 4) { why("too few block starts found", m, nch); return PNA_OK; }                                      // (fixed-code blocks, or blocks of more than a chunk each: not worth the two passes)
    bool counted = false;
    rc = count_chunks(c, f, ch, d_chunks, d_src, (ZBlock *)c->z_blocks.p, (uint8_t *)c->z_lit.p, (uint64_t *)c->z_seqs.p, st, why, &counted); if (rc) return rc;
    if (!counted) { for (const ISChunkH &h : ch) reason->corrupt |= h.status == 1u; return PNA_OK; }
    m = (uint32_t)ch.size();
    uint64_t lit = 0, out = 0, rec = 0;
    for (uint32_t k = 0; k < m; k++) { const ISChunkH &h = ch[k]; lit += h.nlit; out += (uint64_t)h.nlit + h.mtot; rec += h.nrec; }
    if (open ? out > fr.dst_len : out != fr.dst_len) { why("sizes do not add up: output, expected", out, fr.dst_len); return PNA_OK; }   // (open: dst_len is the room)
    *out_len = out;
    if (rec > x.seq_cap) { why("more records than room: records, room", rec, x.seq_cap); return PNA_OK; }
    if ((ch[m - 1].end_found + 7) / 8 != fr.src_len) { why("the last chunk does not end with the stream: end bit, stream bytes", ch[m - 1].end_found, fr.src_len); return PNA_OK; }
    lit = out = rec = 0;
    for (uint32_t k = 0; k < m; k++) { ISChunkH &h = ch[k]; h.lit_base = lit; h.out_base = out; h.rec_base = rec; lit += h.nlit; out += (uint64_t)h.nlit + h.mtot; rec += h.nrec; }
    rc = run_chunks(c, f, ch, std::vector<uint32_t>(), 1, d_chunks, d_src, (ZBlock *)c->z_blocks.p, (uint8_t *)c->z_lit.p, (uint64_t *)c->z_seqs.p, st); if (rc) return rc;
    for (uint32_t k = 0; k < m; k++) if (ch[k].status) { why("a chunk's second walk failed: chunk, status", k, ch[k].status); reason->corrupt = ch[k].status == 1u; return PNA_OK; }
    *nblk_out = m; *ok = true;
    return PNA_OK;
}

struct InflateRun {
    pna_gpu_ctx *c; const DecodeBatch &b; const uint8_t *src; uint8_t *dst;
    std::vector<ZFrame> frs; std::vector<ZFrameX> fxs; struct VPieceH { uint32_t frame, j; }; std::vector<VPieceH> vp; std::vector<uint32_t> cbase, modes; bool lanes = false; uint32_t scan_g = 1; uint64_t nseq_cap = 0, out_span = 0, pieces = 0, nblk = 0;
    std::vector<uint32_t> cand; std::vector<uint64_t> cand_base;   // large streams that may be a foreign encoder's, and where their chunks' blocks start
    std::vector<std::pair<uint32_t, ZFrameX>> spec; std::vector<uint64_t> spec_len;   // ... those of them the chunk decoder took, and their decoded sizes
    // Streams of known size go lane-per-piece (k_vinflate): a stream of at most BLK_SIZE decoded bytes is one piece, a larger one is taken
    // to consist of ceil(raw_len / BLK_SIZE) sync-flush delimited pieces of BLK_SIZE bytes each (what this library's encoder writes) --
    // k_imark / k_vinflate / k_vfin check that and leave every stream that does not fit to the wave-per-stream kernel.  Streams of
    // unknown size (`open`) take the wave-per-stream kernel directly.
    // pieces per stream: from the size when it is known; for streams of unknown size (solid streams, entries without fSIZ) from a count of
    // the sync-flush markers (one pass + one small read-back): markers + 1 pieces, all but the last holding BLK_SIZE bytes
    int count_pieces_and_plan() {
        const size_t n = b.n;
        if (n > 0x3FFFFFFFull) return fail(c, PNA_E_INVAL, "batch too large for one decode call");
        std::vector<uint64_t> npc(n);                                  // pieces per stream
        lanes = !c->tun.inflate_serial;
        // workgroups per stream for the marker scans: one per 256 KiB of the batch's longest stream (n x G bounded)
        uint64_t max_src = 0, tot_pieces = 0;
        for (size_t i = 0; i < n; i++) max_src = std::max<uint64_t>(max_src, b.src_len[i]);
        scan_g = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(std::min<uint64_t>(max_src >> 18, 1024), (1ull << 24) / std::max<size_t>(n, 1)));
        if (lanes && b.open) {
            std::vector<uint32_t> cnt(n);
            if (c->z_pb.ensure(n * 4 + 8) || c->z_vp.ensure(n * 16 + 16)) return fail(c, PNA_E_NOMEM, "decoder workspace");
            HIPCHK(c, hipMemcpyAsync(c->z_vp.p, b.src_off, n * 8, hipMemcpyHostToDevice, b.st));
            HIPCHK(c, hipMemcpyAsync((uint8_t *)c->z_vp.p + n * 8, b.src_len, n * 8, hipMemcpyHostToDevice, b.st));
            launch_icount(src, (const uint64_t *)c->z_vp.p, (const uint64_t *)((uint8_t *)c->z_vp.p + n * 8), (uint32_t)n, (uint32_t *)c->z_pb.p, scan_g, b.st);
            HIPCHK(c, hipMemcpyAsync(cnt.data(), c->z_pb.p, n * 4, hipMemcpyDeviceToHost, b.st));
            HIPCHK(c, hipStreamSynchronize(b.st));
            for (size_t i = 0; i < n; i++) { npc[i] = (uint64_t)cnt[i] + 1; if ((npc[i] - 1) * BLK_SIZE > b.raw_len[i]) npc[i] = 1; }   // more pieces than the room allows: not this library's layout
        } else
            for (size_t i = 0; i < n; i++) npc[i] = std::max<uint64_t>(1, (b.raw_len[i] + BLK_SIZE - 1) / BLK_SIZE);
        for (size_t i = 0; i < n; i++) tot_pieces += npc[i];
        // a handful of pieces is served better by the wave-per-stream walk (a lane needs ~110 ms for a 128 KiB piece, however few there are)
        if (tot_pieces < 1024) lanes = false;
        // host arithmetic: every stream's ZFrame and its share of the blocks, records and Adler pieces; the candidates for the chunk decoder
        frs.resize(n); fxs.resize(n); cbase.resize(n + 1);
        // large streams that may turn out to be a foreign encoder's (inflate_spec_stream): candidates by size; their chunks' blocks live behind the batch's own
        const uint64_t spec_min = (uint64_t)c->tun.zexec_par_min_mib << 20;
        for (size_t i = 0; i < n; i++) {
            const uint64_t src_len = b.src_len[i], raw_len = b.raw_len[i];
            // (open: raw_len is the room, the size comes out of the count; the stream must be worth it by its compressed size then)
            const bool is_cand = spec_min && (b.open ? src_len >= spec_min / 4 : raw_len >= spec_min) && src_len >= 8ull * SPEC_CHUNK;   // (output of any size: the executor works in windows)
            // streams of 4 GiB and more: decoded by pieces (this library's layout: a sync flush behind every 128 KiB) or in chunks; the wave-per-stream walk counts in 32 bits
            if ((raw_len > 0xFFFFFFFFull || src_len > 0xFFFFFFFFull) && !lanes && !is_cand) return fail(c, PNA_E_UNSUPPORTED, "zlib streams of 4 GiB and more are decoded by sync-flush delimited pieces or in chunks only");
            frs[i] = ZFrame{b.src_off[i], b.dst_off[i], src_len, raw_len, 0, b.open ? ZF_OPEN : 0u};   // open: raw_len is a capacity
            ZFrameX &x = fxs[i];
            const uint64_t P = lanes ? npc[i] : 1;
            const uint64_t pcap = std::min<uint64_t>(raw_len, lanes ? BLK_SIZE : raw_len) / 3 + (raw_len >> 16) / P + 16;   // matches are >= 3 bytes; + literal-run splits (serial walk)
            if (nblk + P > 0x7FFFFFFFull) return fail(c, PNA_E_INVAL, "batch too large for one decode call");
            x.blk_base = (uint32_t)nblk; x.blk_cap = (uint32_t)P; x.slot_base = 0; x.slot_cap = 0; x.nblk = 0;
            x.seq_base = nseq_cap; x.seq_cap = (uint32_t)std::min<uint64_t>(P * pcap, 0x7FFFFFFFu); x.pcap = (uint32_t)std::min<uint64_t>(pcap, 0x7FFFFFFFu); x.pad = 0;
            nseq_cap += P * pcap;
            if (lanes) for (uint64_t j = 0; j < P; j++) vp.push_back(VPieceH{(uint32_t)i, (uint32_t)j});
            nblk += P;
            out_span = std::max<uint64_t>(out_span, b.dst_off[i] + raw_len);
            cbase[i] = (uint32_t)pieces;
            pieces += (raw_len + 65535) >> 16;
            if (pieces > 0xFFFFFFF0ull) return fail(c, PNA_E_INVAL, "batch too large for one decode call");
            if (is_cand) cand.push_back((uint32_t)i);
        }
        cbase[n] = (uint32_t)pieces;
        for (uint32_t i : cand) { cand_base.push_back(nblk); nblk += (b.src_len[i] + SPEC_CHUNK - 1) / SPEC_CHUNK; if (nblk > 0x7FFFFFFFull) return fail(c, PNA_E_INVAL, "batch too large for one decode call"); }
        return PNA_OK;
    }
    int workspace_upload_and_lanes() {
        const size_t n = b.n;
        if (c->z_frames.ensure(n * sizeof(ZFrame)) || c->z_fx.ensure(n * sizeof(ZFrameX)) || c->z_blocks.ensure(nblk * sizeof(ZBlock)) ||
            c->z_lit.ensure(out_span + 64) || c->z_seqs.ensure(nseq_cap * 8 + 64) || c->z_cbase.ensure((n + 1) * 4) || c->z_apart.ensure(pieces * 8 + 8) ||
            c->z_mode.ensure(n * 4 + 8 + (lanes ? (size_t)n * scan_g * 4 : 0)) ||
            (lanes && (c->z_vp.ensure(vp.size() * 8 + 8) || c->z_pb.ensure((nblk + n) * 8 + 8))))
            return fail(c, PNA_E_NOMEM, "decoder workspace");
        modes.assign(n, (uint32_t)VM_SERIAL);                          // the wave-per-stream walk's; the lane-per-piece decoder decides for itself when it runs
        if (!lanes) HIPCHK(c, hipMemcpyAsync(c->z_mode.p, modes.data(), n * 4, hipMemcpyHostToDevice, b.st));
        HIPCHK(c, hipMemcpyAsync(c->z_frames.p, frs.data(), n * sizeof(ZFrame), hipMemcpyHostToDevice, b.st));
        HIPCHK(c, hipMemcpyAsync(c->z_fx.p, fxs.data(), n * sizeof(ZFrameX), hipMemcpyHostToDevice, b.st));
        HIPCHK(c, hipMemcpyAsync(c->z_cbase.p, cbase.data(), (n + 1) * 4, hipMemcpyHostToDevice, b.st));
        if (lanes) HIPCHK(c, hipMemcpyAsync(c->z_vp.p, vp.data(), vp.size() * 8, hipMemcpyHostToDevice, b.st));
        HIPCHK(c, hipEventRecord(c->ev[0], b.st));
        // the lane-per-piece decoder over every piece of the batch (in z_mode it says which streams it leaves to the wave-per-stream walk)
        if (lanes) launch_vinflate(zframes(c), zfx(c), (uint32_t)b.n, c->z_vp.p, (uint32_t)vp.size(), (uint64_t *)c->z_pb.p, (uint32_t *)c->z_mode.p, (uint32_t *)c->z_mode.p + b.n + 2, scan_g,
                                   src, zblocks(c), zlit(c), zseqs(c), b.st);
        return PNA_OK;
    }
    // ---- large foreign streams: chunks between block starts found by trial, walked side by side; what does not fit stays with the serial walk below
    int decode_spec_candidates() {
        if (cand.empty()) return PNA_OK;
        if (lanes) { HIPCHK(c, hipMemcpyAsync(modes.data(), c->z_mode.p, b.n * 4, hipMemcpyDeviceToHost, b.st)); HIPCHK(c, hipStreamSynchronize(b.st)); }
        for (size_t k = 0; k < cand.size(); k++) {
            const uint32_t i = cand[k];
            if (modes[i] != VM_SERIAL) continue;                              // this library's layout: the lane-per-piece decoder has it
            ZFrameX xs = fxs[i];
            xs.blk_base = (uint32_t)cand_base[k]; xs.blk_cap = (uint32_t)((b.src_len[i] + SPEC_CHUNK - 1) / SPEC_CHUNK); xs.nblk = 0; xs.pad = 0;
            HIPCHK(c, hipMemcpyAsync(zfx(c) + i, &xs, sizeof xs, hipMemcpyHostToDevice, b.st));
            bool ok = false; uint32_t m = 0; uint64_t olen = 0; SpecWhy reason;
            const int rcs = inflate_spec_stream(c, i, frs[i], xs, b.d_src, b.st, &m, &ok, b.open, &olen, &reason); if (rcs) return rcs;
            if (!ok && (b.src_len[i] > 0xFFFFFFFFull || b.raw_len[i] > 0xFFFFFFFFull)) return big_unsplit(c, b.src_len[i], reason);   // (the serial walk counts in 32 bits)
            if (ok) {
                xs.nblk = m; xs.pad = 1; HIPCHK(c, poke32((uint32_t *)c->z_mode.p + i, VM_CHUNKS, b.st));   // (not VM_SERIAL: the serial walk leaves the stream alone)
                if (b.open) {                                           // the size found: what the serial walk reports through ZFrame::dst_len
                    frs[i].dst_len = olen;
                    HIPCHK(c, hipMemcpyAsync(&zframes(c)[i].dst_len, &frs[i].dst_len, 8, hipMemcpyHostToDevice, b.st));
                }
            }
            else xs = fxs[i];
            HIPCHK(c, hipMemcpyAsync(zfx(c) + i, &xs, sizeof xs, hipMemcpyHostToDevice, b.st));
            HIPCHK(c, hipStreamSynchronize(b.st));                      // (xs is read by the copy until then)
            if (ok) { spec.emplace_back(i, xs); spec_len.push_back(olen); }
        }
        return PNA_OK;
    }
    // the wave-per-stream walk over what is left to it, then the records' execution: execution groups side by side (k_vfin) behind the lanes, a wave per stream otherwise
    int walk_and_execute() {
        launch_inflate(zframes(c), zfx(c), (uint32_t)b.n, src, zblocks(c), zlit(c), zseqs(c), (const uint32_t *)c->z_mode.p, b.st);
        HIPCHK(c, hipEventRecord(c->ev[2], b.st));
        if (lanes) launch_zexec_groups(zframes(c), zfx(c), (uint32_t)b.n, zblocks(c), c->z_vp.p, (uint32_t)vp.size(), src, zlit(c), zseqs(c), dst, b.st);
        else launch_zexec(zframes(c), zfx(c), (uint32_t)b.n, zblocks(c), src, zlit(c), zseqs(c), dst, b.st);
        // the spec streams' chunks' records: pointer jumping over the stream's output positions (k_zexec_par.hip); a stream the executor gives up on is corrupt
        for (size_t si = 0; si < spec.size(); si++) {
            const uint32_t i = spec[si].first; const ZFrameX &x = spec[si].second;
            uint32_t zst = 0;
            const int rc = exec_par_frame(c, ZxFrame{frs[i].dst_off, spec_len[si], x.blk_base, x.nblk, 0, 0}, b.d_src, b.d_dst, b.st, &zst, "parallel stream execution failed"); if (rc) return rc;
            if (zst) HIPCHK(c, poke32(&zframes(c)[i].status, 1u, b.st));
        }
        c->inflate_spec_streams = (uint32_t)spec.size();
        HIPCHK(c, hipEventRecord(c->ev[3], b.st));
        return PNA_OK;
    }
    // the Adler-32 trailers against the output, the streams' ZFrames back, the call's times
    int check_and_read_back() {
        launch_iadler(zframes(c), zfx(c), zblocks(c), (uint32_t)b.n, (const uint32_t *)c->z_cbase.p, (uint32_t)pieces, dst, c->z_apart.p, b.st);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipEventRecord(c->ev[1], b.st));
        HIPCHK(c, hipMemcpyAsync(frs.data(), c->z_frames.p, b.n * sizeof(ZFrame), hipMemcpyDeviceToHost, b.st));
        if (lanes) HIPCHK(c, hipMemcpyAsync(modes.data(), c->z_mode.p, b.n * 4, hipMemcpyDeviceToHost, b.st));   // (which streams the lane-per-piece decoder kept: pna_gpu_last_decode_forms says how many)
        HIPCHK(c, hipStreamSynchronize(b.st));                          // (frs is written by the copy above until then)
        float ms = 0, ms_h = 0, ms_x = 0;
        (void)hipEventElapsedTime(&ms, c->ev[0], c->ev[1]); (void)hipEventElapsedTime(&ms_h, c->ev[0], c->ev[2]); (void)hipEventElapsedTime(&ms_x, c->ev[2], c->ev[3]);
        c->timing = pna_gpu_timing{}; c->timing.ms_lz = ms; c->timing.ms_stats = ms_h; c->timing.ms_lit = ms_x;   // total, Huffman walk, execution
        c->timing.lz_match_launches = spec.size();                      // (decode calls: the large foreign streams that went through the chunk decoder)
        c->forms = pna_gpu_decode_forms{}; c->forms.inflate_chunk_streams = spec.size();
        if (lanes) { c->forms.inflate_lane_pieces = vp.size(); for (uint32_t m : modes) c->forms.inflate_lane_streams += m == VM_PIECES; }
        return PNA_OK;
    }
    // what the caller gets: verdict mode -- every stream's own status, no call-level failure --, or the first bad stream as the call's failure; the sizes found
    int settle() {
        if (b.ent_status) for (size_t i = 0; i < b.n; i++) b.ent_status[i] = frs[i].status;
        for (size_t i = 0; i < b.n && !b.ent_status; i++) if (frs[i].status) return fail_status(c, "entry " + std::to_string(i), frs[i], "size mismatch");
        if (b.open && b.raw_out) for (size_t i = 0; i < b.n; i++) b.raw_out[i] = frs[i].dst_len;
        return PNA_OK;
    }
};
static int inflate_batch_device(pna_gpu_ctx *c, const DecodeBatch &b) {
    InflateRun r{c, b, (const uint8_t *)b.d_src, (uint8_t *)b.d_dst};
    int rc = r.count_pieces_and_plan(); if (rc) return rc;
    rc = r.workspace_upload_and_lanes(); if (rc) return rc;
    rc = r.decode_spec_candidates(); if (rc) return rc;
    rc = r.walk_and_execute(); if (rc) return rc;
    rc = r.check_and_read_back(); if (rc) return rc;
    return r.settle();
}

// ---------------------------------------------------------------------------------------------------------
// The decoded size of one stream whose size is recorded nowhere, measured before it is decoded: no output buffer, scratch by the compressed length.
// zlib: k_inflate's chunk mode in its count pass (emit = 0: nothing but the chunk descriptors is written) between block starts found by trial (k_ispec --
// this library's sync-flush pieces, a foreign encoder's dynamic and stored blocks alike), one wave per chunk, false starts repaired; one wave over the whole
// stream when there are fewer than four starts (small streams, fixed-code blocks) or the chain does not hold -- below 4 GiB of compressed bytes: a longer
// stream that does not split is refused (big_unsplit).  The count is exact.
static int inflate_measure(pna_gpu_ctx *c, const void *d_src, uint64_t src_off, uint64_t src_len, uint64_t *size, hipStream_t st) {
    const uint32_t nch = src_len >= 8ull * SPEC_CHUNK ? (uint32_t)((src_len + SPEC_CHUNK - 1) / SPEC_CHUNK) : 1u;
    if (c->z_spec.ensure((size_t)nch * (8 + sizeof(ISChunkH)) + 64) || c->z_frames.ensure(sizeof(ZFrame)) || c->z_fx.ensure(sizeof(ZFrameX)))
        return fail(c, PNA_E_NOMEM, "measurement workspace");
    uint64_t *d_start = (uint64_t *)c->z_spec.p;
    ISChunkH *d_chunks = (ISChunkH *)((uint8_t *)c->z_spec.p + (size_t)nch * 8);
    uint8_t *none = (uint8_t *)c->z_spec.p;                              // (the count pass writes no literals, records or blocks)
    static const ZFrame fr0{0, 0, 0, ~0ull, 0, 0};                        // dst_len: no limit
    ZFrame fr = fr0; fr.src_off = src_off; fr.src_len = src_len;
    ZFrameX x{}; x.seq_cap = 0xFFFFFFFFu;
    HIPCHK(c, hipMemcpyAsync(c->z_frames.p, &fr, sizeof fr, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(c->z_fx.p, &x, sizeof x, hipMemcpyHostToDevice, st));
    std::vector<ISChunkH> ch;
    int rc = PNA_OK;
    if (nch >= 8) { rc = find_chunks(c, d_src, src_off, src_len, nch, d_start, ch, st); if (rc) return rc; }
    SpecWhy w;
    auto why = [&](const char *what, uint64_t a, uint64_t b) {
        char t[192]; snprintf(t, sizeof t, "%s (%llu, %llu)", what, (unsigned long long)a, (unsigned long long)b); w.text = t;
        if (c->tun.trace) fprintf(stderr, "[pna inflate] stream of %llu B measured by one wave: %s\n", (unsigned long long)src_len, t);
    };
    bool ok = false;
    if (ch.size() >= 4) { rc = count_chunks(c, 0, ch, d_chunks, d_src, (ZBlock *)none, none, (uint64_t *)none, st, why, &ok); if (rc) return rc; }
    if (!ok && src_len > 0xFFFFFFFFull) {                                 // (the one-wave walk reads 32 bits' worth of a stream)
        for (const ISChunkH &h : ch) w.corrupt |= h.status == 1u;
        return big_unsplit(c, src_len, w);
    }
    if (!ok) {                                                            // one wave over the whole stream: its verdict stands
        ch.assign(1, ISChunkH{}); ch[0].end_bit = ~0ull;
        rc = run_chunks(c, 0, ch, std::vector<uint32_t>(), 0, d_chunks, d_src, (ZBlock *)none, none, (uint64_t *)none, st); if (rc) return rc;
        if (ch[0].status == 2) return fail(c, PNA_E_UNSUPPORTED, "zlib stream with a preset dictionary, or of more than 4 GiB of content and no block starts to split it at");
        if (ch[0].status) return fail(c, PNA_E_INVAL, "corrupt zlib stream (measuring its size)");
    }
    uint64_t out = 0;
    for (const ISChunkH &h : ch) out += (uint64_t)h.nlit + h.mtot;
    *size = out;
    return PNA_OK;
}

// ---------------------------------------------------------------------------------------------------------
// Read side, Compression::XZ: one .xz stream per entry (liblzma::bufread::XzDecoder, lib/src/entry/read.rs:171-190; include/pna_gpu.h says what is read).
// k_xzscan walks every stream's container (pass 1: status, blocks, decoded size, largest lc + lp -- read back once), the host makes room, pass 2 writes a
// descriptor per block; k_lzma2 decodes one block per wave, k_xzcheck / k_xzfin verify the blocks' checks and fold the statuses per stream.
struct XzStreamInH { uint64_t src_off, src_len, dst_off; uint32_t blk_base, blk_cap, piece_base, piece_cap; };   // = XzStreamIn of k_xz.hip
static_assert(sizeof(XzStreamInH) == 40 && sizeof(XzScan) == 32 && sizeof(XzBlock) == 56, "xz descriptor layouts");
static constexpr uint64_t XZ_PIECE_BYTES = 256u << 10;               // = XZ_PIECE of k_xz.hip
static const char *xz_unsup_text(uint32_t why) {
    switch (why) {
        case XZ_UNSUP_SHA256:    return "xz stream with a SHA-256 check (None, CRC32 and CRC64 are verified on the device)";
        case XZ_UNSUP_CHECK:     return "xz stream with a check of an unassigned type";
        case XZ_UNSUP_FILTER:    return "xz stream with a filter chain other than LZMA2 alone (Delta, BCJ)";
        case XZ_UNSUP_BIG_BLOCK: return "xz stream with a block of 4 GiB or more of decoded bytes";
        default:                 return "xz stream with header fields of a later format version";
    }
}
// pass 1 over n streams: their scan results
static int xz_scan_counts(pna_gpu_ctx *c, size_t n, const void *d_src, std::vector<XzStreamInH> &ins, std::vector<XzScan> &sc, hipStream_t st) {
    if (c->xz_in.ensure(n * sizeof(XzStreamInH)) || c->xz_scan.ensure(n * sizeof(XzScan))) return fail(c, PNA_E_NOMEM, "decoder workspace");
    HIPCHK(c, hipMemcpyAsync(c->xz_in.p, ins.data(), n * sizeof(XzStreamInH), hipMemcpyHostToDevice, st));
    HIPCHK(c, hipEventRecord(c->ev[0], st));
    launch_xzscan(c->xz_in.p, (uint32_t)n, (const uint8_t *)d_src, (XzScan *)c->xz_scan.p, nullptr, nullptr, st);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(c->ev[2], st));
    sc.resize(n);
    HIPCHK(c, hipMemcpyAsync(sc.data(), c->xz_scan.p, n * sizeof(XzScan), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    return PNA_OK;
}
// raw_len[i]: the decoded size (it must be the Index's total), or with `open` the room; why: which stream failed and for what reason, for a caller that names its streams
static int xz_decode_device(pna_gpu_ctx *c, const DecodeBatch &b, XzFail *why) {
    const size_t n = b.n; const void *d_src = b.d_src; void *d_dst = b.d_dst; const uint64_t *raw_len = b.raw_len; const bool open = b.open; hipStream_t st = b.st;
    if (!xz_kernels_present()) return fail(c, PNA_E_UNSUPPORTED, "only zstd and deflate streams are decoded on the device");
    if (n > 0x3FFFFFFFull) return fail(c, PNA_E_INVAL, "batch too large for one decode call");
    std::vector<XzStreamInH> ins(n);
    for (size_t i = 0; i < n; i++) ins[i] = XzStreamInH{b.src_off[i], b.src_len[i], b.dst_off[i], 0, 0, 0, 0};
    std::vector<XzScan> sc;
    int rc = xz_scan_counts(c, n, d_src, ins, sc, st); if (rc) return rc;
    std::vector<uint32_t> status(n);
    uint64_t nblk = 0, npieces = 0;
    uint32_t lclp = 0;
    for (size_t i = 0; i < n; i++) {
        status[i] = sc[i].status;
        if (!status[i] && (open ? sc[i].total > raw_len[i] : sc[i].total != raw_len[i])) status[i] = XZ_SIZE;
        if (status[i]) continue;
        ins[i].blk_base = (uint32_t)nblk; ins[i].blk_cap = sc[i].nblk; nblk += sc[i].nblk;
        if (sc[i].check != XZ_CHECK_NONE) {
            const uint64_t cap = sc[i].total / XZ_PIECE_BYTES + sc[i].nblk;
            if (cap > 0x7FFFFFFFull - npieces) return fail(c, PNA_E_INVAL, "batch too large for one decode call");
            ins[i].piece_base = (uint32_t)npieces; ins[i].piece_cap = (uint32_t)cap; npieces += cap;
        }
        lclp = std::max(lclp, sc[i].lclp);
        if (nblk > 0x7FFFFFFFull) return fail(c, PNA_E_INVAL, "batch too large for one decode call");
    }
    float ms_scan = 0, ms_dec = 0;
    (void)hipEventElapsedTime(&ms_scan, c->ev[0], c->ev[2]);
    if (nblk) {
        const size_t acc_bytes = (size_t)nblk * 8, stat_bytes = n * 4;
        if (c->xz_blocks.ensure((size_t)nblk * sizeof(XzBlock)) || c->xz_pieces.ensure((size_t)npieces * 8 + 8) || c->xz_acc.ensure(acc_bytes + stat_bytes))
            return fail(c, PNA_E_NOMEM, "decoder workspace");
        uint32_t *d_status = (uint32_t *)((uint8_t *)c->xz_acc.p + acc_bytes);
        HIPCHK(c, hipMemcpyAsync(c->xz_in.p, ins.data(), n * sizeof(XzStreamInH), hipMemcpyHostToDevice, st));
        HIPCHK(c, hipMemsetAsync(c->xz_acc.p, 0, acc_bytes + stat_bytes, st));
        HIPCHK(c, hipEventRecord(c->ev[3], st));
        launch_xzscan(c->xz_in.p, (uint32_t)n, (const uint8_t *)d_src, (XzScan *)c->xz_scan.p, (XzBlock *)c->xz_blocks.p, c->xz_pieces.p, st);
        launch_lzma2((XzBlock *)c->xz_blocks.p, (uint32_t)nblk, (const uint8_t *)d_src, (uint8_t *)d_dst, lclp, st);
        launch_xzcheck(c->xz_pieces.p, (uint32_t)npieces, (const XzBlock *)c->xz_blocks.p, (uint32_t)nblk, (const uint8_t *)d_src, (const uint8_t *)d_dst,
                       (uint64_t *)c->xz_acc.p, d_status, st);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipEventRecord(c->ev[1], st));
        std::vector<uint32_t> dev(n);
        HIPCHK(c, hipMemcpyAsync(dev.data(), d_status, stat_bytes, hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipStreamSynchronize(st));
        (void)hipEventElapsedTime(&ms_dec, c->ev[3], c->ev[1]);
        for (size_t i = 0; i < n; i++) if (!status[i]) status[i] = dev[i];
    }
    c->forms = pna_gpu_decode_forms{};
    c->timing = pna_gpu_timing{}; c->timing.ms_lz = ms_scan + ms_dec; c->timing.ms_stats = ms_scan; c->timing.ms_lit = ms_dec;   // the xz kernels, the first scan, the rest
    if (b.ent_status) for (size_t i = 0; i < n; i++) b.ent_status[i] = status[i];
    for (size_t i = 0; i < n && !b.ent_status; i++)
        if (status[i]) {
            char reason[192];
            if (status[i] == XZ_UNSUPPORTED) snprintf(reason, sizeof reason, "%s", xz_unsup_text(sc[i].why));
            else if (status[i] == XZ_SIZE) snprintf(reason, sizeof reason, "size mismatch (the xz stream's Index adds up to %llu bytes, %s %llu)", (unsigned long long)sc[i].total,
                                                    open ? "the room is" : "expected", (unsigned long long)raw_len[i]);
            else snprintf(reason, sizeof reason, "corrupt xz stream");
            if (why) { why->index = i; why->reason = reason; }
            return fail(c, status[i] == XZ_UNSUPPORTED ? PNA_E_UNSUPPORTED : PNA_E_INVAL, ("entry " + std::to_string(i) + ": " + reason).c_str());
        }
    if (open && b.raw_out) for (size_t i = 0; i < n; i++) b.raw_out[i] = sc[i].total;
    return PNA_OK;
}
// the decoded size of one xz stream: the sum of its Index records, after the whole container walk -- exact, nothing is decoded
static int xz_measure(pna_gpu_ctx *c, const void *d_src, uint64_t src_off, uint64_t src_len, uint64_t *size, hipStream_t st) {
    std::vector<XzStreamInH> ins(1, XzStreamInH{src_off, src_len, 0, 0, 0, 0, 0});
    std::vector<XzScan> sc;
    const int rc = xz_scan_counts(c, 1, d_src, ins, sc, st); if (rc) return rc;
    if (sc[0].status == XZ_UNSUPPORTED) return fail(c, PNA_E_UNSUPPORTED, xz_unsup_text(sc[0].why));
    if (sc[0].status) return fail(c, PNA_E_INVAL, "corrupt xz stream (measuring its size)");
    *size = sc[0].total;
    return PNA_OK;
}

int pna::open_size(pna_gpu_ctx *c, int algo, const void *d_src, uint64_t src_off, uint64_t src_len, OpenSize *m, hipStream_t st) {
    *m = OpenSize();
    if (algo == PNA_ALGO_STORE) { m->size = src_len; m->exact = 1; return PNA_OK; }
    if (algo == PNA_ALGO_XZ && xz_kernels_present()) {
        const int rc = xz_measure(c, d_src, src_off, src_len, &m->size, st); if (rc) return rc;
        m->exact = 1;
        return PNA_OK;
    }
    if (algo != PNA_ALGO_ZSTD && algo != PNA_ALGO_DEFLATE) return fail(c, PNA_E_UNSUPPORTED, "only zstd, deflate and stored streams are measured");
    if (algo == PNA_ALGO_DEFLATE) {
        const int rc = inflate_measure(c, d_src, src_off, src_len, &m->size, st); if (rc) return rc;
        m->exact = 1;
        return PNA_OK;
    }
    if (!launch_zsize) return fail(c, PNA_E_UNSUPPORTED, "this build has no k_zsize");
    if (c->z_work.ensure(64)) return fail(c, PNA_E_NOMEM, "measurement workspace");
    unsigned long long o[5] = {0, 0, 0, 0, 0};
    launch_zsize((const uint8_t *)d_src, src_off, src_len, (unsigned long long *)c->z_work.p, st);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(o, c->z_work.p, sizeof o, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    if (o[2]) return fail(c, PNA_E_INVAL, "corrupt stream (not a sequence of well-formed zstd frames)");
    m->size = o[0]; m->exact = o[1] ? 1 : 0; m->frames = o[3]; m->last = o[4];
    return PNA_OK;
}

// A caller's base address, aligned or not, as a 16-byte aligned base and what its low bits add to every offset: the kernels take their aligned words and
// groups from base + offset, some from the offset alone (k_inflate), some from the address (k_zhuf, k_zx_emit) -- with an aligned base the two agree.
template <class T> static uint64_t fold_base(T *&p) { const uint64_t m = (uint64_t)((uintptr_t)p & 15u); p = (T *)((uintptr_t)p - m); return m; }
extern "C" int pna_gpu_open_size_device(pna_gpu_ctx *c, int algo, const void *d_src, uint64_t src_off, uint64_t src_len, uint64_t *size, int *exact, void *hip_stream) {
    if (!c || (!d_src && src_len) || !size || !exact) return fail(c, PNA_E_INVAL, "null argument");
    *size = 0; *exact = 0;
    HIPCHK(c, hipSetDevice(c->device));
    if (d_src) src_off += fold_base(d_src);
    OpenSize m;
    const int rc = open_size(c, algo, d_src, src_off, src_len, &m, hip_stream ? (hipStream_t)hip_stream : c->stream); if (rc) return rc;
    *size = m.size; *exact = m.exact;
    return PNA_OK;
}

// A zstd stream whose decoded size is not recorded anywhere (the SDAT stream of a solid entry: SHED carries no size): step 1 counts
// its frames, the caller provides frames x 1 MiB (this library's segmentation; one frame of any size: `cap` bytes), step 2 decodes
// and reports the size found.
extern "C" int pna_gpu_zstd_stream_frames_device(pna_gpu_ctx *c, const void *d_src, uint64_t src_off, uint64_t src_len, uint32_t *n_frames, void *hip_stream) {
    if (!c || !d_src || !n_frames) return fail(c, PNA_E_INVAL, "null argument");
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : c->stream;
    if (c->z_ents.ensure(sizeof(ZEntry)) || c->z_work.ensure(64)) return fail(c, PNA_E_NOMEM, "decoder workspace");
    const ZEntry en{src_off, src_len, 0, 0, 0, 0, 1, 0};
    HIPCHK(c, hipMemcpyAsync(c->z_ents.p, &en, sizeof en, hipMemcpyHostToDevice, st));
    launch_zcount((const ZEntry *)c->z_ents.p, 1, (const uint8_t *)d_src, (uint32_t *)c->z_work.p, st);
    HIPCHK(c, hipMemcpyAsync(n_frames, c->z_work.p, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    if (*n_frames == 0 && src_len) return fail(c, PNA_E_INVAL, "not a sequence of zstd frames");
    return PNA_OK;
}
// ---------------------------------------------------------------------------------------------------------
// Read side: decompress_reader (lib/src/entry/read.rs:171-190); entries already in device memory.  allow_foreign: payloads k_zscan could not place go through zstd_decode_foreign
// (which decodes their frames with this function again, allow_foreign off); b.plan: the measurement of an open stream (n = 1) -- how many frames it has, what the last one holds.
static int zstd_decode_device(pna_gpu_ctx *c, const DecodeBatch &b, bool allow_foreign);
// A payload k_zscan could not place -- frames of other sizes than this library's grid, skippable frames between them: anything zstd::stream::read::Decoder
// reads (lib/src/entry/read.rs:171-190) --: its frames are listed (k_zlist), every run of frames whose headers carry a content size is decoded as one batch of
// single-frame entries (the pipeline above, side by side), a frame without one on its own with an open size (its content's length is only known once it is
// decoded), one after the other.  Entry i of batch b: its room is raw_len[i] (open: its capacity); *found = the bytes produced.
static int zstd_decode_foreign(pna_gpu_ctx *c, const DecodeBatch &b, size_t i, uint64_t *found, bool *size_mismatch) {
    struct Item { uint64_t off, len, fcs; };
    constexpr uint32_t CAP = 4096;
    const uint64_t src_off = b.src_off[i], src_len = b.src_len[i], dst_off = b.dst_off[i], room = b.raw_len[i]; hipStream_t st = b.st;
    if (c->z_list.ensure(CAP * sizeof(Item) + 64)) return fail(c, PNA_E_NOMEM, "decoder workspace");
    uint64_t *d_hdr = (uint64_t *)((uint8_t *)c->z_list.p + CAP * sizeof(Item));
    std::vector<Item> items(CAP);
    uint64_t ip = 0, produced = 0;
    // (verdict mode, size_mismatch given: the frames' own statuses, so that a frame that overflows the entry's size is told from a corrupt one)
    auto decode_frames = [&](DecodeBatch run) {
        std::vector<uint32_t> fst(size_mismatch ? run.n : 0); if (size_mismatch) run.ent_status = fst.data();
        const int rc = zstd_decode_device(c, run, false); if (rc) return rc;
        for (uint32_t v : fst) if (v) { *size_mismatch = v == 3; return fail(c, v == 2 ? PNA_E_UNSUPPORTED : PNA_E_INVAL, "corrupt or mis-sized frame"); }
        return (int)PNA_OK;
    };
    for (;;) {
        uint64_t hdr[3] = {0, 0, 0};
        launch_zlist((const uint8_t *)b.d_src, src_off, src_len, ip, c->z_list.p, CAP, d_hdr, st);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipMemcpyAsync(hdr, d_hdr, sizeof hdr, hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipStreamSynchronize(st));
        if (hdr[2]) return fail(c, PNA_E_INVAL, "corrupt stream (not a sequence of zstd frames)");
        const size_t k = (size_t)hdr[0];
        if (k) { HIPCHK(c, hipMemcpyAsync(items.data(), c->z_list.p, k * sizeof(Item), hipMemcpyDeviceToHost, st)); HIPCHK(c, hipStreamSynchronize(st)); }
        for (size_t a = 0; a < k;) {
            if (items[a].fcs != ~0ull) {                                  // a run of frames that say what they hold: one batch
                size_t e = a; uint64_t pos = produced;
                std::vector<uint64_t> so, sl, dof, rl;
                while (e < k && items[e].fcs != ~0ull) {
                    if (items[e].fcs > room - pos) { if (size_mismatch) *size_mismatch = true; return fail(c, PNA_E_INVAL, "size mismatch: the frames hold more than the entry's size"); }
                    so.push_back(items[e].off); sl.push_back(items[e].len); dof.push_back(dst_off + pos); rl.push_back(items[e].fcs); pos += items[e].fcs; e++;
                }
                const int rc = decode_frames(DecodeBatch{so.size(), b.d_src, so.data(), sl.data(), b.d_dst, dof.data(), rl.data(), false, nullptr, nullptr, st}); if (rc) return rc;
                produced = pos; a = e;
            } else {                                                      // no content size in the header: decoded with an open size
                uint64_t cap = room - produced, got = 0, dof = dst_off + produced;
                const int rc = decode_frames(DecodeBatch{1, b.d_src, &items[a].off, &items[a].len, b.d_dst, &dof, &cap, true, &got, nullptr, st}); if (rc) return rc;
                produced += got; a++;
            }
        }
        ip = hdr[1];
        if (ip >= src_len) break;
        if (k == 0) return fail(c, PNA_E_INVAL, "corrupt stream");        // (no progress: cannot happen with hdr[2] == 0)
    }
    if (!b.open && produced != room) { if (size_mismatch) *size_mismatch = true; return fail(c, PNA_E_INVAL, "size mismatch (the frames do not add up to the entry's size)"); }
    *found = produced;
    return PNA_OK;
}

struct ZstdRun {
    pna_gpu_ctx *c; const DecodeBatch &b; const uint8_t *src; uint8_t *dst; bool allow_foreign;
    std::vector<ZEntry> ents; std::vector<ZFrameX> fxs, fxd;                             // the frames' shares of the workspace as planned; as read back behind k_zparse_a (the large frames' blocks)
    std::vector<ZFrame> frs;                                         // the frames as the device has them, read back
    uint64_t nfr = 0, nblk_cap = 0, nslot = 0, nseq_cap = 0, out_span = 0;
    std::vector<uint32_t> big;                                       // large frames: parsed side by side, executed by the parallel executor
    uint64_t n_par = 0, n_fallback = 0;                              // frames the parallel executor executed, frames the one-workgroup kernel decoded: pna_gpu_last_decode_forms
    // host arithmetic: frames per entry, every frame's share of the workspace, the batch limits
    int plan() {
        ents.resize(b.n);
        for (size_t i = 0; i < b.n; i++) {
            uint64_t k = b.raw_len[i] ? (b.raw_len[i] + SEG_SIZE - 1) / SEG_SIZE : 1;
            // a measured stream of several frames (b.plan: n = 1): one slot per frame, 1 MiB each but the last, which gets its own measured room -- a stream
            // that does not have this library's shape goes through zstd_decode_foreign with all of raw_len
            if (b.plan && b.plan->frames > 1) k = b.plan->frames;
            if (nfr + k > 0x7FFFFFFFull) return fail(c, PNA_E_INVAL, "too many frames");
            const uint64_t room = b.plan && b.plan->frames > 1 ? std::min<uint64_t>(b.raw_len[i], (k - 1) * SEG_SIZE + b.plan->last) : b.raw_len[i];
            ents[i] = ZEntry{b.src_off[i], b.src_len[i], b.dst_off[i], room, (uint32_t)nfr, (uint32_t)k, b.open ? 1u : 0u, 0u};
            nfr += k;
        }
        // per-frame bounds of the lane-parallel pipeline (frames that exceed them fall back to the one-workgroup-per-frame kernel).  They are planned per MiB of
        // content -- 260 block descriptors, 10 table sets, 262 160 sequence records -- and ONE frame that holds an entry gets the sum (k_zscan, each sum saturated
        // at 2^31 - 1).  One frame of 8 GiB: 2.1 M descriptors for its 65 536 blocks of 128 KiB, 81 920 table sets (it needs a set per block at most), and
        // 2^31 - 1 records: the records' sum saturates from 8 GiB of content on, so a frame with more sequences than that -- one per four bytes of 8 GiB -- goes
        // to the fallback (k_zparse_a finds out).  The batch limit below, 2^30 - 1 descriptors, is 4 TiB of content.  The min() of a single slot only binds where a
        // measured stream's last frame gets room of its own (b.plan): 2^20 descriptors = 128 GiB of 128 KiB blocks, 2^16 table sets.  Compressed bytes and literals
        // are not bounded here: the header walk and the literal scratch (z_lit: as long as the output span) count in 64 bits.
        fxs.resize(nfr);
        for (size_t i = 0; i < b.n; i++) {
            const uint64_t room = ents[i].raw_len;
            out_span = std::max<uint64_t>(out_span, b.dst_off[i] + room);
            for (uint32_t f = 0; f < ents[i].n_frames; f++) {
                const uint64_t done = (uint64_t)f * SEG_SIZE;
                const uint64_t dl = (f + 1 == ents[i].n_frames) ? (room > done ? room - done : 0) : SEG_SIZE;
                ZFrameX &x = fxs[ents[i].first_frame + f];
                x.blk_base = (uint32_t)nblk_cap; x.blk_cap = (uint32_t)std::min<uint64_t>((dl >> 12) + 4, 1u << 20);
                x.slot_base = (uint32_t)nslot; x.slot_cap = (uint32_t)std::min<uint64_t>((dl >> 17) + 2, 1u << 16);
                x.seq_base = nseq_cap; x.seq_cap = (uint32_t)std::min<uint64_t>(dl / 4 + 16, 0x7FFFFFFFu); x.nblk = 0;
                nblk_cap += x.blk_cap; nslot += x.slot_cap; nseq_cap += x.seq_cap;
                if (nblk_cap > 0x3FFFFFFFull) return fail(c, PNA_E_INVAL, "batch too large for one decode call");
            }
        }
        return PNA_OK;
    }
    // the workspace, the plan's upload, and k_zscan: every frame's header walked, its ZFrame written
    int workspace_and_scan() {
        if (c->z_ents.ensure(b.n * sizeof(ZEntry)) || c->z_frames.ensure(nfr * sizeof(ZFrame)) || c->z_lit.ensure(out_span + 64) ||
            c->z_fx.ensure(nfr * sizeof(ZFrameX)) || c->z_blocks.ensure(nblk_cap * sizeof(ZBlock)) || c->z_tabs.ensure(nslot * sizeof(ZTables)) ||
            c->z_seqs.ensure(nseq_cap * 8 + 64) || c->z_hlist.ensure(nblk_cap * 16 + 16) || c->z_slist.ensure(nblk_cap * 4 + 16) || c->z_work.ensure(64))
            return fail(c, PNA_E_NOMEM, "decoder workspace");
        HIPCHK(c, hipMemcpyAsync(c->z_ents.p, ents.data(), b.n * sizeof(ZEntry), hipMemcpyHostToDevice, b.st));
        HIPCHK(c, hipMemcpyAsync(c->z_fx.p, fxs.data(), nfr * sizeof(ZFrameX), hipMemcpyHostToDevice, b.st));
        HIPCHK(c, hipMemsetAsync(c->z_work.p, 0, 64, b.st));
        launch_zscan((const ZEntry *)c->z_ents.p, (uint32_t)b.n, src, zframes(c), zfx(c), b.st);
        HIPCHK(c, hipEventRecord(c->ev[0], b.st));
        frs.resize(nfr);
        return PNA_OK;
    }
    // (not a stage: the frames as the device has them now; all_to_fallback -- diagnostics, zdec_serial, instead of the three stages below --: every well-formed frame is routed through the fallback)
    int read_frames(bool all_to_fallback) {
        HIPCHK(c, hipMemcpyAsync(frs.data(), c->z_frames.p, nfr * sizeof(ZFrame), hipMemcpyDeviceToHost, b.st));
        HIPCHK(c, hipStreamSynchronize(b.st));
        for (auto &fr : frs) if (all_to_fallback && fr.status == 0) fr.status = 2;
        return PNA_OK;
    }
    // Large frames (the reference writes ONE frame per entry whatever its size): k_zscan has found them -- a frame whose content takes zexec_par_min_mib
    // and more, of any content, compressed and literal size (the executor works in windows, the header walk counts in 64 bits).  Their blocks are PARSED side by side (k_zparse_a: the header walk,
    // k_zparse<true>: a wave per block for the tables) and their sequences EXECUTED in parallel by pointer jumping (k_zexec_par.hip) instead of by one
    // wave each; the per-frame kernels skip them (ZFrameX::pad).
    int mark_large_frames() {
        const uint64_t big_min = (uint64_t)c->tun.zexec_par_min_mib << 20;
        bool any = false;
        for (size_t i = 0; i < b.n && !any; i++) any = c->tun.zexec_par_min_mib > 0 && ents[i].raw_len >= big_min;
        if (!any) return PNA_OK;
        const int rc = read_frames(false); if (rc) return rc;
        for (uint64_t f = 0; f < nfr; f++)
            if (frs[f].status == 0 && frs[f].dst_len >= big_min) big.push_back((uint32_t)f);            // (any size: the executor works in windows of 1 GiB)
        if (big.empty()) return PNA_OK;
        if (c->z_big.ensure(big.size() * 4 + 64) || c->z_one.ensure(nblk_cap * 4 + 64)) return fail(c, PNA_E_NOMEM, "decoder workspace");
        for (uint32_t f : big) HIPCHK(c, poke32(&zfx(c)[f].pad, 1u, b.st));
        HIPCHK(c, hipMemcpyAsync(c->z_big.p, big.data(), big.size() * 4, hipMemcpyHostToDevice, b.st));
        return PNA_OK;
    }
    // the bounded pipeline: block headers and tables (k_zparse; the large frames' by k_zparse_a / _b), literal and sequence streams (k_zstreams), execution (k_zexec)
    int parse_and_execute() {
        uint32_t *hlist = (uint32_t *)c->z_hlist.p, *slist = (uint32_t *)c->z_slist.p, *one = (uint32_t *)c->z_one.p; ZTables *tabs = (ZTables *)c->z_tabs.p;
        // sequence records of frame f start at seq_base: k_zparse adds it to the block's running count
        launch_zparse(zframes(c), zfx(c), (uint32_t)nfr, src, zblocks(c), tabs, hlist, slist, c->z_work.p, b.st);
        uint32_t work[4] = {0, 0, 0, 0};
        if (!big.empty()) {
            launch_zparse_big_a(zframes(c), zfx(c), (const uint32_t *)c->z_big.p, (uint32_t)big.size(), src, zblocks(c), one, c->z_work.p, b.st);
            fxd.resize(nfr);
            HIPCHK(c, hipMemcpyAsync(work, c->z_work.p, 16, hipMemcpyDeviceToHost, b.st));
            HIPCHK(c, hipMemcpyAsync(fxd.data(), c->z_fx.p, nfr * sizeof(ZFrameX), hipMemcpyDeviceToHost, b.st));
            HIPCHK(c, hipStreamSynchronize(b.st));
            launch_zparse_big_b(zframes(c), zfx(c), work[2], src, zblocks(c), tabs, hlist, slist, c->z_work.p, one, b.st);
        }
        HIPCHK(c, hipMemcpyAsync(work, c->z_work.p, 16, hipMemcpyDeviceToHost, b.st));
        HIPCHK(c, hipStreamSynchronize(b.st));
        launch_zstreams(work[0], work[1], hlist, slist, c->z_work.p, zblocks(c), zframes(c), tabs, src, zlit(c), zseqs(c), b.st);
        launch_zexec(zframes(c), zfx(c), (uint32_t)nfr, zblocks(c), src, zlit(c), zseqs(c), dst, b.st);
        return PNA_OK;
    }
    // the large frames' sequences through the parallel executor, one frame after the other; then the content checksums of the frames that carry one (k_zxxh), and the frames back
    int execute_large_frames_and_checksum() {
        int rc = big.empty() ? (int)PNA_OK : read_frames(false); if (rc) return rc;   // (k_zoff has fixed the sizes of open frames)
        for (uint32_t f : big) {
            if (frs[f].status) continue;
            uint32_t zst = 0;
            rc = exec_par_frame(c, ZxFrame{frs[f].dst_off, frs[f].dst_len, fxd[f].blk_base, fxd[f].nblk, 0, 0}, b.d_src, b.d_dst, b.st, &zst, "parallel frame execution failed"); if (rc) return rc;
            n_par += zst == 0;
            if (zst) HIPCHK(c, poke32(&zframes(c)[f].status, zst == 2 ? 2u : 1u, b.st));   // 2: the serial kernel takes the frame (it decodes from the source again); 3: corrupt
        }
        launch_zxxh(zframes(c), (uint32_t)nfr, src, dst, b.st);
        HIPCHK(c, hipGetLastError());
        return read_frames(false);
    }
    // ---- frames the bounded pipeline could not take: one workgroup per frame
    int fallback() {
        std::vector<uint32_t> fb;
        for (uint64_t f = 0; f < nfr; f++) if (frs[f].status == 2) fb.push_back((uint32_t)f);
        if (c->tun.zdec_fallback_max_mib > 0)
            for (uint32_t f : fb) if (frs[f].dst_len > ((uint64_t)c->tun.zdec_fallback_max_mib << 20)) {
                char msg[160];
                snprintf(msg, sizeof msg, "frame %u: %llu bytes of content would be decoded by one workgroup (option zdec_fallback_max_mib)", f, (unsigned long long)frs[f].dst_len);
                return fail(c, PNA_E_UNSUPPORTED, msg);
            }
        if (fb.empty()) return PNA_OK;
        n_fallback = fb.size();
        std::vector<ZFrame> sub(fb.size());
        for (size_t k = 0; k < fb.size(); k++) { sub[k] = frs[fb[k]]; sub[k].status = 0; sub[k].out_len = 0; }
        if (b.open)                                                   // the frame that closes a stream of unknown size keeps its flag
            for (size_t k = 0; k < fb.size(); k++)
                for (size_t i = 0; i < b.n; i++) {
                    const uint32_t f0 = ents[i].first_frame, f1 = f0 + ents[i].n_frames;
                    if (fb[k] >= f0 && fb[k] < f1 && (fb[k] + 1 == f1 || (fb[k] == f0 && f1 - f0 > 1 && frs[f0 + 1].status == 4))) sub[k].out_len = ZF_OPEN;
                }
        if (c->z_fb.ensure(sub.size() * sizeof(ZFrame)) || c->z_lit.ensure(std::max<uint64_t>(out_span + 64, sub.size() * (uint64_t)(128u << 10) + 64)))
            return fail(c, PNA_E_NOMEM, "decoder workspace");
        HIPCHK(c, hipMemcpyAsync(c->z_fb.p, sub.data(), sub.size() * sizeof(ZFrame), hipMemcpyHostToDevice, b.st));
        launch_zdec((ZFrame *)c->z_fb.p, (uint32_t)sub.size(), src, dst, zlit(c), (uint32_t)c->tun.zdec_dbg, b.st);
        launch_zxxh((ZFrame *)c->z_fb.p, (uint32_t)sub.size(), src, dst, b.st);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipMemcpyAsync(sub.data(), c->z_fb.p, sub.size() * sizeof(ZFrame), hipMemcpyDeviceToHost, b.st));
        HIPCHK(c, hipStreamSynchronize(b.st));
        for (size_t k = 0; k < fb.size(); k++) frs[fb[k]] = sub[k];
        return PNA_OK;
    }
    // The call's time, then what the caller gets, entry by entry: the foreign path for a payload k_zscan could not place, verdict mode -- this entry's status, the
    // others go on --, or the first bad frame as the call's failure; the sizes found.
    int settle() {
        const size_t n = b.n; HIPCHK(c, hipEventRecord(c->ev[1], b.st));
        HIPCHK(c, hipStreamSynchronize(b.st));
        float ms = 0; (void)hipEventElapsedTime(&ms, c->ev[0], c->ev[1]);
        c->timing = pna_gpu_timing{}; c->timing.ms_lz = ms;            // decoder time reported in the first stage slot
        pna_gpu_decode_forms forms{}; forms.zstd_executor_frames = n_par; forms.zstd_workgroup_frames = n_fallback;   // (the frame list below runs decode calls of its own)
        c->forms = forms;
        std::vector<uint64_t> foreign_len(n, ~0ull);                  // entries that went through zstd_decode_foreign: the bytes they produced
        const pna_gpu_timing outer_timing = c->timing;                // (the foreign path runs decode calls of its own: this call's timing stays what it measured)
        if (b.ent_status) for (size_t i = 0; i < n; i++) b.ent_status[i] = 0;
        for (size_t i = 0; i < n; i++)
            for (uint32_t f = 0; f < ents[i].n_frames; f++) {
                const ZFrame &fr = frs[ents[i].first_frame + f];
                if (allow_foreign && (fr.status == 1 || fr.status == 3)) {
                    // not one of the two shapes k_zscan places (or a frame of the grid walk did not hold its MiB): the payload's frames as they are
                    uint64_t got = 0; bool mism = false;
                    const int rcf = zstd_decode_foreign(c, b, i, &got, b.ent_status ? &mism : nullptr);
                    c->timing = outer_timing; forms.zstd_listed_entries++; c->forms = forms;
                    if (rcf && b.ent_status && (rcf == PNA_E_INVAL || rcf == PNA_E_UNSUPPORTED)) { b.ent_status[i] = rcf == PNA_E_UNSUPPORTED ? 2u : (mism ? 3u : 1u); break; }
                    if (rcf) return rcf;
                    foreign_len[i] = got; break;
                }
                if (fr.status && fr.status != 4 && b.ent_status) { b.ent_status[i] = fr.status; break; }
                if (fr.status && fr.status != 4) return fail_status(c, "entry " + std::to_string(i) + " frame " + std::to_string(f), fr, "size mismatch (foreign multi-frame stream?)");   // 4: void slot behind a single frame that holds the whole entry
            }
        if (b.open && b.raw_out)
            for (size_t i = 0; i < n; i++) {                          // sizes found by the decoder: frames in front hold SEG_SIZE each
                if (foreign_len[i] != ~0ull) { b.raw_out[i] = foreign_len[i]; continue; }
                uint64_t total = 0;
                for (uint32_t f = 0; f < ents[i].n_frames; f++) { const ZFrame &fr = frs[ents[i].first_frame + f]; if (fr.status != 4) total += fr.dst_len; }
                b.raw_out[i] = total;
            }
        return PNA_OK;
    }
};
static int zstd_decode_device(pna_gpu_ctx *c, const DecodeBatch &b, bool allow_foreign) {
    ZstdRun r{c, b, (const uint8_t *)b.d_src, (uint8_t *)b.d_dst, allow_foreign};
    int rc = r.plan(); if (rc) return rc;
    rc = r.workspace_and_scan(); if (rc) return rc;
    if (c->tun.zdec_serial != 0) { rc = r.read_frames(true); if (rc) return rc; }
    else {
        rc = r.mark_large_frames(); if (rc) return rc;
        rc = r.parse_and_execute(); if (rc) return rc;
        rc = r.execute_large_frames_and_checksum(); if (rc) return rc;
    }
    rc = r.fallback(); if (rc) return rc;
    return r.settle();
}
// ---------------------------------------------------------------------------------------------------------
// One batch to its codec's decoder (the caller has set the device).  Verdict mode (b.ent_status, `pna verify`): ent_status[i] = stream i's status (0 good,
// 1 corrupt, 2 unsupported, 3 size mismatch) instead of a failure of the call at the first bad stream; workspace, HIP and batch-shape errors still fail the call.
int pna::decode_batch(pna_gpu_ctx *c, int algo, const DecodeBatch &b, XzFail *why) {
    if (!b.n) return PNA_OK;
    if (algo == PNA_ALGO_XZ) return xz_decode_device(c, b, why);
    if (algo == PNA_ALGO_DEFLATE) return inflate_batch_device(c, b);
    return zstd_decode_device(c, b, true);
}
extern "C" int pna_gpu_decompress_batch_device(pna_gpu_ctx *c, int algo, size_t n, const void *d_src, const uint64_t *src_off, const uint64_t *src_len, void *d_dst, const uint64_t *dst_off, const uint64_t *raw_len, void *hip_stream) {
    if (!c || (n && (!d_src || !src_off || !src_len || !d_dst || !dst_off || !raw_len))) return fail(c, PNA_E_INVAL, "null argument");
    if (algo != PNA_ALGO_ZSTD && algo != PNA_ALGO_DEFLATE && !(algo == PNA_ALGO_XZ && xz_kernels_present())) return fail(c, PNA_E_UNSUPPORTED, "only zstd and deflate streams are decoded on the device");
    if (!n) return PNA_OK;
    HIPCHK(c, hipSetDevice(c->device));
    std::vector<uint64_t> so, dof;                                    // (only for a base that is not 16-byte aligned)
    if (const uint64_t m = fold_base(d_src)) { so.assign(src_off, src_off + n); for (uint64_t &v : so) v += m; src_off = so.data(); }
    if (const uint64_t m = fold_base(d_dst)) { dof.assign(dst_off, dst_off + n); for (uint64_t &v : dof) v += m; dst_off = dof.data(); }
    return decode_batch(c, algo, DecodeBatch{n, d_src, src_off, src_len, d_dst, dst_off, raw_len, false, nullptr, nullptr, hip_stream ? (hipStream_t)hip_stream : c->stream});
}
// One stream whose decoded size is recorded nowhere (entries without fSIZ, solid streams), decoded into dst_cap bytes of room; the size found is reported (PNA_E_INVAL when it does
// not fit): zstd -- the caller provides frames x 1 MiB (pna_gpu_zstd_stream_frames_device; one frame of any size: its size) --, zlib, and xz (the size: the sum of its Index records).
static int open_device(pna_gpu_ctx *c, int algo, const void *d_src, uint64_t src_off, uint64_t src_len, void *d_dst, uint64_t dst_off, uint64_t dst_cap, uint64_t *raw_len, void *hip_stream) {
    if (!c || !d_src || !d_dst || !raw_len) return fail(c, PNA_E_INVAL, "null argument");
    HIPCHK(c, hipSetDevice(c->device));
    src_off += fold_base(d_src); dst_off += fold_base(d_dst);
    return decode_batch(c, algo, DecodeBatch{1, d_src, &src_off, &src_len, d_dst, &dst_off, &dst_cap, true, raw_len, nullptr, hip_stream ? (hipStream_t)hip_stream : c->stream});
}
extern "C" int pna_gpu_zstd_decompress_open_device(pna_gpu_ctx *c, const void *d_src, uint64_t src_off, uint64_t src_len, void *d_dst, uint64_t dst_off, uint64_t dst_cap, uint64_t *raw_len, void *hip_stream) {
    return open_device(c, PNA_ALGO_ZSTD, d_src, src_off, src_len, d_dst, dst_off, dst_cap, raw_len, hip_stream);
}
extern "C" int pna_gpu_inflate_open_device(pna_gpu_ctx *c, const void *d_src, uint64_t src_off, uint64_t src_len, void *d_dst, uint64_t dst_off, uint64_t dst_cap, uint64_t *raw_len, void *hip_stream) {
    return open_device(c, PNA_ALGO_DEFLATE, d_src, src_off, src_len, d_dst, dst_off, dst_cap, raw_len, hip_stream);
}
extern "C" int pna_gpu_xz_decompress_open_device(pna_gpu_ctx *c, const void *d_src, uint64_t src_off, uint64_t src_len, void *d_dst, uint64_t dst_off, uint64_t dst_cap, uint64_t *raw_len, void *hip_stream) {
    return open_device(c, PNA_ALGO_XZ, d_src, src_off, src_len, d_dst, dst_off, dst_cap, raw_len, hip_stream);
}

// The same for payloads in host memory (extract / verify of an archive read from disk).
extern "C" int pna_gpu_decompress_batch(pna_gpu_ctx *c, int algo, size_t n, const void *const *src, const size_t *src_len, void *const *dst, const size_t *raw_len) {
    if (!c || (n && (!src || !src_len || !dst || !raw_len))) return fail(c, PNA_E_INVAL, "null argument");
    if (algo != PNA_ALGO_ZSTD && algo != PNA_ALGO_DEFLATE && !(algo == PNA_ALGO_XZ && xz_kernels_present())) return fail(c, PNA_E_UNSUPPORTED, "only zstd and deflate streams are decoded on the device");
    HIPCHK(c, hipSetDevice(c->device));
    std::vector<uint64_t> so(n), sl(n), dof(n), rl(n);
    uint64_t sp = 0, dp = 0;
    for (size_t i = 0; i < n; i++) { so[i] = sp; sl[i] = src_len[i]; sp = (sp + src_len[i] + 15) & ~(uint64_t)15; dof[i] = dp; rl[i] = raw_len[i]; dp = (dp + raw_len[i] + 15) & ~(uint64_t)15; }
    if (c->stage_in.ensure(sp + 64) || c->stage_out.ensure(dp + 64)) return fail(c, PNA_E_NOMEM, "staging allocation failed");
    for (size_t i = 0; i < n; i++) if (src_len[i]) HIPCHK(c, hipMemcpyAsync((uint8_t *)c->stage_in.p + so[i], src[i], src_len[i], hipMemcpyHostToDevice, c->stream));
    const int rc = pna_gpu_decompress_batch_device(c, algo, n, c->stage_in.p, so.data(), sl.data(), c->stage_out.p, dof.data(), rl.data(), nullptr); if (rc) return rc;
    for (size_t i = 0; i < n; i++) if (raw_len[i]) HIPCHK(c, hipMemcpyAsync(dst[i], (uint8_t *)c->stage_out.p + dof[i], raw_len[i], hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return PNA_OK;
}

