// pna_lz.cpp -- the host side of the LZ stage, in one place: the level's parameter set (LzSet), the launch flag word, and the one decision path from a sub-batch's
// plan to its launches (lz_run).  A launch is described by an LzLaunch (pna_dev.h) that names its form; the launch layer (k_lz.hip, k_lz_split.hip) picks the kernel
// instance by the flag word (lz_common.h lz_instance) and decides nothing else.
//   lz_run      units (latency mode): ONE launch over the units -- the one-kernel form, the max set the split form -- and the short segments behind it;
//               whole segments: lz_stage
//   lz_stage    choose the form (lz_choose), size the runs (lz_run_blocks), then per run: the workspace or a shorter run / the one-kernel form (lz_workspace),
//               the timing events, the tail units (lz_tail_units), the launches (lz_split_run); what no split run took goes through the one-kernel form and the
//               short segments' pass (lz_one_kernel)
// All forms give the same bytes (tests/test_gpu_parity.py); tests/san's launch matrix pins every launch of every branch here.
#include "pna_ctx.h"
#include "xz_enc_core.h"

// option mtile as the launch flag of k_lzm (FLAG_MT_SHIFT): only where the match finder's table lies in LDS
static uint32_t mtile_flag(const pna_gpu_ctx *c, bool gt) {
    uint32_t k = 0;
    for (long v = c->tun.mtile; v >= 256; v >>= 1) k++;
    return gt ? 0u : k << FLAG_MT_SHIFT;
}

// zstd light / default run the match finder's 32 KiB-window geometry, high the 16 KiB one (lz_common.h LzGeo), both with the PACKED table (three 21-bit
// entries per 64-bit LDS word: 49 062 / 55 206 slots; option tab3 = 0: 32-bit entries, 32 704 / 36 800); the others and deflate the 64 KiB geometry (24 512);
// max the table in global memory.  (The level sets themselves: level_flags, pna_host.cpp.)
constexpr int HIGH_FROM = 4;        // the first zstd level of the high set
LzSet lz_level_set(const pna_gpu_ctx *c, int algo, int level, bool xz) {
    const bool zstd = algo != PNA_ALGO_DEFLATE;
    const int lv = pna_gpu_clamp_level(algo, level);
    const uint32_t cf = c->call_flags;
    const bool strong = (cf & F_STRONG) && (cf & F_ADOPT);
    LzSet s;
    s.bits = cf & INIT_TO_LAUNCH;
    s.gtab = zstd && lv >= 10 && strong && c->tun.strong_gtab != 0;
    s.w32 = zstd && !s.gtab && (cf & F_FAR) && (cf & F_LAZY) && c->tun.win32k != 0;
    s.w16 = s.w32 && (c->tun.win32k >= 2 || lv >= HIGH_FROM);   // the high set's geometry (round 4: chosen by the level, no longer by F_STRONG; round 5: from level 4 on -- libzstd 1.5.7's own 4 / 5 give 2.863 / 2.906 on the corpus, the default set 2.850, the high set 2.884)
    s.tab3 = s.w32 && (cf & F_INS2) && (cf & F_ADOPT) && c->tun.tab3 != 0;
    s.far1 = s.tab3 && !s.w16 && c->tun.far1 != 0;
    s.strong2 = zstd && lv >= HIGH_FROM && strong && c->tun.strong2 != 0 && (s.gtab || (s.tab3 && s.w16));
    s.lazy2 = (cf & F_LAZY) && (c->tun.lazy2 != 0 || (cf & F_STRONG));   // every lazy set defers over two positions (the high sets always did)
    s.lazy3 = s.lazy2 && c->tun.lazy2 >= 2;                              // ... and over three (option lazy2 = 2, the default)
    s.max_off = !zstd ? 32768u : (cf & F_FAR) ? (s.gtab ? MAX_OFF : MAX_OFF_W3) : NEAR_OFF;   // (3-byte words keep 19 bits of offset)
    s.max_len = !zstd ? 258u : xz ? (uint32_t)XZE_MAX_LEN : 0xFFFFFFFFu;
    return s;
}
// The flag word of a sub-batch's launches (pna_dev.h: the launch flags): the set, the codec, the short segments' geometry (SubPlan::small_fl)
static uint32_t lz_launch_flags(const LzSet &s, int algo, uint32_t small_fl) {
    const uint32_t keep = algo == PNA_ALGO_DEFLATE ? (F_LAZY | F_ADOPT | F_INS2 | F_STRONG | FLAG_STAMP | FLAG_FORCE_SERIAL) : INIT_TO_LAUNCH;
    return (s.bits & keep) | (s.w32 ? (s.w16 ? FLAG_W16 : FLAG_W32) : 0u) | (s.lazy2 ? FLAG_LAZY2 : 0u) | (s.lazy3 ? FLAG_LAZY3 : 0u) | (s.gtab ? 0u : FLAG_LEN36) |
           (s.tab3 ? FLAG_TAB3 : 0u) | (s.far1 ? FLAG_FAR1 : 0u) | (s.strong2 ? FLAG_STRONG2 : 0u) | small_fl;
}

// What every run of a sub-batch shares: the context, the plan's host tables, the launch descriptor as lz_run built it (no form, no segments yet)
struct LzStage { pna_gpu_ctx *c; const SegDesc *segs; uint32_t nseg, nblk; LzLaunch L; uint32_t *hist; bool timed; };
static uint32_t blk_base_of(const LzStage &S, uint32_t s) { return s < S.nseg ? S.segs[s].blk_base : S.nblk; }
static void set_range(LzLaunch &L, LzForm form, const SegDesc *d_segs, uint32_t nseg) { L.form = form; L.segs = d_segs; L.nseg = nseg; }

// The end of a run of segments from `a` on: the first segment before s1 whose blocks no longer fit `run_blocks` blocks from a's first one (block bases grow
// with the index: a binary search -- 10^6 small entries made the linear walk a millisecond)
static uint32_t run_end(const LzStage &S, uint32_t a, uint32_t s1, uint32_t bps, uint32_t run_blocks) {
    uint32_t b = a + 1, hi = s1;
    while (b < hi) { const uint32_t mid = b + (hi - b) / 2; if (blk_base_of(S, mid) - S.segs[a].blk_base + bps <= run_blocks) b = mid + 1; else hi = mid; }
    return b;
}
// option lz_split_blocks counts blocks of 128 KiB: a run is that many BYTES of input whatever the batch's block size
static uint32_t option_run_blocks(const LzStage &S) { return (uint32_t)std::min<uint64_t>((uint64_t)S.c->tun.lz_split_blocks << (PNA_BLK_LOG - S.segs[0].blk_log), 1u << 30); }
// The SHORT segments among [s0, s1) behind a launch of the one-kernel form, which skips them (pna_dev.h SMALL_SEG): k_lzms + the parse kernel over their blocks, through
// the words workspace, in runs of blocks as the split form's
static int lz_small_pass(const LzStage &S, uint32_t s0, uint32_t s1) {
    pna_gpu_ctx *c = S.c;
    uint32_t run_blocks = option_run_blocks(S);
    const uint32_t bps = 1u << (20 - S.segs[s0].blk_log);
    for (uint32_t a = s0; a < s1;) {
        const uint32_t b = run_end(S, a, s1, bps, run_blocks), b0 = S.segs[a].blk_base, b1 = blk_base_of(S, b);
        if (c->pbuf.ensure(((size_t)std::max<uint32_t>(b1 - b0, 1) << S.segs[a].blk_log) * 4)) {
            (void)hipGetLastError();
            if (run_blocks > 1024 && b - a > 1) { run_blocks /= 2; continue; }
            return fail(c, PNA_E_NOMEM, "no room for the short segments' words");
        }
        LzLaunch L = S.L;
        set_range(L, LzForm::Small, c->d_segs + a, b - a);
        L.pbuf = (uint32_t *)c->pbuf.p; L.blk0 = b0; L.pg.nb = b1 - b0;
        launch_lz_small(L, (L.flags & FLAG_LEN36) != 0);
        a = b;
    }
    return PNA_OK;
}

// ---- whole segments: lz_stage and its steps
// The form of a sub-batch's runs.  Split at every size: its parse kernel runs one wave per BLOCK (a block's parse depends on nothing outside the block), so a short run
// does not wait for one wave's walk over a whole segment (N x 1 MiB, one-kernel / split: 32: 2.3 / 1.6 ms, 256: 2.4 / 1.8, 1 024: 9.3 / 6.3, 2 048: 18.6 / 12.3;
// scripts/lz_forms.py).  The one-kernel form remains for PNA_F_LZ_FUSED / lz_split = 0, the phase stamps (which live in that kernel), runs shorter than lz_split_min, a
// workspace that cannot be had and the units of the latency mode; PNA_F_LZ_WAVEPARSE / lz_split = 2: the split form with k_lz's halves (testing).
//   gt (zstd 10 .. 22): the match kernel's hash tables lie in global memory (2^19 slots per segment instead of what LDS holds) -- only k_lzm has that form, so these levels
//     always take the split form with k_lzp, whatever the run's length
//   mt (option mtile): only k_lzm has sub-tiles, so every run with a segment of the large geometry takes the split form, in whole segments (no tail units: their pre-warm
//     replays tiles), and a workspace that cannot be had is an error: the one-kernel form would write other bytes
struct LzChoice { bool gt, fused, waveparse; uint32_t mt, min_segs; };
static LzChoice lz_choose(const pna_gpu_ctx *c, uint32_t flags) {
    LzChoice ch;
    ch.gt = c->lz.gtab;
    ch.mt = (flags & FLAG_ALL_SMALL) ? 0u : mtile_flag(c, ch.gt);
    ch.fused = !ch.gt && !ch.mt && ((c->call_flags & PNA_F_LZ_FUSED) || c->tun.lz_split == 0 || (flags & FLAG_STAMP));
    ch.waveparse = !ch.gt && ((c->call_flags & PNA_F_LZ_WAVEPARSE) || c->tun.lz_split == 2);
    ch.min_segs = (ch.gt || ch.mt) ? 0u : (uint32_t)c->tun.lz_split_min;
    return ch;
}
// Blocks per run over [s0, s1).  Several runs: of about equal size (whole rounds of one segment per CU) instead of full ones and a short tail -- a tail under
// lz_split_min would fall back to the slower one-kernel form (5 000 segments: 2 560 + 2 440 instead of 4 096 + 904)
static uint32_t lz_run_blocks(const LzStage &S, uint32_t s0, uint32_t s1, uint32_t bps) {
    const uint32_t limit = option_run_blocks(S), total = blk_base_of(S, s1) - S.segs[s0].blk_base, nruns = (total + limit - 1) / limit;
    if (nruns <= 1) return limit;
    const uint32_t round = S.c->n_cus * bps, even = ((total + nruns - 1) / nruns + round - 1) / round * round;
    return std::min(even, limit);
}
// The workspace of the run [a, b): a word of four bytes per position of its blocks (one run at a time on the stream, so runs share it) and, gt, its hash tables
static bool lz_workspace(pna_gpu_ctx *c, bool gt, const SegDesc &first, uint32_t nsegs, uint32_t nblocks) {
    if ((c->tun.lz_pbuf_fail && !gt) /* testing: as if the allocation failed */ || c->pbuf.ensure(((size_t)std::max<uint32_t>(nblocks, 1) << first.blk_log) * 4) ||
        (gt && c->gtab.ensure((size_t)nsegs << (lz_gtab_log() + 2)))) {
        (void)hipGetLastError();                                   // (the failed allocation's sticky code)
        return false;
    }
    return true;
}
// Timed calls: a pair of events around the run's match kernels; the first is recorded here, the second goes to the launch
static int lz_match_events(pna_gpu_ctx *c, hipStream_t st, hipEvent_t &after) {
    while (c->lzm_ev.size() < c->lzm_used + 2) { hipEvent_t e = nullptr; HIPCHK(c, hipEventCreate(&e)); c->lzm_ev.push_back(e); }
    HIPCHK(c, hipEventRecord(c->lzm_ev[c->lzm_used], st)); after = c->lzm_ev[c->lzm_used + 1]; c->lzm_used += 2; c->lzm_nl.push_back(1);
    return PNA_OK;
}
// The match kernel runs one workgroup per segment and CU, all of equal length: a run of 3 334 segments is 13 full rounds of the 256 CUs and a 14th for
// 6 of them.  The R segments behind the last full round are therefore cut into UNITS of one block each (table pre-warmed: the same words, SS4a), a launch
// of their own behind the full rounds: R x 8 short workgroups instead of R long ones next to 256 - R idle CUs.  Returns the units (0: the run goes whole),
// staged at `hu` for the copy to `du`.
static size_t lz_tail_units(const LzStage &S, const LzChoice &ch, uint32_t a, uint32_t b, uint32_t &R, SegDesc *&hu, SegDesc *&du) {
    pna_gpu_ctx *c = S.c; const SegDesc *segs = S.segs;
    R = (!ch.gt && !ch.mt && !ch.waveparse && c->tun.tail_units && b - a >= 2 * c->n_cus) ? (b - a) % c->n_cus : 0;     // (n_cus: the device's compute units, 256 on an MI355X)
    if (R > 3 * c->n_cus / 8 || (S.L.flags & FLAG_ALL_SMALL)) R = 0;
    if (!R) return 0;
    const uint32_t bl = segs[a].blk_log, bs = 1u << bl;
    size_t nu = 0;
    for (uint32_t sgi = b - R; sgi < b; sgi++) nu += std::max<uint32_t>(1, (segs[sgi].len + bs - 1) >> bl);
    constexpr size_t TAIL_CAP = 16 * 96 * 128;                 // (allocated once at this size: a buffer that grew would move under the launches already queued)
    if (c->tail_used + nu > TAIL_CAP || c->h_tail.ensure(TAIL_CAP * sizeof(SegDesc)) || c->d_tail.ensure(TAIL_CAP * sizeof(SegDesc))) return 0;
    hu = (SegDesc *)c->h_tail.p + c->tail_used; du = (SegDesc *)c->d_tail.p + c->tail_used;
    size_t k = 0;
    for (uint32_t sgi = b - R; sgi < b; sgi++)
        for (uint32_t u = 0; u < std::max<uint32_t>(segs[sgi].len, 1); u += bs) { SegDesc us = segs[sgi]; us.u0 = u; us.u1 = std::min<uint32_t>(segs[sgi].len, u + bs); hu[k++] = us; }
    c->tail_used += nu;
    return nu;
}
// One run [a, b) in the split form, its workspace at hand: the events, then the launch -- or, with tail units, the full rounds' match kernel and the units' launch
// with the parse kernel over the whole run
static int lz_split_run(const LzStage &S, const LzChoice &ch, uint32_t a, uint32_t b) {
    pna_gpu_ctx *c = S.c;
    LzLaunch L = S.L;
    L.pbuf = (uint32_t *)c->pbuf.p; L.gtab = ch.gt ? (uint32_t *)c->gtab.p : nullptr; L.blk0 = S.segs[a].blk_base;
    L.pg.nb = blk_base_of(S, b) - L.blk0; L.pg.hist = S.hist;         // the parse kernel: one wave per block of the run; (the sequence codes' counters, where the entropy stage takes them from the parse kernel)
    if (S.timed) { const int rc = lz_match_events(c, L.st, L.ev_match); if (rc) return rc; }
    if (ch.waveparse) c->lzp_hist_all = false;
    uint32_t R = 0; SegDesc *hu = nullptr, *du = nullptr;
    const size_t nu = lz_tail_units(S, ch, a, b, R, hu, du);
    if (nu) {
        HIPCHK(c, hipMemcpyAsync(du, hu, nu * sizeof(SegDesc), hipMemcpyHostToDevice, L.st));
        LzLaunch M = L; M.ev_match = nullptr;
        set_range(M, LzForm::MatchOnly, c->d_segs + a, b - a - R);
        launch_lz(M);                                                  // the full rounds: match kernel only
        set_range(L, LzForm::Split, du, (uint32_t)nu);
        launch_lz(L);                                                  // the rest in units, then the parse kernel over the whole run
        if (S.timed) c->lzm_nl.back() = 2;                             // (the pair of events spans both launches of the match kernel)
        return PNA_OK;
    }
    if (ch.waveparse) L.flags |= FLAG_SPLIT_WAVEPARSE;
    set_range(L, ch.waveparse ? LzForm::SplitWaveParse : LzForm::Split, c->d_segs + a, b - a);
    launch_lz(L);
    return PNA_OK;
}
// Segments [s0, s1) through the one-kernel form, the short ones (which it skips) through their own pass behind it
static int lz_one_kernel(const LzStage &S, uint32_t s0, uint32_t s1) {
    S.c->lzp_hist_all = false;                                         // (the one-kernel form: its parse counts nothing)
    LzLaunch L = S.L;
    set_range(L, LzForm::OneKernel, S.c->d_segs + s0, s1 - s0);
    if (!(L.flags & FLAG_ALL_SMALL)) launch_lz(L);
    return (L.flags & FLAG_HAS_SMALL) ? lz_small_pass(S, s0, s1) : PNA_OK;
}
// The LZ stage over all segments of a sub-batch.  Each pass of the outer loop takes a stretch of runs in the split form and ends in a one-kernel launch: over a run
// shorter than lz_split_min (the runs behind it are sized anew: only with tiny lz_split_blocks), or over everything left when the words workspace cannot be had --
// the run is halved down to 1 024 blocks first, for this stretch only: the next call tries the full run again
static int lz_stage(LzStage &S) {
    pna_gpu_ctx *c = S.c;
    const LzChoice ch = lz_choose(c, S.L.flags);
    S.L.flags |= ch.mt;
    const uint32_t s1 = S.nseg, bps = 1u << (20 - S.segs[0].blk_log);          // bps: blocks of a full segment
    for (uint32_t s0 = 0; s0 < s1;) {
        uint32_t run_blocks = lz_run_blocks(S, s0, s1, bps), a = s0, one_end = s1;   // [a, one_end): what is left to the one-kernel form
        while (a < s1 && !ch.fused) {
            const uint32_t b = run_end(S, a, s1, bps, run_blocks);
            if (b - a < ch.min_segs && !ch.waveparse) { one_end = b; break; }
            if (!lz_workspace(c, ch.gt, S.segs[a], b - a, blk_base_of(S, b) - S.segs[a].blk_base)) {
                if (run_blocks > 1024 && b - a > 1) { run_blocks /= 2; continue; }
                if (ch.gt) return fail(c, PNA_E_NOMEM, "no room for the strong level set's hash tables");    // (the one-kernel form has LDS tables: other bytes)
                if (ch.mt) return fail(c, PNA_E_NOMEM, "mtile: no room for the words workspace (the one-kernel form has no sub-tiles)");
                break;
            }
            const int rc = lz_split_run(S, ch, a, b); if (rc) return rc;
            a = b;
        }
        if (a >= s1) break;
        const int rc = lz_one_kernel(S, a, one_end); if (rc) return rc;
        s0 = one_end;
    }
    return PNA_OK;
}

// The LZ stage of one sub-batch, every codec: sequences, literals and block records of all its blocks in c->seqs / lits / blk
int lz_run(pna_gpu_ctx *c, int algo, const uint8_t *d_src, const SubPlan &p, hipStream_t st, bool timed) {
    c->lzm_used = 0; c->lzm_nl.clear(); c->lzp_hist_all = false;
    const bool defl = algo == PNA_ALGO_DEFLATE;
    if (defl && c->call_stored) return PNA_OK;                 // deflate level 0 = Compression::none(): stored blocks only, no match finder, no codes
    LzStage S{c, p.segs, p.nseg, p.nblk, LzLaunch{}, nullptr, timed};
    LzLaunch &L = S.L;
    L.src = d_src; L.seqs = (uint64_t *)c->seqs.p; L.lits = (uint8_t *)c->lits.p; L.blk = (BlkInfo *)c->blk.p; L.ctab = defl ? (uint4 *)c->ctab.p : nullptr;
    L.flags = lz_launch_flags(c->lz, algo, p.small_fl); L.max_off = c->lz.max_off; L.max_len = c->lz.max_len; L.st = st;
    L.pg = LzParseGrid{c->d_segs, c->d_blk_seg, 0};
    if (!p.unit_mode) {
        S.hist = (!defl && p.seq_hist) ? c->d_hist : nullptr; c->lzp_hist_all = S.hist != nullptr;
        return lz_stage(S);
    }
    // latency mode: one launch over all units (the max set: split form over the units, tables in global memory -- it takes the short segments itself)
    LzLaunch U = L;
    set_range(U, LzForm::OneKernel, c->d_units, p.nunits);
    if (c->lz.gtab) {
        if (c->pbuf.ensure(((size_t)p.nblk << p.blk_log) * 4) || c->gtab.ensure((size_t)p.nunits << (lz_gtab_log() + 2))) return fail(c, PNA_E_NOMEM, "no room for the strong level set's hash tables");
        U.form = LzForm::Split; U.pbuf = (uint32_t *)c->pbuf.p; U.gtab = (uint32_t *)c->gtab.p; U.pg.nb = p.nblk;
    }
    if (c->lz.gtab || !(L.flags & FLAG_ALL_SMALL)) launch_lz(U);
    return (!c->lz.gtab && (L.flags & FLAG_HAS_SMALL)) ? lz_small_pass(S, 0, p.nseg) : PNA_OK;
}
