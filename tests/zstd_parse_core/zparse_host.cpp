// zparse_host.cpp -- the zstd parse layer (csrc/zstd_parse_core.h) on the CPU: a small complete single-lane decoder.  Frames are walked, every header is
// parsed and every table is built by the core; the literals and the sequences are decoded by the plain loops below over those tables (through ZdWin with
// a bounded fetch), and the sequences are executed byte by byte into the caller's buffer.  What the core leaves to its callers is decided here as the
// device kernels decide it: a dictionary id is unsupported, a reserved bit or block type, a block above 128 KiB and sizes that contradict each other
// are corrupt.  The content checksum is no part of the parse layer: its 4 bytes are stepped over.
// Built two ways by the Makefile beside it:
//   libzparse_host.so   zparse_host_decode() for tests/test_zstd_parse_core.py (ctypes), plain g++;
//   zparse_host_san     the same code with the main() below under -fsanitize=address,undefined: a stand-alone program that decodes every stream of a
//                       manifest ("<stream file> <expected bytes file | -> <capacity>" per line, "-": the stream must be refused) from and into
//                       buffers of exactly those sizes -- damaged streams included.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include "../../portable-network-archive_amd/csrc/zstd_parse_core.h"

// the census: how often the decoder took each branch of the headers
#define ZC_LIST(X) \
    X(frame) X(skippable) X(fcs_0_bytes) X(fcs_1_byte) X(fcs_2_bytes) X(fcs_4_bytes) X(fcs_8_bytes) X(checksum) X(no_checksum) X(window_byte) X(single_segment) \
    X(block_raw) X(block_rle) X(block_compressed) X(lit_raw) X(lit_rle) X(lit_huffman) X(lit_treeless) \
    X(lit_header_1_byte) X(lit_header_2_bytes) X(lit_header_3_bytes_raw) X(lit_header_3_bytes) X(lit_header_4_bytes) X(lit_header_5_bytes) \
    X(huf_1_stream) X(huf_4_streams) X(weights_direct) X(weights_fse) X(nseq_zero) X(nseq_1_byte) X(nseq_2_bytes) X(nseq_3_bytes) \
    X(ll_predefined) X(ll_rle) X(ll_fse) X(ll_repeat) X(of_predefined) X(of_rle) X(of_fse) X(of_repeat) X(ml_predefined) X(ml_rle) X(ml_fse) X(ml_repeat)
#define X(n) ZC_##n,
enum { ZC_LIST(X) ZC_N };
#undef X
#define X(n) #n ","
extern "C" const char *zparse_host_census_names(void) { return ZC_LIST(X); }
#undef X
extern "C" int zparse_host_census_size(void) { return ZC_N; }

namespace {

struct Frame {                                 // what a frame's blocks hand on
    uint16_t huf[1 << ZD_HUF_MAX]; uint32_t hufbits; bool huf_ok;
    uint32_t fse[3][512], alog[3]; bool ok[3];
    uint32_t rep[3];
};
struct Out { uint8_t *dst; uint64_t cap, op, frame_start; };

// word j of the bit string g[0 .. n): bytes behind its end read as zero
struct Fetch {
    const uint8_t *g; uint32_t n;
    uint64_t operator()(int64_t j) const {
        uint64_t v = 0;
        for (uint32_t i = 0; i < 8; i++) { const uint64_t at = 8 * (uint64_t)j + i; if (at < n) v |= (uint64_t)g[at] << (8 * i); }
        return v;
    }
};

int decode_block(Frame &F, const uint8_t *p, uint32_t len, Out &o, uint64_t *cen) {
    uint8_t weights[256]; int16_t norm[256]; uint16_t nexts[256]; uint32_t wtab[64];
    // ---- literals
    ZdLitHdr l;
    if (!zd_literals_header(p, len, l) || l.regen > ZD_BLOCK_MAX || l.size > len) return ZD_CORRUPT;
    cen[ZC_lit_raw + l.ltype]++;
    if (l.ltype < 2) cen[l.hdr == 1 ? ZC_lit_header_1_byte : (l.hdr == 2 ? ZC_lit_header_2_bytes : ZC_lit_header_3_bytes_raw)]++;
    else cen[l.hdr == 3 ? ZC_lit_header_3_bytes : (l.hdr == 4 ? ZC_lit_header_4_bytes : ZC_lit_header_5_bytes)]++;
    std::vector<uint8_t> lit(l.regen);
    if (l.ltype == 0) { if (l.regen) memcpy(lit.data(), p + l.hdr, l.regen); }
    else if (l.ltype == 1) { if (l.regen) memset(lit.data(), p[l.hdr], l.regen); }
    else {
        const uint8_t *cs = p + l.hdr;
        uint32_t used = 0;
        if (l.ltype == 2) {
            uint32_t n = 0, maxbits = 0;
            if (!zd_huf_weights(cs, l.comp, weights, norm, nexts, wtab, n, maxbits, used)) return ZD_CORRUPT;
            cen[cs[0] >= 128 ? ZC_weights_direct : ZC_weights_fse]++;
            zd_huf_fill(F.huf, weights, n, maxbits, 0, 1);
            F.hufbits = maxbits; F.huf_ok = true;
        } else if (!F.huf_ok) return ZD_CORRUPT;
        if (used > l.comp) return ZD_CORRUPT;
        cen[l.streams == 4 ? ZC_huf_4_streams : ZC_huf_1_stream]++;
        for (uint32_t q = 0; q < l.streams; q++) {
            ZdStream s;
            if (!zd_huf_streams(cs + used, l.comp - used, l.regen, l.streams, q, s)) return ZD_CORRUPT;
            const Fetch fetch = {cs + used + s.off, s.len};
            ZdWin w;
            if (!zd_winit(w, fetch, s.len ? fetch.g[s.len - 1] : 0u, s.len)) return ZD_CORRUPT;
            for (uint32_t i = 0; i < s.out_len; i++) {
                const uint32_t cell = F.huf[(uint32_t)zd_wpeek(w, fetch, F.hufbits)];
                lit[s.out_off + i] = (uint8_t)cell;
                w.off -= cell >> 8;
                if (w.off < 0) return ZD_CORRUPT;
            }
            if (w.off != 0) return ZD_CORRUPT;
        }
    }
    // ---- sequences
    uint32_t pos = l.size, nseq, modes, litpos = 0;
    const uint32_t at = pos;
    if (!zd_seq_header(p, len, pos, nseq, modes)) return ZD_CORRUPT;
    const uint32_t count_bytes = pos - at - (nseq ? 1 : 0);
    cen[nseq == 0 ? ZC_nseq_zero : (count_bytes == 1 ? ZC_nseq_1_byte : (count_bytes == 2 ? ZC_nseq_2_bytes : ZC_nseq_3_bytes))]++;
    if (nseq) {
        if (modes & 3) return ZD_CORRUPT;
        for (int k = 0; k < 3; k++) {
            const uint32_t mode = zd_seq_mode(modes, k);
            cen[ZC_ll_predefined + 4 * k + mode]++;
            if (mode == 3) { if (!F.ok[k]) return ZD_CORRUPT; }
            else if (!zd_seq_table(k, mode, p, len, pos, F.fse[k], norm, nexts, F.alog[k])) return ZD_CORRUPT;
            F.ok[k] = true;
        }
        if (pos >= len) return ZD_CORRUPT;
        const Fetch fq = {p + pos, len - pos};
        ZdWin w;
        if (!zd_winit(w, fq, fq.g[fq.n - 1], fq.n)) return ZD_CORRUPT;
        uint32_t sll = (uint32_t)zd_wread(w, fq, F.alog[0]), sof = (uint32_t)zd_wread(w, fq, F.alog[1]), sml = (uint32_t)zd_wread(w, fq, F.alog[2]);
        for (uint32_t i = 0; i < nseq; i++) {
            const uint32_t cl = F.fse[0][sll], co = F.fse[1][sof], cm = F.fse[2][sml];
            const uint32_t llc = cl & 0xFF, ofc = co & 0xFF, mlc = cm & 0xFF;
            if (ofc > 31 || mlc > 52 || llc > 35) return ZD_CORRUPT;
            const uint64_t ofv = ((uint64_t)1 << ofc) + zd_wread(w, fq, ofc);
            const uint32_t ml = ZD_ML_BASE[mlc] + (uint32_t)zd_wread(w, fq, ZD_ML_BITS[mlc]);
            const uint32_t ll = ZD_LL_BASE[llc] + (uint32_t)zd_wread(w, fq, ZD_LL_BITS[llc]);
            if (w.off < 0) return ZD_CORRUPT;
            if (i + 1 < nseq) {
                sll = (cl >> 16) + (uint32_t)zd_wread(w, fq, (cl >> 8) & 0xFF);
                sml = (cm >> 16) + (uint32_t)zd_wread(w, fq, (cm >> 8) & 0xFF);
                sof = (co >> 16) + (uint32_t)zd_wread(w, fq, (co >> 8) & 0xFF);
                if (w.off < 0) return ZD_CORRUPT;
            }
            uint64_t offset;
            if (ofv > 3) { offset = ofv - 3; F.rep[2] = F.rep[1]; F.rep[1] = F.rep[0]; F.rep[0] = (uint32_t)offset; }
            else {
                const uint32_t idx = (uint32_t)ofv - 1 + (ll == 0 ? 1u : 0u);
                if (idx == 0) offset = F.rep[0];
                else {
                    offset = idx == 1 ? F.rep[1] : (idx == 2 ? F.rep[2] : F.rep[0] - 1);
                    if (offset == 0) return ZD_CORRUPT;
                    if (idx > 1) F.rep[2] = F.rep[1];
                    F.rep[1] = F.rep[0]; F.rep[0] = (uint32_t)offset;
                }
            }
            if (litpos + ll > l.regen) return ZD_CORRUPT;
            if (o.op + ll + ml > o.cap) return ZD_DSTSIZE;
            if (offset > o.op + ll - o.frame_start) return ZD_CORRUPT;
            for (uint32_t k = 0; k < ll; k++) o.dst[o.op++] = lit[litpos++];
            for (uint32_t k = 0; k < ml; k++, o.op++) o.dst[o.op] = o.dst[o.op - offset];
        }
        if (w.off != 0) return ZD_CORRUPT;
    } else if (pos != len) return ZD_CORRUPT;
    const uint32_t rest = l.regen - litpos;
    if (o.op + rest > o.cap) return ZD_DSTSIZE;
    for (uint32_t k = 0; k < rest; k++) o.dst[o.op++] = lit[litpos++];
    return ZD_OK;
}

} // namespace

// every frame of src[0 .. n) into dst[0 .. cap): 0 decoded (*out_len bytes), else ZD_CORRUPT / ZD_UNSUPPORTED / ZD_DSTSIZE; census[ZC_N] is added to
extern "C" int zparse_host_decode(const uint8_t *src, size_t n, uint8_t *dst, size_t cap, size_t *out_len, uint64_t *census) {
    uint64_t none[ZC_N] = {0};
    uint64_t *cen = census ? census : none;
    Out o = {dst, cap, 0, 0};
    uint64_t ip = 0;
    while (ip < n) {
        uint64_t skip = 0;
        const int sk = zd_skippable(src + ip, n - ip, &skip);
        if (sk == ZD_SKIP_WHOLE) { cen[ZC_skippable]++; ip += skip; continue; }
        ZdFrameHdr h;
        zd_frame_header(src + ip, n - ip, h);
        if (sk || !h.have || !h.magic || h.reserved) return ZD_CORRUPT;
        if (h.dict_bytes) return ZD_UNSUPPORTED;
        if (!h.complete) return ZD_CORRUPT;
        cen[ZC_frame]++; cen[h.checksum ? ZC_checksum : ZC_no_checksum]++; cen[h.single ? ZC_single_segment : ZC_window_byte]++;
        cen[h.fcs_bytes == 0 ? ZC_fcs_0_bytes : (h.fcs_bytes == 1 ? ZC_fcs_1_byte : (h.fcs_bytes == 2 ? ZC_fcs_2_bytes : (h.fcs_bytes == 4 ? ZC_fcs_4_bytes : ZC_fcs_8_bytes)))]++;
        std::vector<Frame> fv(1);
        Frame &F = fv[0];
        F.huf_ok = false; F.ok[0] = F.ok[1] = F.ok[2] = false; F.rep[0] = 1; F.rep[1] = 4; F.rep[2] = 8;
        o.frame_start = o.op;
        uint64_t q = ip + h.len;
        for (;;) {
            ZdBlockHdr b;
            zd_block_header(src + q, n - q, b);
            if (!b.have || b.type == 3 || b.size > ZD_BLOCK_MAX || !b.fits) return ZD_CORRUPT;
            cen[ZC_block_raw + b.type]++;
            const uint8_t *body = src + q + 3;
            if (b.type < 2) {
                if (o.op + b.size > o.cap) return ZD_DSTSIZE;
                for (uint32_t i = 0; i < b.size; i++) o.dst[o.op++] = b.type == 0 ? body[i] : body[0];
            } else {
                std::vector<uint8_t> blk(body, body + b.size);             // (an exact-size copy: a read outside the block is the sanitizer's to find)
                const int st = decode_block(F, blk.data(), b.size, o, cen);
                if (st) return st;
            }
            q += 3 + b.body;
            if (b.last) break;
        }
        if (h.checksum) { if (n - q < 4) return ZD_CORRUPT; q += 4; }
        if (h.fcs_bytes && o.op - o.frame_start != h.fcs) return ZD_CORRUPT;
        ip = q;
    }
    *out_len = (size_t)o.op;
    return ZD_OK;
}

#ifdef ZPARSE_HOST_MAIN
static bool slurp(const std::string &path, std::vector<uint8_t> &out) {
    FILE *f = fopen(path.c_str(), "rb");
    if (!f) return false;
    out.clear();
    uint8_t buf[65536];
    size_t k;
    while ((k = fread(buf, 1, sizeof buf, f)) > 0) out.insert(out.end(), buf, buf + k);
    fclose(f);
    return true;
}
int main(int argc, char **argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s MANIFEST\n", argv[0]); return 2; }
    FILE *m = fopen(argv[1], "r");
    if (!m) { perror(argv[1]); return 2; }
    char a[1024], b[1024];
    unsigned long long cap;
    int bad = 0, n = 0;
    while (fscanf(m, "%1023s %1023s %llu", a, b, &cap) == 3) {
        std::vector<uint8_t> src, want;
        const bool refuse = strcmp(b, "-") == 0;
        if (!slurp(a, src) || (!refuse && !slurp(b, want))) { fprintf(stderr, "cannot read %s / %s\n", a, b); return 2; }
        std::vector<uint8_t> out((size_t)cap);
        size_t got = 0;
        const int st = zparse_host_decode(src.data(), src.size(), out.data(), out.size(), &got, nullptr);
        const bool ok = refuse ? st != 0 : (st == 0 && got == want.size() && (got == 0 || memcmp(out.data(), want.data(), got) == 0));
        if (!ok) { fprintf(stderr, "FAIL %s: status %d, %zu bytes (expected %s)\n", a, st, got, refuse ? "a refusal" : "the recorded bytes"); bad++; }
        n++;
    }
    fclose(m);
    printf("%d streams, %d failures\n", n, bad);
    return bad ? 1 : 0;
}
#endif
