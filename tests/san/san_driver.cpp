// tests/san/san_driver.cpp -- TEST INFRASTRUCTURE: drives the C ABI of libpna_gpu.so's HOST code (built against the CPU HIP shim and the
// device stub) under AddressSanitizer / UBSan / ThreadSanitizer: the container writer, sanitize, split / join, the password hashes, the
// batch call, the CompressionWriter facade from many threads (group commit, page-locked slab pool), the bounded host pipeline with its
// stager thread, the streaming entry writer, append.  Exit code 0 = every check passed and the sanitizer stayed silent.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <atomic>
#include <functional>
#include <string>
#include <thread>
#include <vector>
#include "../../include/pna_gpu.h"
#include "../../include/pna_archive.h"

static int g_fail = 0;
#define CHECK(c) do { if (!(c)) { fprintf(stderr, "CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #c); g_fail++; } } while (0)

typedef std::vector<uint8_t> Bytes;
static int vec_sink(void *u, const void *b, size_t n) { Bytes *v = (Bytes *)u; v->insert(v->end(), (const uint8_t *)b, (const uint8_t *)b + n); return 0; }

static Bytes text(size_t n, uint32_t seed) {                     // compressible-looking filler (the stub stores it anyway)
    Bytes v(n); uint32_t s = seed * 2654435761u + 1;
    for (size_t i = 0; i < n; i++) { s = s * 1664525u + 1013904223u; v[i] = (uint8_t)("etaoin shrdlu\n"[(s >> 24) % 14]); }
    return v;
}
// decoder for what the device stub writes: frames of RAW blocks (and the 9-byte empty frame)
static bool unraw(const uint8_t *p, size_t n, Bytes &out) {
    size_t pos = 0;
    while (pos < n) {
        if (n - pos < 5 || p[pos] != 0x28 || p[pos + 1] != 0xB5 || p[pos + 2] != 0x2F || p[pos + 3] != 0xFD) return false;
        pos += 4;
        if (p[pos] == 0x20) pos += 2; else if (p[pos] == 0x00) pos += 2; else return false;
        for (;;) {
            if (n - pos < 3) return false;
            const uint32_t h = p[pos] | (p[pos + 1] << 8) | (p[pos + 2] << 16); pos += 3;
            const uint32_t ty = (h >> 1) & 3, sz = h >> 3;
            if (ty != 0 || n - pos < sz) return false;
            out.insert(out.end(), p + pos, p + pos + sz); pos += sz;
            if (h & 1) break;
        }
    }
    return true;
}
struct Chunk { char ty[5]; size_t off, len; };
static bool walk(const Bytes &a, std::vector<Chunk> &out) {      // every chunk's CRC is checked
    if (a.size() < 8) return false;
    size_t pos = 8;
    while (pos < a.size()) {
        if (a.size() - pos < 12) return false;
        const size_t l = ((size_t)a[pos] << 24) | (a[pos + 1] << 16) | (a[pos + 2] << 8) | a[pos + 3];
        if (a.size() - pos - 12 < l) return false;
        Chunk c; memcpy(c.ty, &a[pos + 4], 4); c.ty[4] = 0; c.off = pos + 8; c.len = l;
        const uint32_t crc = pna_crc32(0, &a[pos + 4], 4 + l);
        const uint32_t st = ((uint32_t)a[pos + 8 + l] << 24) | (a[pos + 9 + l] << 16) | (a[pos + 10 + l] << 8) | a[pos + 11 + l];
        if (crc != st) return false;
        out.push_back(c); pos += 12 + l;
    }
    return true;
}
// entries of an archive image: (name, decoded data) for FHED .. FEND records written by the (stubbed) zstd path
static bool read_back(const Bytes &arc, std::vector<std::pair<std::string, Bytes>> &ents) {
    std::vector<Chunk> ch; if (!walk(arc, ch)) return false;
    std::string name; Bytes pay; bool open = false;
    for (const Chunk &c : ch) {
        if (!strcmp(c.ty, "FHED")) { name.assign((const char *)&arc[c.off + 6], c.len - 6); pay.clear(); open = true; }
        else if (!strcmp(c.ty, "FDAT") && open) pay.insert(pay.end(), arc.begin() + c.off, arc.begin() + c.off + c.len);
        else if (!strcmp(c.ty, "FEND") && open) { Bytes d; if (!unraw(pay.data(), pay.size(), d)) return false; ents.emplace_back(name, d); open = false; }
    }
    return !open;
}

static void test_container() {
    Bytes out; pna_archive *a = nullptr;
    CHECK(pna_archive_new(vec_sink, &out, 0, &a) == PNA_OK);
    const Bytes p1 = text(100000, 1);
    CHECK(pna_archive_add_file(a, "dir/../a.txt", 0, (int64_t)p1.size(), p1.data(), p1.size(), 30000) == PNA_OK);
    CHECK(pna_archive_add_dir(a, "/some/dir/") == PNA_OK);
    const void *pcs[2] = {p1.data(), p1.data() + 5}; const size_t pl[2] = {5, 7};
    CHECK(pna_archive_add_solid(a, 0, pcs, pl, 2) == PNA_OK);
    CHECK(pna_archive_finalize(a) == PNA_OK);
    std::vector<Chunk> ch; CHECK(walk(out, ch));
    std::string kinds; for (auto &c : ch) { kinds += c.ty; kinds += ' '; }
    CHECK(kinds == "AHED FHED fSIZ FDAT FDAT FDAT FDAT FEND FHED FEND SHED SDAT SDAT SEND AEND ");
    CHECK(std::string((const char *)&out[ch[1].off + 6], ch[1].len - 6) == "a.txt");
    CHECK(std::string((const char *)&out[ch[8].off + 6], ch[8].len - 6) == "some/dir");
    // sanitize: the reference's vectors through the inner-record writer
    const char *vec[][2] = {{"/var/../tmp/./log", "tmp/log"}, {"test/../test.txt", "test.txt"}, {"../../..", ""}, {"a/b/./../a.txt", "a/a.txt"}, {"x\\y", "x\\y"}, {"", ""}};
    for (auto &v : vec) {
        uint8_t buf[256]; const size_t n = pna_archive_inner_entry_bytes(v[0], "d", 1, buf, sizeof buf);
        CHECK(n > 20 && std::string((const char *)buf + 14, (((size_t)buf[2] << 8) | buf[3]) - 6) == v[1]);
    }
    // seek_to_end / list_entries / split / join
    uint64_t at = 0; int nxt = 0;
    CHECK(pna_archive_seek_to_end(out.data(), out.size(), &at, &nxt) == PNA_OK && at == out.size() - 12 && nxt == 0);
    for (size_t cut = 1; cut <= 8; cut++) CHECK(pna_archive_seek_to_end(out.data(), out.size() - cut, &at, &nxt) == PNA_E_INVAL);
    std::vector<std::string> names;
    auto lcb = [](void *u, size_t, const char *nm, size_t nl, int, uint64_t, uint64_t) -> int { ((std::vector<std::string> *)u)->emplace_back(nm, nl); return 0; };
    CHECK(pna_archive_list_entries(out.data(), out.size(), lcb, &names) == PNA_OK && names.size() == 3 && names[0] == "a.txt" && names[2].empty());
    std::vector<Bytes> parts;
    auto psink = [](void *u, uint32_t idx, const void *b, size_t n) -> int { auto *v = (std::vector<Bytes> *)u; if (v->size() <= idx) v->resize(idx + 1); (*v)[idx].insert((*v)[idx].end(), (const uint8_t *)b, (const uint8_t *)b + n); return 0; };
    uint32_t np = 0;
    CHECK(pna_split_archive(out.data(), out.size(), 20000, psink, &parts, &np) == PNA_OK && np == parts.size() && np >= 5);
    std::vector<const void *> pp; std::vector<size_t> pn; for (auto &p : parts) { pp.push_back(p.data()); pn.push_back(p.size()); CHECK(p.size() <= 20000); }
    Bytes joined; CHECK(pna_join_parts(pp.data(), pn.data(), pp.size(), vec_sink, &joined) == PNA_OK);
    std::vector<Chunk> c2; CHECK(walk(joined, c2));
    Bytes d1, d2; for (auto &c : ch) if (!strcmp(c.ty, "FDAT")) d1.insert(d1.end(), out.begin() + c.off, out.begin() + c.off + c.len);
    for (auto &c : c2) if (!strcmp(c.ty, "FDAT")) d2.insert(d2.end(), joined.begin() + c.off, joined.begin() + c.off + c.len);
    CHECK(d1 == d2 && d1 == p1);
}
static void test_kdf() {
    uint8_t key[32], key2[32]; char phsf[128];
    CHECK(pna_kdf_pbkdf2_sha256("password", 8, "saltsaltsaltsalt", 16, 100, key, 32, phsf, sizeof phsf) == PNA_OK && !strncmp(phsf, "$pbkdf2-sha256$i=100,l=32$", 26));
    CHECK(pna_kdf_argon2(2, "password", 8, "saltsaltsaltsalt", 16, 1, 64, 2, key2, 32) == PNA_OK);
    CHECK(memcmp(key, key2, 32) != 0);
}
static void test_batch(pna_gpu_ctx *c) {
    const size_t lens[] = {0, 1, 7, 4096, 100000, 131072, 131073, (1u << 20), (1u << 20) + 5, 2500000};
    const size_t n = sizeof lens / sizeof lens[0];
    std::vector<Bytes> in(n), out(n); std::vector<const void *> src(n); std::vector<void *> dst(n); std::vector<size_t> sl(n), cap(n), dl(n);
    for (size_t i = 0; i < n; i++) { in[i] = text(lens[i], (uint32_t)i); out[i].resize(pna_gpu_bound(PNA_ALGO_ZSTD, lens[i])); src[i] = in[i].data(); dst[i] = out[i].data(); sl[i] = lens[i]; cap[i] = out[i].size(); }
    CHECK(pna_gpu_compress_batch(c, PNA_ALGO_ZSTD, 3, n, src.data(), sl.data(), dst.data(), cap.data(), dl.data()) == PNA_OK);
    for (size_t i = 0; i < n; i++) { Bytes d; CHECK(unraw(out[i].data(), dl[i], d) && d == in[i]); }
    cap[3] = 10;
    CHECK(pna_gpu_compress_batch(c, PNA_ALGO_ZSTD, 3, n, src.data(), sl.data(), dst.data(), cap.data(), dl.data()) == PNA_E_DSTSIZE);
    CHECK(pna_gpu_compress_batch(c, 4, 3, n, src.data(), sl.data(), dst.data(), cap.data(), dl.data()) == PNA_E_UNSUPPORTED);
}
static void test_streams(pna_gpu_ctx *c) {
    const unsigned T = 24, per = 12;
    std::atomic<int> bad{0};
    std::vector<std::thread> th;
    for (unsigned t = 0; t < T; t++)
        th.emplace_back([&, t]() {
            for (unsigned k = 0; k < per; k++) {
                const Bytes in = text((size_t)((t * 7919u + k * 104729u) % 700000u), t * 100 + k);
                Bytes out; pna_gpu_stream *s = nullptr;
                if (pna_gpu_stream_new(c, PNA_ALGO_ZSTD, 3, vec_sink, &out, &s) != PNA_OK) { bad++; continue; }
                size_t pos = 0; int rc = PNA_OK;
                while (pos < in.size() && rc == PNA_OK) { const size_t w = std::min<size_t>(in.size() - pos, 1 + (pos * 31 + k) % 90000); rc = pna_gpu_stream_write(s, in.data() + pos, w); pos += w; }
                if (rc != PNA_OK) { pna_gpu_stream_abort(s); bad++; continue; }
                if (k % 5 == 4) { pna_gpu_stream_abort(s); continue; }                // a builder dropped without build()
                if (pna_gpu_stream_finish(s) != PNA_OK) { bad++; continue; }
                Bytes d; if (!unraw(out.data(), out.size(), d) || d != in) bad++;
            }
        });
    for (auto &x : th) x.join();
    CHECK(bad.load() == 0);
    uint64_t b = 0, e = 0, mx = 0;
    CHECK(pna_gpu_stream_stats(c, &b, &e, &mx) == PNA_OK && e > 0 && b <= e && mx >= 1);
}
static void test_pipeline_and_append(pna_gpu_ctx *c) {
    setenv("PNA_SUB_MIB", "16", 1);                                      // several sub-batches: the stager thread and both slots are used
    const size_t n = 150;
    std::vector<Bytes> in(n); std::vector<std::string> nm(n); std::vector<const char *> names(n); std::vector<const void *> src(n); std::vector<size_t> sl(n);
    for (size_t i = 0; i < n; i++) { in[i] = text(i % 9 == 0 ? 0 : 200000 + 1777 * i, (uint32_t)i + 1000); nm[i] = "p/" + std::to_string(i) + ".txt"; names[i] = nm[i].c_str(); src[i] = in[i].data(); sl[i] = in[i].size(); }
    Bytes whole;
    CHECK(pna_gpu_create_archive_host(c, PNA_ALGO_ZSTD, 3, n, names.data(), src.data(), sl.data(), vec_sink, &whole) == PNA_OK);
    std::vector<std::pair<std::string, Bytes>> ents;
    CHECK(read_back(whole, ents) && ents.size() == n);
    for (size_t i = 0; i < n && i < ents.size(); i++) CHECK(ents[i].first == nm[i] && ents[i].second == in[i]);
    // append: the first 100 entries, then the other 50 behind them == all at once.  (Byte equality needs the block size to be the same in both runs: the library's
    // latency mode picks it by the size of the batch an entry happens to travel in, so the mode is switched off for this comparison.)
    CHECK(pna_gpu_set_option(c, "latency_max_mib", 0) == PNA_OK);
    whole.clear();
    CHECK(pna_gpu_create_archive_host(c, PNA_ALGO_ZSTD, 3, n, names.data(), src.data(), sl.data(), vec_sink, &whole) == PNA_OK);
    Bytes base, tail; uint64_t at = 0;
    CHECK(pna_gpu_create_archive_host(c, PNA_ALGO_ZSTD, 3, 100, names.data(), src.data(), sl.data(), vec_sink, &base) == PNA_OK);
    CHECK(pna_gpu_append_archive_host(c, PNA_ALGO_ZSTD, 3, base.data(), base.size(), n - 100, names.data() + 100, src.data() + 100, sl.data() + 100, &at, vec_sink, &tail) == PNA_OK);
    Bytes got(base.begin(), base.begin() + at); got.insert(got.end(), tail.begin(), tail.end());
    CHECK(got == whole);
    // streaming entry: FHED, meta, FDAT per burst (<= max chunk), FEND, no fSIZ
    Bytes rec; pna_gpu_entry_writer *w = nullptr;
    const uint8_t meta_body[1] = {1};
    Bytes meta; { const uint8_t h[8] = {0, 0, 0, 1, 'f', 'L', 'T', 'P'}; meta.insert(meta.end(), h, h + 8); meta.push_back(1); const uint32_t crc = pna_crc32(pna_crc32(0, "fLTP", 4), meta_body, 1); const uint8_t t[4] = {(uint8_t)(crc >> 24), (uint8_t)(crc >> 16), (uint8_t)(crc >> 8), (uint8_t)crc}; meta.insert(meta.end(), t, t + 4); }
    CHECK(pna_gpu_stream_entry_begin(c, PNA_ALGO_ZSTD, 3, "./s/../streamed.txt", meta.data(), meta.size(), 5000, vec_sink, &rec, &w) == PNA_OK);
    CHECK(pna_gpu_stream_entry_write(w, in[1].data(), in[1].size()) == PNA_OK && pna_gpu_stream_entry_finish(w) == PNA_OK);
    Bytes arc; { pna_archive *a = nullptr; CHECK(pna_archive_new(vec_sink, &arc, 0, &a) == PNA_OK); arc.insert(arc.end(), rec.begin(), rec.end()); CHECK(pna_archive_finalize(a) == PNA_OK); }
    std::vector<Chunk> ch; CHECK(walk(arc, ch));
    bool has_fsiz = false; size_t nfdat = 0; for (auto &x : ch) { if (!strcmp(x.ty, "fSIZ")) has_fsiz = true; if (!strcmp(x.ty, "FDAT")) { nfdat++; CHECK(x.len <= 5000); } }
    CHECK(!has_fsiz && nfdat >= in[1].size() / 5000 && !strcmp(ch[1].ty, "FHED") && !strcmp(ch[2].ty, "fLTP"));
    ents.clear(); CHECK(read_back(arc, ents) && ents.size() == 1 && ents[0].first == "streamed.txt" && ents[0].second == in[1]);
    CHECK(pna_gpu_stream_entry_begin(c, PNA_ALGO_ZSTD, 3, "x", "garbage", 7, 0, vec_sink, &rec, &w) == PNA_E_INVAL);
}

// Framing matrix: archives of every framing form the encode core lays out -- plain, metadata, several FDAT chunks, device / host layout, part flags,
// CTR / CBC / GCM (several segments per entry, an empty entry), solid on the device and windowed from host memory -- with fixed IVs and salts.  Each one
// is walked (every chunk CRC) and its CRC-32 compared with the value recorded when the matrix was written: any change in what the host hands the
// (stubbed) kernels changes the bytes.
static Bytes chunk(const char ty[4], const Bytes &body) {
    Bytes o = {(uint8_t)(body.size() >> 24), (uint8_t)(body.size() >> 16), (uint8_t)(body.size() >> 8), (uint8_t)body.size()};
    o.insert(o.end(), ty, ty + 4); o.insert(o.end(), body.begin(), body.end());
    const uint32_t crc = pna_crc32(pna_crc32(0, ty, 4), body.data(), body.size());
    for (int s = 24; s >= 0; s -= 8) o.push_back((uint8_t)(crc >> s));
    return o;
}
static void framing_case(const char *what, const Bytes &arc, uint32_t want, const Bytes *whole = nullptr) {   // whole: a part, walked inside an archive
    std::vector<Chunk> ch;
    const bool ok = walk(whole ? *whole : arc, ch);
    const uint32_t got = pna_crc32(0, arc.data(), arc.size());
    printf("framing %-28s %8zu bytes crc %08x\n", what, arc.size(), got);
    if (!ok || got != want) { fprintf(stderr, "framing %s: %s (crc %08x, recorded %08x)\n", what, ok ? "bytes changed" : "malformed archive", got, want); g_fail++; }
}
static void test_framing_matrix() {
    pna_gpu_ctx *c = nullptr;
    CHECK(pna_gpu_init(&c, 0, PNA_F_DEFAULT) == PNA_OK);
    if (!c) return;
    // entries: empty, small, one segment, several segments (the last one short), in one 16-byte aligned device buffer
    const size_t lens[] = {0, 5000, 70000, 1 << 20, (1 << 20) + (1 << 19) + 333, 12345};
    const size_t n = sizeof lens / sizeof lens[0];
    std::vector<uint64_t> off(n), len(n); std::vector<std::string> nm(n); std::vector<const char *> names(n);
    uint64_t at = 0;
    for (size_t i = 0; i < n; i++) { off[i] = at; len[i] = lens[i]; at = (at + lens[i] + 15) & ~(uint64_t)15; nm[i] = "m/" + std::to_string(i) + ".bin"; names[i] = nm[i].c_str(); }
    Bytes src(at + 64, 0);
    for (size_t i = 0; i < n; i++) { const Bytes t = text(lens[i], 7000 + (uint32_t)i); if (!t.empty()) memcpy(&src[off[i]], t.data(), t.size()); }
    uint8_t ivs[6 * 39];
    for (size_t i = 0; i < sizeof ivs; i++) ivs[i] = (uint8_t)(i * 37 + 11);
    pna_gpu_cipher ctr = {PNA_ENC_AES, PNA_MODE_CTR, {0}, "$pbkdf2-sha256$i=100,l=32$c2FsdA$aGFzaA", ivs, 0};
    for (int i = 0; i < 32; i++) ctr.key[i] = (uint8_t)(3 * i + 1);
    pna_gpu_cipher cbc = ctr; cbc.cipher_mode = PNA_MODE_CBC;
    pna_gpu_cipher gcm = ctr; gcm.cipher_mode = PNA_MODE_GCM; gcm.gcm_segment_size = 65536;
    // metadata: an extra chunk in front of fSIZ and a facet behind it, on some entries
    const Bytes ex = chunk("tEST", Bytes{1, 2, 3}), fa = chunk("mTIM", Bytes{0, 0, 0, 0, 0x5F, 0, 0, 1});
    std::vector<const void *> exv(n, ex.data()), fav(n, fa.data()); std::vector<size_t> exl(n, 0), fal(n, 0);
    exl[1] = exl[3] = ex.size(); fal[1] = fal[2] = fal[5] = fa.size();
    const pna_gpu_entry_meta meta = {exv.data(), exl.data(), fav.data(), fal.data()};
    auto dev = [&](const char *what, const pna_gpu_cipher *ci, const pna_gpu_entry_meta *m, uint32_t mcs, uint32_t parts, uint32_t want) {
        const size_t cap = pna_gpu_archive_chunked_bound(PNA_ALGO_ZSTD, n, names.data(), len.data(), ci, mcs) + 4096;
        Bytes dst(cap + 16); uint8_t *d = dst.data() + ((16 - ((uintptr_t)dst.data() & 15)) & 15);
        std::vector<uint64_t> eoff(n + 1); uint64_t alen = 0;
        const int rc = pna_gpu_create_archive_chunked_device(c, PNA_ALGO_ZSTD, 3, n, names.data(), src.data(), off.data(), len.data(), ci, m, mcs, d, cap,
                                                             eoff.data(), &alen, parts, nullptr);
        CHECK(rc == PNA_OK && eoff[n] <= alen);
        Bytes arc(d, d + (rc == PNA_OK ? alen : 0));
        if (parts == (PNA_PART_HEAD | PNA_PART_TAIL)) { framing_case(what, arc, want); return; }
        Bytes empty; pna_archive *a = nullptr;                   // a part: walked between the head and the tail of an empty archive
        CHECK(pna_archive_new(vec_sink, &empty, 0, &a) == PNA_OK && pna_archive_finalize(a) == PNA_OK && empty.size() > 12);
        Bytes whole(empty.begin(), empty.end() - (parts & PNA_PART_HEAD ? empty.size() : 12));
        whole.insert(whole.end(), arc.begin(), arc.end());
        if (!(parts & PNA_PART_TAIL)) whole.insert(whole.end(), empty.end() - 12, empty.end());
        framing_case(what, arc, want, &whole);
    };
    for (long dl = 0; dl <= 1; dl++) {
        CHECK(pna_gpu_set_option(c, "dev_layout", dl) == PNA_OK);
        dev(dl ? "plain dev_layout=1" : "plain dev_layout=0", nullptr, nullptr, 0, PNA_PART_HEAD | PNA_PART_TAIL, 0x8aa4a34fu);
        dev(dl ? "meta dev_layout=1" : "meta dev_layout=0", nullptr, &meta, 0, PNA_PART_HEAD | PNA_PART_TAIL, 0xe08d0a72u);
        dev(dl ? "chunked dev_layout=1" : "chunked dev_layout=0", nullptr, nullptr, 300000, PNA_PART_HEAD | PNA_PART_TAIL, 0xa3b88b24u);
        dev(dl ? "part head dev_layout=1" : "part head dev_layout=0", nullptr, nullptr, 0, PNA_PART_HEAD, 0xb18d2166u);
        dev(dl ? "part tail dev_layout=1" : "part tail dev_layout=0", nullptr, nullptr, 0, PNA_PART_TAIL, 0x9037bfb1u);
    }
    dev("ctr", &ctr, nullptr, 0, PNA_PART_HEAD | PNA_PART_TAIL, 0x67bd3d58u);
    dev("ctr chunked meta", &ctr, &meta, 200000, PNA_PART_HEAD | PNA_PART_TAIL, 0x6f1409eau);
    dev("cbc", &cbc, nullptr, 0, PNA_PART_HEAD | PNA_PART_TAIL, 0xeab93cf6u);
    dev("gcm", &gcm, nullptr, 0, PNA_PART_HEAD | PNA_PART_TAIL, 0x0cd7fb94u);
    dev("gcm meta", &gcm, &meta, 0, PNA_PART_HEAD | PNA_PART_TAIL, 0x7ffab2e6u);
    // solid on the device: plain, CTR, GCM (one IV / salt)
    auto solid_dev = [&](const char *what, const pna_gpu_cipher *ci, uint32_t want) {
        const size_t cap = pna_gpu_solid_archive_enc_bound(PNA_ALGO_ZSTD, n, names.data(), len.data(), ci) + 4096;
        Bytes dst(cap + 16); uint8_t *d = dst.data() + ((16 - ((uintptr_t)dst.data() & 15)) & 15);
        uint64_t alen = 0;
        CHECK(pna_gpu_create_solid_archive_enc_device(c, PNA_ALGO_ZSTD, 3, n, names.data(), src.data(), off.data(), len.data(), ci, d, cap, &alen, nullptr) == PNA_OK);
        framing_case(what, Bytes(d, d + alen), want);
    };
    solid_dev("solid device", nullptr, 0x316d41edu);
    solid_dev("solid device ctr", &ctr, 0xa9278512u);
    solid_dev("solid device gcm", &gcm, 0xa3c3d9cau);
    // solid from host memory in windows of 1 and 2 MiB: plain, CTR, GCM
    std::vector<const void *> hsrc(n); std::vector<size_t> hlen(n);
    Bytes big = text(3 << 20, 99);
    for (size_t i = 0; i < n; i++) { hsrc[i] = &src[off[i]]; hlen[i] = lens[i]; }
    hsrc.push_back(big.data()); hlen.push_back(big.size()); names.push_back("m/big.bin");
    for (long w = 1; w <= 2; w++) {
        CHECK(pna_gpu_set_option(c, "solid_win_mib", w) == PNA_OK);
        const pna_gpu_cipher *cs[3] = {nullptr, &ctr, &gcm}; const char *cn[3] = {"plain", "ctr", "gcm"};
        const uint32_t want[3] = {0xb815dc24u, 0x217ff317u, 0xfd55fdb1u};                 // (the same for both window sizes)
        for (int k = 0; k < 3; k++) {
            Bytes arc;
            CHECK(pna_gpu_create_solid_archive_enc_host(c, PNA_ALGO_ZSTD, 3, n + 1, names.data(), hsrc.data(), hlen.data(), cs[k], vec_sink, &arc) == PNA_OK);
            const std::string what = "solid host win=" + std::to_string(w) + " " + cn[k];
            framing_case(what.c_str(), arc, want[k]);
        }
    }
    pna_gpu_shutdown(c);
}

// Extract matrix: archives through pna_gpu_extract_archive_host -- stored entries (the decoders are not stubbed), solid streams, CTR / CBC under
// PBKDF2 and Argon2id PHSF strings, and the archives it must refuse.  Each case records the return code, the error text, the number of entries
// handed out and one CRC-32 over every callback's (index, name, kind, length, data), compared with the values recorded when the matrix was written.
struct XOut { size_t n = 0; uint32_t crc = 0; };
static int xsink(void *u, size_t index, const char *name, int kind, const void *data, size_t len) {
    XOut *o = (XOut *)u;
    const uint64_t il[2] = {index, len}; const int32_t k = kind;
    o->crc = pna_crc32(o->crc, il, sizeof il); o->crc = pna_crc32(o->crc, name, strlen(name) + 1); o->crc = pna_crc32(o->crc, &k, sizeof k);
    o->crc = pna_crc32(o->crc, data, data ? len : 0); o->n++;
    return 0;
}
static Bytes cat(std::initializer_list<Bytes> parts) { Bytes o; for (const Bytes &p : parts) o.insert(o.end(), p.begin(), p.end()); return o; }
static Bytes str(const std::string &s) { return Bytes(s.begin(), s.end()); }
static Bytes fhed_body(int kind, int comp, int enc, int mode, const std::string &name) { return cat({Bytes{0, 0, (uint8_t)kind, (uint8_t)comp, (uint8_t)enc, (uint8_t)mode}, str(name)}); }
static Bytes fsiz_body(uint64_t v) { Bytes b; for (int s = 56; s >= 0; s -= 8) if (!b.empty() || (uint8_t)(v >> s) || s == 0) b.push_back((uint8_t)(v >> s)); return b; }
static void test_extract_matrix() {
    pna_gpu_ctx *c = nullptr;
    CHECK(pna_gpu_init(&c, 0, PNA_F_DEFAULT) == PNA_OK);
    if (!c) return;
    const char *pw = "password";
    auto xcase = [&](const char *what, const Bytes &arc, const char *pass, int want_rc, const char *want_err, size_t want_n, uint32_t want_crc) {
        XOut o;
        const int rc = pna_gpu_extract_archive_host(c, arc.data(), arc.size(), pass, pass ? strlen(pass) : 0, xsink, &o);
        const std::string err = rc ? pna_gpu_last_error(c) : "";
        printf("extract %-28s rc %d n %zu crc %08x %s\n", what, rc, o.n, o.crc, err.c_str());
        if (rc != want_rc || err != want_err || o.n != want_n || o.crc != want_crc) {
            fprintf(stderr, "extract %s: rc %d \"%s\" n %zu crc %08x (recorded %d \"%s\" %zu %08x)\n", what, rc, err.c_str(), o.n, o.crc, want_rc, want_err, want_n, want_crc);
            g_fail++;
        }
    };
    auto writer = [](const std::function<void(pna_archive *)> &fill) {
        Bytes out; pna_archive *a = nullptr;
        CHECK(pna_archive_new(vec_sink, &out, 0, &a) == PNA_OK);
        if (a) { fill(a); CHECK(pna_archive_finalize(a) == PNA_OK); }
        return out;
    };
    auto inner = [](const char *name, const Bytes &d) {
        Bytes b(pna_archive_inner_entry_bytes(name, d.data(), d.size(), nullptr, 0));
        CHECK(pna_archive_inner_entry_bytes(name, d.data(), d.size(), b.data(), b.size()) == b.size());
        return b;
    };
    const Bytes t1 = text(5000, 1), t2 = text(70000, 2), t3 = text(300, 3);
    Bytes head; { pna_archive *a = nullptr; CHECK(pna_archive_new(vec_sink, &head, 0, &a) == PNA_OK); pna_archive_abort(a); }   // signature + AHED
    const Bytes aend = chunk("AEND", {}), fend = chunk("FEND", {});
    // ---- plain stored entries
    const Bytes plain = writer([&](pna_archive *a) {
        CHECK(pna_archive_add_file(a, "empty", 0, 0, nullptr, 0, 0) == PNA_OK);
        CHECK(pna_archive_add_dir(a, "d/sub") == PNA_OK);
        CHECK(pna_archive_add_file(a, "d/sub/t2", 0, (int64_t)t2.size(), t2.data(), t2.size(), 9000) == PNA_OK);
        CHECK(pna_archive_add_file(a, "nosize", 0, -1, t1.data(), t1.size(), 0) == PNA_OK);
    });
    xcase("plain", plain, nullptr, 0, "", 4, 0x8653a76du);
    const Bytes unsanitised = cat({head, chunk("FHED", fhed_body(0, 0, 0, 1, "/abs/./x/../y")), chunk("FDAT", t3), fend,
                                   chunk("FHED", fhed_body(0, 0, 0, 1, "../../up")), chunk("fSIZ", fsiz_body(t3.size())), chunk("FDAT", t3), fend, aend});
    xcase("names sanitised", unsanitised, nullptr, 0, "", 2, 0x7265ca23u);
    const Bytes big1 = text(700000, 4), big2 = text(900000, 5);
    const Bytes windows = writer([&](pna_archive *a) {
        CHECK(pna_archive_add_file(a, "w1", 0, (int64_t)big1.size(), big1.data(), big1.size(), 200000) == PNA_OK);
        CHECK(pna_archive_add_file(a, "w2", 0, (int64_t)big2.size(), big2.data(), big2.size(), 0) == PNA_OK);
        CHECK(pna_archive_add_file(a, "w3", 0, (int64_t)t2.size(), t2.data(), t2.size(), 0) == PNA_OK);
        CHECK(pna_archive_add_file(a, "w4", 0, (int64_t)big1.size(), big1.data(), big1.size(), 0) == PNA_OK);
    });
    CHECK(pna_gpu_set_option(c, "extract_win_mib", 1) == PNA_OK);
    xcase("windows of 1 MiB", windows, nullptr, 0, "", 4, 0xd6f865fbu);
    xcase("plain, windows of 1 MiB", plain, nullptr, 0, "", 4, 0x8653a76du);
    CHECK(pna_gpu_set_option(c, "extract_win_mib", 1024) == PNA_OK);
    xcase("windows of 1 GiB", windows, nullptr, 0, "", 4, 0xd6f865fbu);
    // ---- stored solid streams: between entries, alone (the deferred hand-out), inner records of several FDAT chunks
    const Bytes istream = cat({inner("s/a", t1), inner("s/empty", {}), inner("s/../b", t2)});
    const Bytes multi_fdat = cat({chunk("FHED", fhed_body(0, 0, 0, 1, "s/multi")), chunk("fSIZ", fsiz_body(t2.size())),
                                  chunk("FDAT", Bytes(t2.begin(), t2.begin() + 1000)), chunk("FDAT", Bytes(t2.begin() + 1000, t2.begin() + 1001)),
                                  chunk("FDAT", Bytes(t2.begin() + 1001, t2.end())), fend});
    auto solid_of = [&](const Bytes &st) {
        return writer([&](pna_archive *a) {
            const void *pcs[3] = {st.data(), st.data() + 7, st.data() + 4000}; const size_t pl[3] = {7, 3993, st.size() - 4000};
            CHECK(pna_archive_add_solid(a, 0, pcs, pl, 3) == PNA_OK);
        });
    };
    const Bytes between = writer([&](pna_archive *a) {
        CHECK(pna_archive_add_file(a, "before", 0, (int64_t)t1.size(), t1.data(), t1.size(), 0) == PNA_OK);
        const void *pcs[2] = {istream.data(), istream.data() + 100}; const size_t pl[2] = {100, istream.size() - 100};
        CHECK(pna_archive_add_solid(a, 0, pcs, pl, 2) == PNA_OK);
        CHECK(pna_archive_add_file(a, "after", 0, (int64_t)t3.size(), t3.data(), t3.size(), 0) == PNA_OK);
        const void *pc2[1] = {istream.data()}; const size_t pl2[1] = {istream.size()};
        CHECK(pna_archive_add_solid(a, 0, pc2, pl2, 1) == PNA_OK);
    });
    xcase("solid between entries", between, nullptr, 0, "", 8, 0xbe48525cu);
    xcase("solid alone", solid_of(istream), nullptr, 0, "", 3, 0x6deabe0fu);
    xcase("solid inner FDAT chunks", solid_of(cat({istream, multi_fdat})), nullptr, 0, "", 4, 0x3070098cu);
    // ---- encrypted stored entries: CTR / CBC, PBKDF2 and Argon2id, two PHSF strings (two key groups), a CTR solid stream
    uint8_t kp[32], ka[32]; char phsf_p[128];
    CHECK(pna_kdf_pbkdf2_sha256(pw, strlen(pw), "saltsaltsaltsalt", 16, 100, kp, 32, phsf_p, sizeof phsf_p) == PNA_OK);
    const std::string phsf_a = "$argon2id$v=19$m=64,t=1,p=1$c2FsdHNhbHRzYWx0c2FsdA";     // B64 of "saltsaltsaltsalt"
    CHECK(pna_kdf_argon2(2, pw, strlen(pw), "saltsaltsaltsalt", 16, 1, 64, 1, ka, 32) == PNA_OK);
    auto encrypt = [&](const uint8_t key[32], int mode, const Bytes &plain_, uint8_t seed) {     // IV || ciphertext
        uint8_t iv[16]; for (int i = 0; i < 16; i++) iv[i] = (uint8_t)(seed * 31 + i);
        const size_t clen = mode == PNA_MODE_CBC ? (plain_.size() / 16 + 1) * 16 : plain_.size();
        Bytes buf(clen + 16, 0); if (!plain_.empty()) memcpy(buf.data(), plain_.data(), plain_.size());
        pna_gpu_cipher ci{}; ci.encryption = PNA_ENC_AES; ci.cipher_mode = mode; memcpy(ci.key, key, 32); ci.phsf = ""; ci.ivs = iv;
        const uint64_t off = 0, len = plain_.size();
        CHECK(pna_gpu_cipher_apply_device(c, &ci, 0, 1, buf.data(), &off, &len, nullptr) == PNA_OK);
        Bytes o(iv, iv + 16); o.insert(o.end(), buf.begin(), buf.begin() + clen);
        return o;
    };
    auto enc_entry = [&](const char *name, const uint8_t key[32], const std::string &phsf, int mode, const Bytes &d, uint8_t seed) {
        const Bytes ct = encrypt(key, mode, d, seed);
        const size_t cut = ct.size() / 3;                                   // the IV and the data in pieces of their own
        return cat({chunk("FHED", fhed_body(0, 0, PNA_ENC_AES, mode, name)), chunk("fSIZ", fsiz_body(d.size())), chunk("PHSF", str(phsf)),
                    chunk("FDAT", Bytes(ct.begin(), ct.begin() + 16)), chunk("FDAT", Bytes(ct.begin() + 16, ct.begin() + 16 + cut)),
                    chunk("FDAT", Bytes(ct.begin() + 16 + cut, ct.end())), fend});
    };
    const Bytes enc_pbkdf2 = cat({head, enc_entry("e/ctr", kp, phsf_p, PNA_MODE_CTR, t2, 1), enc_entry("e/cbc", kp, phsf_p, PNA_MODE_CBC, t1, 2),
                                  enc_entry("e/cbc-empty", kp, phsf_p, PNA_MODE_CBC, {}, 3), enc_entry("e/ctr2", kp, phsf_p, PNA_MODE_CTR, t3, 4), aend});
    xcase("ctr + cbc pbkdf2", enc_pbkdf2, pw, 0, "", 4, 0x3751c832u);
    const Bytes enc_argon = cat({head, enc_entry("e/cbc", ka, phsf_a, PNA_MODE_CBC, t2, 5), enc_entry("e/ctr", ka, phsf_a, PNA_MODE_CTR, t1, 6), aend});
    xcase("ctr + cbc argon2id", enc_argon, pw, 0, "", 2, 0x9e63dc80u);
    const Bytes two_phsf = cat({head, enc_entry("k/1", kp, phsf_p, PNA_MODE_CTR, t1, 7), enc_entry("k/2", ka, phsf_a, PNA_MODE_CTR, t3, 8),
                                enc_entry("k/3", kp, phsf_p, PNA_MODE_CBC, t2, 9), aend});
    xcase("two PHSF strings", two_phsf, pw, 0, "", 3, 0xc9fa9303u);
    const Bytes sct = encrypt(ka, PNA_MODE_CTR, istream, 10);
    const Bytes solid_ctr = cat({head, chunk("SHED", Bytes{0, 0, 0, PNA_ENC_AES, PNA_MODE_CTR}), chunk("PHSF", str(phsf_a)), chunk("SDAT", Bytes(sct.begin(), sct.begin() + 16)),
                                 chunk("SDAT", Bytes(sct.begin() + 16, sct.begin() + 500)), chunk("SDAT", Bytes(sct.begin() + 500, sct.end())), chunk("SEND", {}), aend});
    xcase("solid ctr argon2id", solid_ctr, pw, 0, "", 3, 0x6deabe0fu);
    const Bytes cbc_only = cat({head, enc_entry("e/cbc", kp, phsf_p, PNA_MODE_CBC, t2, 11), aend});
    xcase("cbc wrong password", cbc_only, "passw0rd", -2, "CBC: bad length or padding (wrong password or damaged data)", 0, 0x00000000u);
    // ---- refusals
    const Bytes one = writer([&](pna_archive *a) { CHECK(pna_archive_add_file(a, "one", 0, (int64_t)t1.size(), t1.data(), t1.size(), 0) == PNA_OK); });
    const size_t fdat_at = one.size() - 12 - 12 - 4 - t1.size();          // FDAT body: in front of its CRC, FEND and AEND
    xcase("truncated chunk header", Bytes(one.begin(), one.end() - 5), nullptr, -2, "truncated chunk header", 0, 0x00000000u);
    xcase("truncated chunk body", cat({Bytes(one.begin(), one.end() - 12), Bytes{0, 0, 3, 0, 'F', 'D', 'A', 'T'}, Bytes(40, 1)}), nullptr, -2, "truncated chunk body", 0, 0x00000000u);
    { Bytes b = one; b[8 + 20 + 8 + 2] ^= 1; xcase("chunk CRC mismatch", b, nullptr, -2, "chunk CRC mismatch", 0, 0x00000000u); }
    { Bytes b = one; b[fdat_at + 100] ^= 1; xcase("FDAT CRC mismatch", b, nullptr, -2, "data chunk CRC mismatch (1 FDAT / SDAT chunks)", 0, 0x00000000u); }
    { Bytes b = between; b[b.size() - 40] ^= 1; xcase("SDAT CRC mismatch", b, nullptr, -2, "data chunk CRC mismatch (1 FDAT / SDAT chunks)", 5, 0xe47aa3cfu); }
    const Bytes xbad = chunk("XBAD", Bytes{1}), xanc = chunk("xanc", Bytes{2});
    xcase("critical chunk between entries", cat({Bytes(one.begin(), one.end() - 12), xanc, xbad, aend}), nullptr, -2, "unknown critical chunk between entries", 0, 0x00000000u);
    xcase("critical chunk in an entry", cat({head, chunk("FHED", fhed_body(0, 0, 0, 1, "x")), xanc, xbad, fend, aend}), nullptr, -2, "unknown critical chunk", 0, 0x00000000u);
    xcase("critical chunk in a solid entry", cat({head, chunk("SHED", Bytes{0, 0, 0, 0, 1}), xanc, xbad, chunk("SEND", {}), aend}), nullptr, -2, "unknown critical chunk in a solid entry", 0, 0x00000000u);
    xcase("bad SHED", cat({head, chunk("SHED", Bytes{0, 0, 0, 0}), chunk("SEND", {}), aend}), nullptr, -2, "bad solid header", 0, 0x00000000u);
    xcase("ANXT", cat({Bytes(one.begin(), one.end() - 12), chunk("ANXT", {}), aend}), nullptr, -7, "multipart archives are not read by this driver", 0, 0x00000000u);
    xcase("no AEND", Bytes(one.begin(), one.end() - 12), nullptr, -2, "archive not terminated by AEND", 0, 0x00000000u);
    xcase("stored fSIZ differs", cat({Bytes(one.begin(), one.end() - 12), chunk("FHED", fhed_body(0, 0, 0, 1, "short")), chunk("fSIZ", fsiz_body(t3.size() + 1)),
                                      chunk("FDAT", t3), fend, aend}), nullptr, -2, "stored entry: fSIZ differs from the data length", 1, 0xace9736au);
    xcase("xz", cat({head, chunk("FHED", fhed_body(0, 3, 0, 1, "xz")), chunk("FDAT", t3), fend, aend}), nullptr, -7, "compression method not decoded on the device (xz)", 0, 0x00000000u);
    xcase("encrypted, no password", enc_pbkdf2, nullptr, -2, "encrypted entry and no password", 0, 0x00000000u);
    xcase("camellia", cat({head, chunk("FHED", fhed_body(0, 0, PNA_ENC_CAMELLIA, PNA_MODE_CTR, "cam")), chunk("PHSF", str(phsf_p)), chunk("FDAT", t3), fend, aend}), pw, -7, "only AES entries are decrypted by this driver", 0, 0x00000000u);
    auto phsf_case = [&](const char *what, const std::string &phsf, int want_rc, const char *want_err) {
        xcase(what, cat({head, enc_entry("p", kp, phsf, PNA_MODE_CTR, t3, 12), aend}), pw, want_rc, want_err, 0, 0);
    };
    phsf_case("malformed PHSF", "$pbkdf2-sha256$i=100,l=32", -2, "malformed PHSF");
    phsf_case("malformed argon2 PHSF", "$argon2id$v=19$m=64,t=x,p=1$c2FsdA", -2, "malformed argon2 parameter in PHSF");
    phsf_case("argon2 cost above the cap", "$argon2id$v=19$m=4194305,t=1,p=1$c2FsdA", -7, "argon2 cost beyond the accepted maximum (m <= 4 GiB, t <= 64, p <= 256)");
    phsf_case("pbkdf2 rounds above the cap", "$pbkdf2-sha256$i=10000001,l=32$c2FsdA", -7, "pbkdf2 round count beyond the accepted maximum (10 000 000)");
    phsf_case("unknown password hash", "$scrypt$ln=4,r=8,p=1$c2FsdA", -7, "password hash other than argon2 / pbkdf2-sha256");
    xcase("inner entry not stored", solid_of(cat({istream, chunk("FHED", fhed_body(0, 2, 0, 1, "z")), fend})), nullptr, -7, "solid stream: inner entry that is not stored", 0, 0x00000000u);
    xcase("dangling inner chunks", solid_of(cat({istream, chunk("FHED", fhed_body(0, 0, 0, 1, "open")), chunk("FDAT", t3)})), nullptr, -2, "solid stream: dangling chunks", 0, 0x00000000u);
    xcase("inner FDAT CRC mismatch", [&] { Bytes st = istream; st[st.size() - 40] ^= 1; return solid_of(st); }(), nullptr, -2, "solid stream: inner FDAT CRC mismatch", 0, 0x00000000u);
    pna_gpu_shutdown(c);
}

// ---- the host create pipelines' other branches: compress_batch in pieces, zero-staging slots, the multi-context form, and a sink that fails
struct Entries {                                                 // n entries cut from one generated buffer (16-byte stride), with names
    Bytes buf; std::vector<std::string> nm; std::vector<const char *> names; std::vector<const void *> src; std::vector<size_t> len;
    Entries(const std::vector<size_t> &lens, uint32_t seed) {
        size_t at = 0; std::vector<size_t> off;
        for (size_t l : lens) { off.push_back(at); at = (at + l + 15) & ~(size_t)15; }
        buf = text(at + 16, seed);
        for (size_t i = 0; i < lens.size(); i++) { nm.push_back("e/" + std::to_string(i)); src.push_back(buf.data() + off[i]); len.push_back(lens[i]); }
        for (auto &s : nm) names.push_back(s.c_str());
    }
    size_t n() const { return len.size(); }
    bool same(const std::vector<std::pair<std::string, Bytes>> &ents) const {
        if (ents.size() != n()) return false;
        for (size_t i = 0; i < n(); i++) if (ents[i].first != nm[i] || ents[i].second != Bytes((const uint8_t *)src[i], (const uint8_t *)src[i] + len[i])) return false;
        return true;
    }
};
static pna_gpu_ctx *fresh_ctx(long sub_mib, long solid_win_mib) {
    pna_gpu_ctx *c = nullptr;
    CHECK(pna_gpu_init(&c, 0, PNA_F_DEFAULT) == PNA_OK && c);
    if (c) CHECK(pna_gpu_set_option(c, "sub_mib", sub_mib) == PNA_OK && pna_gpu_set_option(c, "solid_win_mib", solid_win_mib) == PNA_OK && pna_gpu_set_option(c, "latency_max_mib", 0) == PNA_OK);
    return c;
}
// entries of a solid archive written by the (stubbed) zstd path: the SDAT bodies are frames of raw blocks around the stored inner records
static bool read_back_solid(const Bytes &arc, std::vector<std::pair<std::string, Bytes>> &ents) {
    std::vector<Chunk> ch; if (!walk(arc, ch)) return false;
    Bytes pay, inner(8, 0);                                      // (walk skips a signature)
    for (const Chunk &c : ch) if (!strcmp(c.ty, "SDAT")) pay.insert(pay.end(), arc.begin() + c.off, arc.begin() + c.off + c.len);
    if (!unraw(pay.data(), pay.size(), inner)) return false;
    std::vector<Chunk> ic; if (!walk(inner, ic)) return false;
    for (const Chunk &c : ic) {
        if (!strcmp(c.ty, "FHED")) ents.emplace_back(std::string((const char *)&inner[c.off + 6], c.len - 6), Bytes());
        else if (!strcmp(c.ty, "FDAT") && !ents.empty()) ents.back().second.insert(ents.back().second.end(), inner.begin() + c.off, inner.begin() + c.off + c.len);
    }
    return true;
}
static void test_batch_in_pieces() {
    pna_gpu_ctx *c = fresh_ctx(16, 1);
    if (!c) return;
    const Entries e({700000, 420000, 0, 900000, 650000, 800000, 512345}, 4100);   // 1 MiB pieces: {0}, {1, 2}, {3}, {4}, {5, 6} -- the short last piece joined its neighbour
    const size_t n = e.n();
    std::vector<Bytes> out[2]; std::vector<size_t> dl[2];
    for (int k = 0; k < 2; k++) {
        CHECK(pna_gpu_set_option(c, "batch_piece_mib", k == 0 ? 0 : 1) == PNA_OK);
        out[k].resize(n); dl[k].resize(n);
        std::vector<void *> dst(n); std::vector<size_t> cap(n);
        for (size_t i = 0; i < n; i++) { out[k][i].resize(pna_gpu_bound(PNA_ALGO_ZSTD, e.len[i])); dst[i] = out[k][i].data(); cap[i] = out[k][i].size(); }
        CHECK(pna_gpu_compress_batch(c, PNA_ALGO_ZSTD, 3, n, e.src.data(), e.len.data(), dst.data(), cap.data(), dl[k].data()) == PNA_OK);
        for (size_t i = 0; i < n; i++) { out[k][i].resize(dl[k][i]); Bytes d; CHECK(unraw(out[k][i].data(), dl[k][i], d) && d == Bytes((const uint8_t *)e.src[i], (const uint8_t *)e.src[i] + e.len[i])); }
    }
    CHECK(out[0] == out[1]);
    pna_gpu_shutdown(c);
}
static void test_zero_staging_slots() {
    pna_gpu_ctx *c = fresh_ctx(16, 1);
    if (!c) return;
    std::vector<size_t> lens;
    for (size_t i = 0; i < 30; i++) lens.push_back(i == 7 ? 0 : 1200000 + 33333 * i);           // ~50 MiB: four sub-batches of 16 MiB
    const Entries e(lens, 4200);
    void *slot = nullptr;
    CHECK(pna_gpu_host_alloc(c, e.buf.size() + 4096 * e.n(), &slot) == PNA_OK && slot);
    if (!slot) { pna_gpu_shutdown(c); return; }
    // inside the lent buffer: the first ten entries adjacent at 16-byte stride as in `e`, the others with a gap of 4 KiB in front of each
    std::vector<const void *> lent(e.n());
    for (size_t i = 0; i < e.n(); i++) {
        uint8_t *p = (uint8_t *)slot + ((const uint8_t *)e.src[i] - e.buf.data()) + (i < 10 ? 0 : 4096 * (i - 9));
        if (e.len[i]) memcpy(p, e.src[i], e.len[i]);
        lent[i] = p;
    }
    std::vector<const void *> mixed = lent; mixed[12] = e.src[12];                              // one entry elsewhere: the call is staged
    Bytes arc[3];
    const std::vector<const void *> *srcs[3] = {&lent, &mixed, &e.src};
    for (int k = 0; k < 3; k++) {
        CHECK(pna_gpu_create_archive_host(c, PNA_ALGO_ZSTD, 3, e.n(), e.names.data(), srcs[k]->data(), e.len.data(), vec_sink, &arc[k]) == PNA_OK);
        std::vector<std::pair<std::string, Bytes>> ents;
        CHECK(read_back(arc[k], ents) && e.same(ents));
    }
    CHECK(arc[0] == arc[2] && arc[1] == arc[2]);
    int foreign = 0;
    CHECK(pna_gpu_host_free(c, &foreign) == PNA_E_INVAL);
    CHECK(pna_gpu_host_free(c, slot) == PNA_OK);
    pna_gpu_shutdown(c);
}
static void test_multi_context() {
    pna_gpu_ctx *cs[3] = {fresh_ctx(16, 1), fresh_ctx(16, 1), fresh_ctx(16, 1)};
    if (!cs[0] || !cs[1] || !cs[2]) return;
    const Entries many({300000, 0, 1500000, 70000, 900000, 1 << 20, 5000}, 4300), two({800000, 600000}, 4301), one({700000}, 4302);
    struct { const Entries *e; size_t n_ctx; } cases[] = {{&many, 2}, {&many, 3}, {&two, 3}, {&one, 2}};   // (the last two: a range without entries)
    for (auto &k : cases) {
        const Entries &e = *k.e;
        Bytes single, multi;
        CHECK(pna_gpu_create_archive_host(cs[0], PNA_ALGO_ZSTD, 3, e.n(), e.names.data(), e.src.data(), e.len.data(), vec_sink, &single) == PNA_OK);
        CHECK(pna_gpu_create_archive_multi_host(cs, k.n_ctx, PNA_ALGO_ZSTD, 3, e.n(), e.names.data(), e.src.data(), e.len.data(), vec_sink, &multi) == PNA_OK);
        std::vector<std::pair<std::string, Bytes>> ents;
        CHECK(read_back(multi, ents) && e.same(ents));
        CHECK(multi == single);
    }
    for (pna_gpu_ctx *c : cs) pna_gpu_shutdown(c);
}
// A sink that fails on its k-th call: the entry point returns PNA_E_SINK (with every thread of the pipeline stopped and joined: the sanitizers watch), and
// the same context then writes the archive a fresh context writes.
struct FailSink { Bytes out; size_t calls = 0, fail_at = 0; };
static int fail_sink(void *u, const void *b, size_t n) { FailSink *f = (FailSink *)u; if (++f->calls == f->fail_at) return 1; return vec_sink(&f->out, b, n); }
static void failing_sink_case(const char *what, const std::function<int(pna_gpu_ctx *const *, FailSink &)> &create, const Entries &e, bool solid, size_t min_calls) {
    pna_gpu_ctx *fresh[2] = {fresh_ctx(16, 1), fresh_ctx(16, 1)}, *used[2] = {fresh_ctx(16, 1), fresh_ctx(16, 1)};
    if (!fresh[0] || !fresh[1] || !used[0] || !used[1]) return;
    FailSink good;
    CHECK(create(fresh, good) == PNA_OK);
    std::vector<std::pair<std::string, Bytes>> ents;
    CHECK((solid ? read_back_solid(good.out, ents) : read_back(good.out, ents)) && e.same(ents));
    printf("failing sink %-18s %zu sink calls\n", what, good.calls);
    CHECK(good.calls >= min_calls);
    for (size_t at : {(size_t)1, good.calls / 2 + 1, good.calls}) {                            // the head, a piece in the middle, the tail
        FailSink bad; bad.fail_at = at;
        CHECK(create(used, bad) == PNA_E_SINK);
        CHECK(std::string(pna_gpu_last_error(used[0])) == "sink failed");
        FailSink again;
        CHECK(create(used, again) == PNA_OK);
        CHECK(again.out == good.out);
    }
    for (pna_gpu_ctx *c : fresh) pna_gpu_shutdown(c);
    for (pna_gpu_ctx *c : used) pna_gpu_shutdown(c);
}
static void test_failing_sink() {
    const Entries big(std::vector<size_t>(56, 1310720), 4400);                                  // 70 MiB: five sub-batches of 16 MiB
    failing_sink_case("create", [&](pna_gpu_ctx *const *cs, FailSink &s) {
        return pna_gpu_create_archive_host(cs[0], PNA_ALGO_ZSTD, 3, big.n(), big.names.data(), big.src.data(), big.len.data(), fail_sink, &s); }, big, false, 6);
    const Entries small({900000, 0, 1 << 20, 1400000, 12345, 850000}, 4401);                    // ~4 MiB: windows of 1 MiB
    failing_sink_case("solid", [&](pna_gpu_ctx *const *cs, FailSink &s) {
        return pna_gpu_create_solid_archive_host(cs[0], PNA_ALGO_ZSTD, 3, small.n(), small.names.data(), small.src.data(), small.len.data(), fail_sink, &s); }, small, true, 6);
    failing_sink_case("multi-context", [&](pna_gpu_ctx *const *cs, FailSink &s) {              // (range 0 owns the head and the middle call, the last range the tail)
        return pna_gpu_create_archive_multi_host(cs, 2, PNA_ALGO_ZSTD, 3, small.n(), small.names.data(), small.src.data(), small.len.data(), fail_sink, &s); }, small, false, 3);
}

// LZ launch matrix: what the host asks of the LZ stage's launch layer -- which form, over which segments or units, with which flag word, in which order -- for
// every branch of the stage's driver (pna_lz.cpp).  The device stub records one text row per launch; each case goes through pna_gpu_compress_batch_device on a
// context of its own and compares the CRC-32 of its rows (and of the error text of a failing call), the return code and pna_gpu_timing's lz_match_launches and
// lz_units with the values recorded when the matrix was written.  On a mismatch the rows are printed.
namespace pna { void lz_rows_begin(); std::string lz_rows_take(); }
struct LzOpt { const char *name; long v; };
struct LzCase { const char *what; uint32_t init; int algo, level; const std::vector<size_t> *lens; std::vector<LzOpt> opts; int rc; uint64_t launches; uint32_t units, crc; };
static void test_lz_launch_matrix() {
    const size_t K = 1024, M = K * K;
    std::vector<size_t> lat(2, 300 * K), seg(3, M + 1), mix{0, 100, 5000, 12000, 20000}, small{0, 100, 5000, 12000}, empty(3, 0), tail(600, 20 * K), tail700(700, 16400),
                        runs{0, M, M, 0, 0, M}, many(4200, 1), latmix{300 * K, 100, 300 * K, 5000};
    many.push_back(20 * K);
    const uint32_t D = PNA_F_DEFAULT; const int Z = PNA_ALGO_ZSTD, F = PNA_ALGO_DEFLATE;
    const LzOpt L0{"latency_max_mib", 0};
    const LzCase cases[] = {
        // latency mode: one launch over the units (zstd: the one-kernel form; the max set: the split form over the units), the short segments behind it
        {"units z3", D, Z, 3, &lat, {}, 0, 0, 38, 0x8d7c6783u},
        {"units z3 unit_log=14", D, Z, 3, &lat, {{"unit_log", 14}}, 0, 0, 38, 0x8d7c6783u},
        {"units z1", D, Z, 1, &lat, {}, 0, 0, 38, 0x2a8d6f3au},
        {"units z6", D, Z, 6, &lat, {}, 0, 0, 38, 0xd85a5819u},
        {"units z10 (global table)", D, Z, 10, &lat, {}, 0, 0, 38, 0x68b41dfau},
        {"units z19 strong_gtab=0", D, Z, 19, &lat, {{"strong_gtab", 0}}, 0, 0, 38, 0xd85a5819u},
        {"units d6", D, F, 6, &lat, {}, 0, 0, 38, 0x96e5f7b8u},
        {"units d1", D, F, 1, &lat, {}, 0, 0, 38, 0x21107ad3u},
        {"units d9 unit_log=14", D, F, 9, &lat, {{"unit_log", 14}}, 0, 0, 38, 0x3bdb3dcdu},
        {"units mix z3", D, Z, 3, &mix, {}, 0, 1, 0, 0x04be8ce0u},
        {"units mix z10", D, Z, 10, &mix, {}, 0, 1, 0, 0x9ddce176u},
        {"units mix d6", D, F, 6, &mix, {}, 0, 1, 0, 0x377df913u},
        {"units small z3 (all small)", D, Z, 3, &small, {}, 0, 1, 0, 0x9d54a23au},
        {"units small d6 (all small)", D, F, 6, &small, {}, 0, 1, 0, 0xff93768cu},
        {"units mtile=512 z3 (whole segments)", D, Z, 3, &lat, {{"mtile", 512}}, 0, 1, 0, 0x79f4e351u},
        {"units + short z3", D, Z, 3, &latmix, {}, 0, 0, 40, 0xbfe6c8fcu},
        {"units + short z10", D, Z, 10, &latmix, {}, 0, 0, 40, 0x0fb8713cu},
        {"units + short d6", D, F, 6, &latmix, {}, 0, 0, 40, 0x14943babu},
        {"units + short z3 small_geometry=0", D, Z, 3, &latmix, {{"small_geometry", 0}}, 0, 0, 40, 0x3c2d7301u},
        {"stored d0", D, F, 0, &lat, {}, 0, 0, 38, 0x00000000u},
        // whole segments: the split form, the level sets and their options
        {"segments z1", D, Z, 1, &seg, {L0}, 0, 1, 0, 0xadb0a290u},
        {"segments z3", D, Z, 3, &seg, {L0}, 0, 1, 0, 0x4a58e198u},
        {"segments z6", D, Z, 6, &seg, {L0}, 0, 1, 0, 0x1f7ede02u},
        {"segments z10", D, Z, 10, &seg, {L0}, 0, 1, 0, 0x5bdf0640u},
        {"segments z19", D, Z, 19, &seg, {L0}, 0, 1, 0, 0x5bdf0640u},
        {"segments d1", D, F, 1, &seg, {L0}, 0, 1, 0, 0x93506727u},
        {"segments d6", D, F, 6, &seg, {L0}, 0, 1, 0, 0x24a5ea4cu},
        {"segments d9", D, F, 9, &seg, {L0}, 0, 1, 0, 0x899b2039u},
        {"segments z3 win32k=0", D, Z, 3, &seg, {L0, {"win32k", 0}}, 0, 1, 0, 0x83e2cdbeu},
        {"segments z3 win32k=2", D, Z, 3, &seg, {L0, {"win32k", 2}}, 0, 1, 0, 0x24ea343eu},
        {"segments z3 tab3=0", D, Z, 3, &seg, {L0, {"tab3", 0}}, 0, 1, 0, 0x35763509u},
        {"segments z6 tab3=0", D, Z, 6, &seg, {L0, {"tab3", 0}}, 0, 1, 0, 0x460e95b1u},
        {"segments z6 strong2=0", D, Z, 6, &seg, {L0, {"strong2", 0}}, 0, 1, 0, 0x24ea343eu},
        {"segments z10 strong2=0", D, Z, 10, &seg, {L0, {"strong2", 0}}, 0, 1, 0, 0x748bee2du},
        {"segments z10 strong_gtab=0", D, Z, 10, &seg, {L0, {"strong_gtab", 0}}, 0, 1, 0, 0x1f7ede02u},
        {"segments z3 far1=0", D, Z, 3, &seg, {L0, {"far1", 0}}, 0, 1, 0, 0x57929486u},
        {"segments z3 lazy2=0", D, Z, 3, &seg, {L0, {"lazy2", 0}}, 0, 1, 0, 0x716dc5b0u},
        {"segments z3 lazy2=1", D, Z, 3, &seg, {L0, {"lazy2", 1}}, 0, 1, 0, 0x716dc5b0u},
        {"segments z1 lazy2=0", D, Z, 1, &seg, {L0, {"lazy2", 0}}, 0, 1, 0, 0x394b967cu},
        {"segments d6 lazy2=1", D, F, 6, &seg, {L0, {"lazy2", 1}}, 0, 1, 0, 0x9702d8a3u},
        // the forms: options, init flags, a workspace that cannot be had, mtile
        {"segments z3 lz_split=0", D, Z, 3, &seg, {L0, {"lz_split", 0}}, 0, 0, 0, 0xb3c2509cu},
        {"segments z3 lz_split=2", D, Z, 3, &seg, {L0, {"lz_split", 2}}, 0, 1, 0, 0xac692a45u},
        {"segments d6 lz_split=0", D, F, 6, &seg, {L0, {"lz_split", 0}}, 0, 0, 0, 0xc81cb6d0u},
        {"segments d6 lz_split=2", D, F, 6, &seg, {L0, {"lz_split", 2}}, 0, 1, 0, 0xf7c29d9fu},
        {"segments z10 lz_split=0 (stays split)", D, Z, 10, &seg, {L0, {"lz_split", 0}}, 0, 1, 0, 0x5bdf0640u},
        {"segments z10 lz_split=2 (stays k_lzp)", D, Z, 10, &seg, {L0, {"lz_split", 2}}, 0, 1, 0, 0x5bdf0640u},
        {"segments z3 FUSED", D | PNA_F_LZ_FUSED, Z, 3, &seg, {L0}, 0, 0, 0, 0xb3c2509cu},
        {"segments z3 WAVEPARSE", D | PNA_F_LZ_WAVEPARSE, Z, 3, &seg, {L0}, 0, 1, 0, 0xac692a45u},
        {"segments d6 FUSED", D | PNA_F_LZ_FUSED, F, 6, &seg, {L0}, 0, 0, 0, 0xc81cb6d0u},
        {"segments z3 FUSED + WAVEPARSE", D | PNA_F_LZ_FUSED | PNA_F_LZ_WAVEPARSE, Z, 3, &seg, {L0}, 0, 0, 0, 0xb3c2509cu},
        {"segments z3 stamps (0x100)", 0x177u, Z, 3, &seg, {L0}, 0, 0, 0, 0xe78da8b3u},
        {"segments z3 serial end scan (0x200)", 0x277u, Z, 3, &seg, {L0}, 0, 1, 0, 0x7cf3ab50u},
        {"segments d6 stamps + serial (0x300)", 0x377u, F, 6, &seg, {L0}, 0, 0, 0, 0xcd969fbbu},
        // (the init diagnostics 0x1000 / 0x2000 choose the sequence coder: they are not the launch flags of the same value)
        {"segments z1 init 0x1000 (no wave parse)", 0x1077u, Z, 1, &seg, {L0}, 0, 1, 0, 0x00444131u},
        {"segments z1 init 0x2000 (no 32 KiB window)", 0x2077u, Z, 1, &seg, {L0}, 0, 1, 0, 0xadb0a290u},
        {"segments d6 init 0x3000", 0x3077u, F, 6, &seg, {L0}, 0, 1, 0, 0x24a5ea4cu},
        // the parse kernel counts the sequence codes (seq_hist) where the entropy stage runs per segment; not behind the wave parse or the one-kernel form
        {"segments z3 hist_by_block=0", D, Z, 3, &seg, {L0, {"hist_by_block", 0}}, 0, 1, 0, 0xe7ac0239u},
        {"segments z3 hist_by_block=0 lz_split=2", D, Z, 3, &seg, {L0, {"hist_by_block", 0}, {"lz_split", 2}}, 0, 1, 0, 0x1886f8a5u},
        {"segments z3 hist_by_block=0 lz_split=0", D, Z, 3, &seg, {L0, {"hist_by_block", 0}, {"lz_split", 0}}, 0, 0, 0, 0x6e548919u},
        {"runs 2-1-3 z3 hist_by_block=0 lz_split_min=2", D, Z, 3, &runs, {L0, {"hist_by_block", 0}, {"lz_split_blocks", 8}, {"lz_split_min", 2}}, 0, 2, 0, 0x03df9a7du},
        {"units z3 hist_by_block=0", D, Z, 3, &lat, {{"hist_by_block", 0}}, 0, 0, 38, 0x50eabe06u},
        {"segments z3 lz_pbuf_fail", D, Z, 3, &seg, {L0, {"lz_pbuf_fail", 1}}, 0, 0, 0, 0xb3c2509cu},
        {"segments d6 lz_pbuf_fail", D, F, 6, &seg, {L0, {"lz_pbuf_fail", 1}}, 0, 0, 0, 0xc81cb6d0u},
        {"segments z10 lz_pbuf_fail (ignored)", D, Z, 10, &seg, {L0, {"lz_pbuf_fail", 1}}, 0, 1, 0, 0x5bdf0640u},
        {"segments z3 mtile=512", D, Z, 3, &seg, {L0, {"mtile", 512}}, 0, 1, 0, 0x650c09f5u},
        {"segments d6 mtile=2048", D, F, 6, &seg, {L0, {"mtile", 2048}}, 0, 1, 0, 0xfec2115fu},
        {"segments z10 mtile=512 (ignored)", D, Z, 10, &seg, {L0, {"mtile", 512}}, 0, 1, 0, 0x5bdf0640u},
        {"segments z3 mtile=512 FUSED (stays split)", D | PNA_F_LZ_FUSED, Z, 3, &seg, {L0, {"mtile", 512}}, 0, 1, 0, 0x650c09f5u},
        {"segments z3 mtile=512 lz_split=2", D, Z, 3, &seg, {L0, {"mtile", 512}, {"lz_split", 2}}, 0, 1, 0, 0x833dc228u},
        {"segments z3 mtile=512 lz_pbuf_fail", D, Z, 3, &seg, {L0, {"mtile", 512}, {"lz_pbuf_fail", 1}}, -3, 0, 0, 0x5a63b6b8u},
        // short segments next to a large one, alone, and none at all
        {"mix z3", D, Z, 3, &mix, {L0}, 0, 1, 0, 0x04be8ce0u},
        {"mix z6 lz_split=0", D, Z, 6, &mix, {L0, {"lz_split", 0}}, 0, 0, 0, 0xfb992f2cu},
        {"mix z3 lz_split=2", D, Z, 3, &mix, {L0, {"lz_split", 2}}, 0, 1, 0, 0x386efab7u},
        {"mix z3 lz_pbuf_fail", D, Z, 3, &mix, {L0, {"lz_pbuf_fail", 1}}, 0, 0, 0, 0x0f3df5aau},
        {"mix d6", D, F, 6, &mix, {L0}, 0, 1, 0, 0x377df913u},
        {"mix d9 lz_split=0", D, F, 9, &mix, {L0, {"lz_split", 0}}, 0, 0, 0, 0xd96a837du},
        {"mix z3 small_geometry=0", D, Z, 3, &mix, {L0, {"small_geometry", 0}}, 0, 1, 0, 0x80084eb4u},
        {"mix z3 mtile=512 lz_split=2", D, Z, 3, &mix, {L0, {"mtile", 512}, {"lz_split", 2}}, 0, 1, 0, 0x03fa108bu},
        {"small z3 (all small)", D, Z, 3, &small, {L0}, 0, 1, 0, 0x9d54a23au},
        {"small z3 lz_split=0", D, Z, 3, &small, {L0, {"lz_split", 0}}, 0, 0, 0, 0xf0aaad46u},
        {"small z3 lz_split=2", D, Z, 3, &small, {L0, {"lz_split", 2}}, 0, 1, 0, 0x01939e2fu},
        {"small z10", D, Z, 10, &small, {L0}, 0, 1, 0, 0xd4f836feu},
        {"small d6 mtile=512 (no sub-tiles)", D, F, 6, &small, {L0, {"mtile", 512}}, 0, 1, 0, 0xff93768cu},
        {"small z3 small_geometry=0", D, Z, 3, &small, {L0, {"small_geometry", 0}}, 0, 1, 0, 0xb9e51c78u},
        {"empty z3", D, Z, 3, &empty, {L0}, 0, 1, 0, 0xce1d5adau},
        {"empty z3 latency mode", D, Z, 3, &empty, {}, 0, 1, 0, 0xce1d5adau},
        {"empty d6 lz_split=0", D, F, 6, &empty, {L0, {"lz_split", 0}}, 0, 0, 0, 0x70b210beu},
        // the tail units: 600 mod 256 = 88 segments behind the last full round; 700 mod 256 = 188 is too many
        {"tail z3", D, Z, 3, &tail, {L0}, 0, 2, 0, 0x696f87ccu},
        {"tail z3 tail_units=0", D, Z, 3, &tail, {L0, {"tail_units", 0}}, 0, 1, 0, 0xabee78c0u},
        {"tail d6", D, F, 6, &tail, {L0}, 0, 2, 0, 0xc54b4c59u},
        {"tail z10 (global table: none)", D, Z, 10, &tail, {L0}, 0, 1, 0, 0x8061be88u},
        {"tail z3 lz_split=2 (none)", D, Z, 3, &tail, {L0, {"lz_split", 2}}, 0, 1, 0, 0x0e6e6718u},
        {"tail z3 mtile=512 (none)", D, Z, 3, &tail, {L0, {"mtile", 512}}, 0, 1, 0, 0x98c231cdu},
        {"tail z3 700 segments (none)", D, Z, 3, &tail700, {L0}, 0, 1, 0, 0xd38a31fdu},
        {"tail z3 lz_pbuf_fail (halved, then one kernel)", D, Z, 3, &tail, {L0, {"lz_pbuf_fail", 1}}, 0, 0, 0, 0xb867de41u},
        // several runs: one segment each; runs of 2, 1 and 3 segments with the short one in the middle taking the one-kernel form; runs evened to whole rounds
        {"runs z3 lz_split_blocks=8", D, Z, 3, &seg, {L0, {"lz_split_blocks", 8}}, 0, 6, 0, 0x3535d4c8u},
        {"runs d6 lz_split_blocks=8", D, F, 6, &seg, {L0, {"lz_split_blocks", 8}}, 0, 6, 0, 0x9afbf01eu},
        {"runs z3 lz_split_blocks=8 lz_split=0", D, Z, 3, &seg, {L0, {"lz_split_blocks", 8}, {"lz_split", 0}}, 0, 0, 0, 0x7e8683c7u},
        {"runs 2-1-3 z3 lz_split_blocks=8", D, Z, 3, &runs, {L0, {"lz_split_blocks", 8}}, 0, 3, 0, 0x5057be18u},
        {"runs 2-1-3 z3 lz_split_min=2", D, Z, 3, &runs, {L0, {"lz_split_blocks", 8}, {"lz_split_min", 2}}, 0, 2, 0, 0x1f3f0102u},
        {"runs 2-1-3 d6 lz_split_min=2", D, F, 6, &runs, {L0, {"lz_split_blocks", 8}, {"lz_split_min", 2}}, 0, 2, 0, 0x4303da9eu},
        {"runs 2-1-3 z3 lz_split_min=3", D, Z, 3, &runs, {L0, {"lz_split_blocks", 8}, {"lz_split_min", 3}}, 0, 1, 0, 0xc3579f81u},
        {"runs 2-1-3 z3 lz_split_min=4 (all one kernel)", D, Z, 3, &runs, {L0, {"lz_split_blocks", 8}, {"lz_split_min", 4}}, 0, 0, 0, 0x40702774u},
        {"runs 2-1-3 z10 lz_split_min=2 (ignored)", D, Z, 10, &runs, {L0, {"lz_split_blocks", 8}, {"lz_split_min", 2}}, 0, 3, 0, 0xad972255u},
        {"runs 2-1-3 z3 lz_split_min=2 lz_split=2 (ignored)", D, Z, 3, &runs, {L0, {"lz_split_blocks", 8}, {"lz_split_min", 2}, {"lz_split", 2}}, 0, 3, 0, 0x33e8d264u},
        {"runs 2-1-3 z3 lz_split_min=2 lz_pbuf_fail", D, Z, 3, &runs, {L0, {"lz_split_blocks", 8}, {"lz_split_min", 2}, {"lz_pbuf_fail", 1}}, 0, 0, 0, 0x682fe307u},
        {"runs evened z3 lz_split_blocks=2100", D, Z, 3, &many, {L0, {"blk_log", 17}, {"lz_split_blocks", 2100}}, 0, 3, 0, 0x35bfe524u},
        {"runs evened d6 lz_split_blocks=2100 lz_pbuf_fail", D, F, 6, &many, {L0, {"blk_log", 17}, {"lz_split_blocks", 2100}, {"lz_pbuf_fail", 1}}, 0, 0, 0, 0x15b58b66u},
        {"runs evened z3 lz_split_blocks=2100 small pass", D, Z, 3, &many, {L0, {"blk_log", 17}, {"lz_split_blocks", 2100}, {"lz_split", 0}}, 0, 0, 0, 0xec85229au},
    };
    const bool record = getenv("PNA_SAN_RECORD_LZ") != nullptr;         // print the table's last four columns instead of comparing (how the values were recorded)
    for (const LzCase &k : cases) {
        pna_gpu_ctx *c = nullptr;
        CHECK(pna_gpu_init(&c, 0, k.init) == PNA_OK);
        if (!c) return;
        for (const LzOpt &o : k.opts) CHECK(pna_gpu_set_option(c, o.name, o.v) == PNA_OK);
        const size_t n = k.lens->size();
        std::vector<uint64_t> off(n), len(n), doff(n + 1); uint64_t at = 0; size_t cap = 4096;
        for (size_t i = 0; i < n; i++) { off[i] = at; len[i] = (*k.lens)[i]; at = (at + len[i] + 15) & ~(uint64_t)15; cap += pna_gpu_bound(k.algo, (*k.lens)[i]); }
        const Bytes src = text(at + 64, 9000); Bytes dst(cap);
        pna::lz_rows_begin();
        const int rc = pna_gpu_compress_batch_device(c, k.algo, k.level, n, src.data(), off.data(), len.data(), dst.data(), cap, doff.data(), nullptr);
        std::string rows = pna::lz_rows_take();
        if (rc) rows += std::string("error: ") + pna_gpu_last_error(c) + "\n";
        pna_gpu_timing t; CHECK(pna_gpu_last_timing(c, &t) == PNA_OK);
        const uint32_t crc = pna_crc32(0, rows.data(), rows.size());
        if (record) printf("LZREC \"%s\" %d, %llu, %u, 0x%08xu\n", k.what, rc, (unsigned long long)t.lz_match_launches, t.lz_units, crc);
        else {
            printf("lz launches %-52s rc %d match launches %llu units %u crc %08x\n", k.what, rc, (unsigned long long)t.lz_match_launches, t.lz_units, crc);
            if (rc != k.rc || t.lz_match_launches != k.launches || t.lz_units != k.units || crc != k.crc) {
                fprintf(stderr, "lz launches %s: rc %d launches %llu units %u crc %08x (recorded %d %llu %u %08x); the rows:\n%s", k.what, rc, (unsigned long long)t.lz_match_launches,
                        t.lz_units, crc, k.rc, (unsigned long long)k.launches, k.units, k.crc, rows.c_str());
                g_fail++;
            }
        }
        if (record) fputs(rows.c_str(), stdout);
        pna_gpu_shutdown(c);
    }
}

int main() {
    if (getenv("PNA_SAN_RECORD_LZ")) { test_lz_launch_matrix(); return 0; }
    pna_gpu_ctx *c = nullptr;
    CHECK(pna_gpu_init(&c, 0, PNA_F_DEFAULT) == PNA_OK);
    if (!c) return 2;
    test_container();
    test_kdf();
    test_batch(c);
    test_streams(c);
    test_pipeline_and_append(c);
    test_batch_in_pieces();
    test_zero_staging_slots();
    test_multi_context();
    test_failing_sink();
    test_framing_matrix();
    test_extract_matrix();
    test_lz_launch_matrix();
    pna_gpu_shutdown(c);
    if (g_fail) { fprintf(stderr, "%d check(s) failed\n", g_fail); return 1; }
    printf("san_driver: all checks passed\n");
    return 0;
}
