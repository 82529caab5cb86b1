// pna_archive.cpp -- host-side PNA container writer (C ABI in include/pna_archive.h).
// Byte-exact restatement of the reference's writer for the chunks the compression path produces; every function
// cites the reference code it mirrors.  No compression happens here.
#include <stdint.h>
#include <string.h>
#include <string>
#include <vector>
#include <algorithm>
#include <sys/random.h>
#include "pna_ctx.h"
#include "kdf_core.h"

namespace {

// ---- CRC-32 (IEEE 802.3, reflected 0xEDB88320), slice-by-8 -- chunk_crc, lib/src/format/chunk.rs:7-12
struct CrcTables {
    uint32_t t[8][256];
    CrcTables() {
        for (uint32_t i = 0; i < 256; i++) {
            uint32_t c = i;
            for (int k = 0; k < 8; k++) c = (c & 1) ? (c >> 1) ^ 0xEDB88320u : c >> 1;
            t[0][i] = c;
        }
        for (uint32_t i = 0; i < 256; i++)
            for (int s = 1; s < 8; s++) t[s][i] = (t[s - 1][i] >> 8) ^ t[0][t[s - 1][i] & 0xFF];
    }
};
const CrcTables &crc_tables() { static CrcTables T; return T; }

} // namespace

namespace pna {
extern const uint8_t PNA_SIGNATURE[8] = {0x89, 0x50, 0x4E, 0x41, 0x0D, 0x0A, 0x1A, 0x0A};        // lib/src/format/signature.rs:6
void put_be32(uint8_t *p, uint32_t v) { p[0] = (uint8_t)(v >> 24); p[1] = (uint8_t)(v >> 16); p[2] = (uint8_t)(v >> 8); p[3] = (uint8_t)v; }
uint32_t rd_be32(const uint8_t *p) { return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3]; }
// One chunk of a chunk stream (read_chunk, lib/src/io.rs:117-149): length BE | type | body | crc BE.  The chunk at `pos` goes to `out` and `pos` moves
// behind it; the stream's end is not an error here, the callers decide what ends a walk.  No CRC is checked: chunk_crc_ok does that.
int next_chunk(const uint8_t *buf, size_t len, size_t &pos, PnaChunk &out) {
    if (pos > len || len - pos < 12) return CHUNK_SHORT_HEADER;
    const uint32_t l = rd_be32(buf + pos);
    if (len - pos - 12 < l) return CHUNK_SHORT_BODY;
    out = PnaChunk{pos, l, buf + pos + 4, buf + pos + 8};
    pos += 12 + (size_t)l;
    return CHUNK_OK;
}
// write_chunk (lib/src/io.rs:183-197): the 8 bytes in front of a chunk's body (length BE | type) and the 4 behind it (CRC-32 of type || body, BE)
static void chunk_frame(const void *ty, const void *data, size_t len, uint8_t head[8], uint8_t tail[4]) {
    put_be32(head, (uint32_t)len); memcpy(head + 4, ty, 4); put_be32(tail, pna_crc32(pna_crc32(0, ty, 4), data, len));
}
bool chunk_crc_ok(const PnaChunk &ch) { return pna_crc32(pna_crc32(0, ch.type, 4), ch.data, ch.len) == rd_be32(ch.data + ch.len); }
} // namespace pna

extern "C" uint32_t pna_crc32(uint32_t crc, const void *buf, size_t len) {
    const CrcTables &T = crc_tables();
    const uint8_t *p = (const uint8_t *)buf;
    uint32_t c = ~crc;
    while (len && ((uintptr_t)p & 7)) { c = T.t[0][(c ^ *p++) & 0xFF] ^ (c >> 8); len--; }
    while (len >= 8) {
        uint64_t v; memcpy(&v, p, 8);
        uint32_t lo = (uint32_t)v ^ c, hi = (uint32_t)(v >> 32);
        c = T.t[7][lo & 0xFF] ^ T.t[6][(lo >> 8) & 0xFF] ^ T.t[5][(lo >> 16) & 0xFF] ^ T.t[4][lo >> 24] ^
            T.t[3][hi & 0xFF] ^ T.t[2][(hi >> 8) & 0xFF] ^ T.t[1][(hi >> 16) & 0xFF] ^ T.t[0][hi >> 24];
        p += 8; len -= 8;
    }
    while (len--) c = T.t[0][(c ^ *p++) & 0xFF] ^ (c >> 8);
    return ~c;
}

struct pna_archive {
    pna_sink_fn sink; void *user; int err;
    int emit(const void *p, size_t n) { if (err) return err; if (n && sink(user, p, n) != 0) err = PNA_E_SINK; return err; }
    // write_chunk: length BE | type | data | crc32(type||data) BE -- lib/src/io.rs:183-197
    int chunk(const char ty[4], const void *data, size_t len) {
        if (len > 0xFFFFFFFFull) return err = PNA_E_INVAL;
        uint8_t head[8], tail[4]; chunk_frame(ty, data, len, head, tail);
        emit(head, 8); emit(data, len); return emit(tail, 4);
    }
};

// EntryName::sanitize (lib/src/entry/name.rs:148-156): the path is NORMALISED first (normalize_utf8path, lib/src/util/utf8path.rs:6-33:
// "." dropped, ".." pops the preceding normal component, "//" collapsed), then only the normal components are kept and joined by '/'.
// A ".." that finds nothing to pop (or only other ".." / the root) never survives the filter, so a stack of normal components is enough.
// '/' is the only separator: the reference splits at '\\' on Windows only (camino follows the host's std::path).
static std::string sanitize_n(const char *name, size_t n) {
    std::vector<std::pair<size_t, size_t>> st;          // (start, length) of the normal components kept so far
    size_t i = 0;
    while (i <= n) {
        size_t j = i;
        while (j < n && name[j] != '/') j++;
        const size_t len = j - i;
        if (len == 0 || (len == 1 && name[i] == '.')) { /* empty, "." */ }
        else if (len == 2 && name[i] == '.' && name[i + 1] == '.') { if (!st.empty()) st.pop_back(); }
        else st.emplace_back(i, len);
        i = j + 1;
    }
    std::string out;
    for (auto &c : st) { if (!out.empty()) out += '/'; out.append(name + c.first, c.second); }
    return out;
}
static std::string sanitize(const char *name) { return sanitize_n(name ? name : "", name ? strlen(name) : 0); }
namespace pna { std::string pna_sanitize_name(const char *name, size_t n) { return sanitize_n(name, n); } }      // the read side hands out EntryHeader::path(), the sanitised form

static std::vector<uint8_t> fhed(int kind, int compression, int encryption, int cipher_mode, const std::string &name) {
    // EntryHeader::to_bytes, lib/src/entry/header.rs:123-134
    std::vector<uint8_t> h = {0, 0, (uint8_t)kind, (uint8_t)compression, (uint8_t)encryption, (uint8_t)cipher_mode};
    h.insert(h.end(), name.begin(), name.end());
    return h;
}

static size_t fsiz(uint64_t raw, uint8_t out[16]) {        // u128 BE, leading zeros stripped -- lib/src/entry.rs:900-903
    uint8_t be[16] = {0};
    for (int i = 0; i < 8; i++) be[15 - i] = (uint8_t)(raw >> (8 * i));
    size_t skip = 0; while (skip < 16 && be[skip] == 0) skip++;
    memcpy(out, be + skip, 16 - skip);
    return 16 - skip;
}

// ---- pieces of the entry record used by the in-HBM framing path (pna_gpu_create_archive_device, pna_host.cpp)
namespace pna {
static void put_chunk(std::vector<uint8_t> &o, const char ty[4], const uint8_t *data, size_t len) {
    uint8_t head[8], tail[4]; chunk_frame(ty, data, len, head, tail);
    o.insert(o.end(), head, head + 8); if (len) o.insert(o.end(), data, data + len); o.insert(o.end(), tail, tail + 4);
}
// signature + AHED -- lib/src/archive/write.rs (write_header), lib/src/archive/header.rs:27-39
void frame_archive_head(std::vector<uint8_t> &o, uint32_t archive_number) {
    uint8_t ahed[8] = {0, 0, 0, 0, 0, 0, 0, 0}; put_be32(ahed + 4, archive_number);
    o.insert(o.end(), PNA_SIGNATURE, PNA_SIGNATURE + 8); put_chunk(o, "AHED", ahed, 8);
}
void frame_archive_tail(std::vector<uint8_t> &o) { put_chunk(o, "AEND", nullptr, 0); }
// FHED | fSIZ | FDAT length + type: everything of a file entry that precedes its payload (NormalEntry::write_chunks_to, lib/src/entry.rs:895-911)
// true when EntryName::sanitize would return the name unchanged: relative, '/'-separated, no empty / "." / ".." component
static bool name_is_clean(const char *name, size_t n) {
    if (n == 0 || name[0] == '/' || name[n - 1] == '/') return false;
    size_t comp = 0;
    for (size_t i = 0; i <= n; i++) {
        const char ch = i < n ? name[i] : '/';
        if (ch == '/') {
            if (comp == 0) return false;
            if (comp == 1 && name[i - 1] == '.') return false;
            if (comp == 2 && name[i - 1] == '.' && name[i - 2] == '.') return false;
            comp = 0;
        } else comp++;
    }
    return true;
}
// the same record pieces written straight into `out` (>= frame_entry_prefix_bound(name) bytes); returns the length.  The many-entry path
// (hundreds of thousands of 4 KiB files) builds one of these per entry on the host while the kernels run: no allocation, no string copy
// for names that are already in sanitised form.
size_t frame_entry_prefix_into(uint8_t *out, const char *name, int compression, uint64_t raw_size) {
    std::string tmp;
    const char *nm = name ? name : ""; size_t nl = strlen(nm);
    if (!name_is_clean(nm, nl)) { tmp = sanitize(nm); nm = tmp.c_str(); nl = tmp.size(); }
    uint8_t *p = out;
    put_be32(p, (uint32_t)(6 + nl)); memcpy(p + 4, "FHED", 4);
    p[8] = 0; p[9] = 0; p[10] = 0; p[11] = (uint8_t)compression; p[12] = 0; p[13] = 1;      // cipher_mode CTR (1) when unencrypted
    memcpy(p + 14, nm, nl);
    put_be32(p + 14 + nl, pna_crc32(0, p + 4, 4 + 6 + nl));
    p += 12 + 6 + nl;
    uint8_t b[16]; const size_t n = fsiz(raw_size, b);
    put_be32(p, (uint32_t)n); memcpy(p + 4, "fSIZ", 4); memcpy(p + 8, b, n);
    put_be32(p + 8 + n, pna_crc32(0, p + 4, 4 + n));
    p += 12 + n;
    put_be32(p, 0); memcpy(p + 4, "FDAT", 4);
    return (size_t)(p + 8 - out);
}
void frame_entry_prefix(std::vector<uint8_t> &o, const char *name, int compression, uint64_t raw_size, uint32_t payload_len) {
    std::vector<uint8_t> h = fhed(0, compression, 0, 1, sanitize(name));
    put_chunk(o, "FHED", h.data(), h.size());
    uint8_t b[16]; size_t n = fsiz(raw_size, b); put_chunk(o, "fSIZ", b, n);
    uint8_t head[8]; put_be32(head, payload_len); memcpy(head + 4, "FDAT", 4);
    o.insert(o.end(), head, head + 8);
}
// The same for an entry written with a cipher: FHED(encryption, cipher_mode) | fSIZ | PHSF | FDAT(iv) | FDAT length + type.  The IV is
// the data-stream prefix and becomes a data piece of its own (prepend_data_prefix, lib/src/entry/builder.rs:62-69,171-188); PHSF
// stands between the metadata and the data chunks (lib/src/entry.rs:905-910).
void frame_entry_prefix_enc(std::vector<uint8_t> &o, const char *name, int compression, uint64_t raw_size, int encryption, int cipher_mode,
                            const char *phsf, const uint8_t *prefix, size_t prefix_len) {
    std::vector<uint8_t> h = fhed(0, compression, encryption, cipher_mode, sanitize(name));
    put_chunk(o, "FHED", h.data(), h.size());
    uint8_t b[16]; size_t n = fsiz(raw_size, b); put_chunk(o, "fSIZ", b, n);
    put_chunk(o, "PHSF", (const uint8_t *)phsf, strlen(phsf));
    put_chunk(o, "FDAT", prefix, prefix_len);                  // block IV (CBC / CTR) or the 75-byte GCM stream header: prefix_bytes(), lib/src/entry/write.rs:46-51
    uint8_t head[8]; put_be32(head, 0); memcpy(head + 4, "FDAT", 4);
    o.insert(o.end(), head, head + 8);
}
size_t frame_entry_prefix_enc_bound(const char *name, const char *phsf) { return 12 + 6 + (name ? strlen(name) : 0) + 12 + 16 + 12 + strlen(phsf) + 12 + 75 + 8; }
// body of the FHED chunk of a file entry (what the GCM stream key is bound to: entry_context, lib/src/cipher/aead.rs:165-182)
std::vector<uint8_t> frame_fhed_bytes(const char *name, int compression, int encryption, int cipher_mode) { return fhed(0, compression, encryption, cipher_mode, sanitize(name)); }
// an inner entry of a solid archive without data: FHED | fSIZ | FEND, no FDAT (FlattenWriter ignores empty writes)
void frame_inner_entry_empty(std::vector<uint8_t> &o, const char *name) {
    std::vector<uint8_t> h = fhed(0, 0, 0, 1, sanitize(name));
    put_chunk(o, "FHED", h.data(), h.size());
    uint8_t b[16]; size_t n = fsiz(0, b); put_chunk(o, "fSIZ", b, n);
    put_chunk(o, "FEND", nullptr, 0);
}
// SHED chunk of an unencrypted solid entry -- lib/src/entry/header.rs:274-282; SEND -- lib/src/archive/write.rs:716-727
void frame_solid_head(std::vector<uint8_t> &o, int compression) { const uint8_t shed[5] = {0, 0, (uint8_t)compression, 0, 1}; put_chunk(o, "SHED", shed, 5); }
// SHED | PHSF | SDAT(iv) of a solid entry written with a cipher -- into_solid_archive, lib/src/archive/write.rs:443-470
void frame_solid_head_enc(std::vector<uint8_t> &o, int compression, int encryption, int cipher_mode, const char *phsf, const uint8_t *prefix, size_t prefix_len) {
    const uint8_t shed[5] = {0, 0, (uint8_t)compression, (uint8_t)encryption, (uint8_t)cipher_mode};
    put_chunk(o, "SHED", shed, 5);
    put_chunk(o, "PHSF", (const uint8_t *)phsf, strlen(phsf));
    put_chunk(o, "SDAT", prefix, prefix_len);                       // CTR: the IV; GCM STREAM: the stream header
}
void frame_solid_tail(std::vector<uint8_t> &o) { put_chunk(o, "SEND", nullptr, 0); }
// The whole record of an entry that is not a file -- kind 1 directory (DirEntryBuilder, EntryHeader::for_dir), 2 symbolic link, 3 hard link
// (SymlinkEntryBuilder::new / HardLinkEntryBuilder::new, cli/src/command/core.rs:938-955; for_symlink / for_hard_link, lib/src/entry/header.rs:65-78: compression 0,
// encryption 0, cipher_mode 0): FHED | extra | facets | FDAT* | FEND (NormalEntry::write_chunks_to, lib/src/entry.rs:895-911).  No fSIZ: only DataKind::FILE records one
// (lib/src/entry/builder.rs:630-632).  A link's target is stored and never encrypted (new_link takes WriteOptions::store(), builder.rs:341-349) and is cut into FDAT
// chunks as FlattenWriter cuts any stream (lib/src/util/io.rs:60-77); a directory has no data chunk.  `extra` / `facets`: chunks the caller has already framed.
void frame_nonfile_record(std::vector<uint8_t> &o, int kind, const char *name, const void *extra, size_t extra_len, const void *facets, size_t facets_len,
                          const void *target, size_t target_len, uint32_t max_chunk) {
    std::vector<uint8_t> h = fhed(kind, 0, 0, 0, sanitize(name));
    put_chunk(o, "FHED", h.data(), h.size());
    if (extra_len) o.insert(o.end(), (const uint8_t *)extra, (const uint8_t *)extra + extra_len);
    if (facets_len) o.insert(o.end(), (const uint8_t *)facets, (const uint8_t *)facets + facets_len);
    const size_t mx = max_chunk ? max_chunk : 0xFFFFFFFFull;
    if (kind != 1) for (size_t p = 0; p < target_len; p += mx) put_chunk(o, "FDAT", (const uint8_t *)target + p, std::min(mx, target_len - p));
    put_chunk(o, "FEND", nullptr, 0);
}
size_t frame_entry_prefix_bound(const char *name) { return 12 + 6 + (name ? strlen(name) : 0) + 12 + 16 + 8; }
uint32_t frame_fend_crc() { return pna_crc32(0, "FEND", 4); }
} // namespace pna

extern "C" int pna_archive_new(pna_sink_fn sink, void *user, uint32_t archive_number, pna_archive **out) {
    if (!sink || !out) return PNA_E_INVAL;
    pna_archive *a = new pna_archive{sink, user, 0};
    uint8_t ahed[8] = {0, 0, 0, 0, 0, 0, 0, 0}; put_be32(ahed + 4, archive_number);     // lib/src/archive/header.rs:27-39
    a->emit(PNA_SIGNATURE, 8); a->chunk("AHED", ahed, 8);
    if (a->err) { int e = a->err; delete a; return e; }
    *out = a; return PNA_OK;
}

extern "C" int pna_archive_add_file(pna_archive *a, const char *name, int compression, int64_t raw_size,
                                    const void *payload, size_t payload_len, uint32_t max_chunk_size) {
    if (!a || (!payload && payload_len)) return PNA_E_INVAL;
    // cipher_mode is CTR (1) when unencrypted: lib/src/entry/options.rs:156-159
    std::vector<uint8_t> h = fhed(0, compression, 0, 1, sanitize(name));
    a->chunk("FHED", h.data(), h.size());
    if (raw_size >= 0) { uint8_t b[16]; size_t n = fsiz((uint64_t)raw_size, b); a->chunk("fSIZ", b, n); }
    // FlattenWriter: one write of the whole stream -> pieces of at most max_chunk_size, lib/src/util/io.rs:60-77
    size_t mx = max_chunk_size ? max_chunk_size : 0xFFFFFFFFull;
    for (size_t p = 0; p < payload_len; p += mx) a->chunk("FDAT", (const uint8_t *)payload + p, std::min(mx, payload_len - p));
    return a->chunk("FEND", nullptr, 0);
}

extern "C" int pna_archive_add_dir(pna_archive *a, const char *name) {
    if (!a) return PNA_E_INVAL;
    std::vector<uint8_t> rec;
    frame_nonfile_record(rec, 1, name, nullptr, 0, nullptr, 0, nullptr, 0, 0);              // lib/src/entry/header.rs:44-52,65-67
    return a->emit(rec.data(), rec.size());
}

extern "C" size_t pna_archive_entry_record_bytes(int kind, const char *name, const void *extra, size_t extra_len, const void *facets, size_t facets_len,
                                                 const void *target, size_t target_len, uint32_t max_chunk_size, void *dst, size_t cap) {
    if (kind < 1 || kind > 3 || (extra_len && !extra) || (facets_len && !facets)) return 0;
    if (kind != 1 && (!target || !target_len)) return 0;          // a link without a target
    std::vector<uint8_t> rec;
    frame_nonfile_record(rec, kind, name, extra, extra_len, facets, facets_len, target, target_len, max_chunk_size);
    if (!dst) return rec.size();
    if (cap < rec.size()) return 0;
    memcpy(dst, rec.data(), rec.size());
    return rec.size();
}

extern "C" int pna_archive_add_solid(pna_archive *a, int compression, const void *const *pieces, const size_t *piece_len, size_t n) {
    if (!a || (n && (!pieces || !piece_len))) return PNA_E_INVAL;
    uint8_t shed[5] = {0, 0, (uint8_t)compression, 0, 1};                                 // lib/src/entry/header.rs:274-282
    a->chunk("SHED", shed, 5);
    for (size_t i = 0; i < n; i++) if (piece_len[i]) a->chunk("SDAT", pieces[i], piece_len[i]);   // chunk/write.rs:32-47
    return a->chunk("SEND", nullptr, 0);
}

extern "C" size_t pna_archive_inner_entry_bytes(const char *name, const void *data, size_t len, void *dst, size_t cap) {
    std::vector<uint8_t> h = fhed(0, 0, 0, 1, sanitize(name));
    uint8_t fs[16]; size_t fn = fsiz(len, fs);
    size_t need = (12 + h.size()) + (12 + fn) + (len ? 12 + len : 0) + 12;
    if (!dst) return need;
    if (cap < need) return 0;
    struct Mem { uint8_t *p; size_t pos; } m{(uint8_t *)dst, 0};
    auto sink = [](void *u, const void *b, size_t n) -> int { Mem *mm = (Mem *)u; memcpy(mm->p + mm->pos, b, n); mm->pos += n; return 0; };
    pna_archive tmp{sink, &m, 0};
    tmp.chunk("FHED", h.data(), h.size());
    tmp.chunk("fSIZ", fs, fn);
    if (len) tmp.chunk("FDAT", data, len);                    // an empty payload produces no FDAT (FlattenWriter ignores empty writes)
    tmp.chunk("FEND", nullptr, 0);
    return m.pos;
}

extern "C" int pna_archive_finalize(pna_archive *a) {
    if (!a) return PNA_E_INVAL;
    int rc = a->chunk("AEND", nullptr, 0);                     // lib/src/io.rs:45-51
    delete a; return rc;
}
extern "C" void pna_archive_abort(pna_archive *a) { delete a; }

// create_archive_file -- cli/src/command/create.rs:575-635
extern "C" int pna_create_archive(pna_gpu_ctx *ctx, int algo, int level, int solid, size_t n, const char *const *names,
                                  const void *const *src, const size_t *src_len, pna_sink_fn sink, void *user) {
    if (!sink || (n && (!names || !src || !src_len))) return PNA_E_INVAL;
    if (algo != PNA_ALGO_STORE && !ctx) return PNA_E_NODEVICE;
    // non-solid compressed archives: pipelined device path, archive bytes (framing + CRC included) come back from the GPU
    if (!solid && algo != PNA_ALGO_STORE) return pna_gpu_create_archive_host(ctx, algo, level, n, names, src, src_len, sink, user);
    if (solid && algo != PNA_ALGO_STORE) return pna_gpu_create_solid_archive_host(ctx, algo, level, n, names, src, src_len, sink, user);
    pna_archive *a = nullptr;
    int rc = pna_archive_new(sink, user, 0, &a);
    if (rc) return rc;
    if (!solid) {
        for (size_t i = 0; i < n && !rc; i++)                 // STORE; drain_entry_results: index order, core.rs:471-493
            rc = pna_archive_add_file(a, names[i], algo, (int64_t)src_len[i], src[i], src_len[i], 0);
    } else {
        // solid: inner entries are STORE (create.rs:594-598), serialised as chunk bytes, then ONE compressed stream
        std::vector<uint8_t> plain;
        for (size_t i = 0; i < n; i++) {
            size_t need = pna_archive_inner_entry_bytes(names[i], src[i], src_len[i], nullptr, 0);
            size_t at = plain.size(); plain.resize(at + need);
            pna_archive_inner_entry_bytes(names[i], src[i], src_len[i], plain.data() + at, need);
        }
        struct Pieces { std::vector<std::vector<uint8_t>> v; } pcs;
        if (algo == PNA_ALGO_STORE) { if (!plain.empty()) pcs.v.push_back(plain); }
        else {
            auto psink = [](void *u, const void *b, size_t l) -> int { ((Pieces *)u)->v.emplace_back((const uint8_t *)b, (const uint8_t *)b + l); return 0; };
            rc = pna_gpu_compress_solid(ctx, algo, level, plain.data(), plain.size(), psink, &pcs);
            if (rc) { pna_archive_abort(a); return rc; }
        }
        std::vector<const void *> pp; std::vector<size_t> pl;
        for (auto &v : pcs.v) { pp.push_back(v.data()); pl.push_back(v.size()); }
        rc = pna_archive_add_solid(a, algo, pp.data(), pl.data(), pp.size());
    }
    if (rc) { pna_archive_abort(a); return rc; }
    return pna_archive_finalize(a);
}

// ---------------------------------------------------------------------------------------------------------
// Password hashing for `pna create --aes --pbkdf2` on the C++ host: PBKDF2-HMAC-SHA-256 (FIPS 180-4, RFC 2104, RFC 8018), the
// reference's hash::pbkdf2_with_salt (lib/src/hash.rs:35-45; pbkdf2 0.12 defaults: 600 000 rounds, 32-byte output) with a
// password-hash SaltString (16 random bytes, B64 without padding; the hash function is fed the decoded bytes).
namespace {
typedef KdfSha256 Sha256;                                     // kdf_core.h: SHA-256 and HMAC, one home for the host code and k_kdf.hip
typedef KdfHmac Hmac;
const char B64[] = "ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789+/";
std::string b64_nopad(const uint8_t *p, size_t n) {
    std::string o;
    for (size_t i = 0; i < n; i += 3) {
        const uint32_t v = ((uint32_t)p[i] << 16) | ((i + 1 < n ? (uint32_t)p[i + 1] : 0u) << 8) | (i + 2 < n ? (uint32_t)p[i + 2] : 0u);
        o += B64[(v >> 18) & 63]; o += B64[(v >> 12) & 63];
        if (i + 1 < n) o += B64[(v >> 6) & 63];
        if (i + 2 < n) o += B64[v & 63];
    }
    return o;
}
} // namespace

namespace pna {
bool b64_decode_nopad(const std::string &s, std::vector<uint8_t> &out) {       // the salt of a PHSF string: the inverse of b64_nopad
    uint32_t acc = 0; int bits = 0;
    for (char ch : s) { const char *q = ch ? strchr(B64, ch) : nullptr; if (!q) return false; acc = (acc << 6) | (uint32_t)(q - B64); bits += 6; if (bits >= 8) { bits -= 8; out.push_back((uint8_t)(acc >> bits)); } }
    return true;
}
void sha256_bytes(const void *a, size_t an, const void *b, size_t bn, uint8_t out[32]) { Sha256 s; s.init(); s.update(a, an); if (bn) s.update(b, bn); s.final(out); }
// HKDF-SHA-256 with one output block (RFC 5869): hkdf_sha256, lib/src/cipher/aead.rs:151-157
void hkdf_sha256_32(const void *ikm, size_t ikm_len, const void *salt, size_t salt_len, const void *info, size_t info_len, uint8_t okm[32]) {
    static const uint8_t zero[32] = {0};
    Hmac ex; if (salt_len) ex.key((const uint8_t *)salt, salt_len); else ex.key(zero, 32);
    uint8_t prk[32]; ex.mac(ikm, ikm_len, nullptr, 0, prk);
    Hmac xp; xp.key(prk, 32);
    const uint8_t one = 1;
    std::vector<uint8_t> m((const uint8_t *)info, (const uint8_t *)info + info_len); m.push_back(one);
    xp.mac(m.data(), m.size(), nullptr, 0, okm);
}
}

extern "C" int pna_kdf_pbkdf2_sha256(const void *password, size_t password_len, const void *salt, size_t salt_len, uint32_t rounds,
                                     uint8_t *key, size_t key_len, char *phsf, size_t phsf_cap) {
    if ((!password && password_len) || (!salt && salt_len) || !key || rounds == 0) return PNA_E_INVAL;
    for (uint32_t blk = 1; key_len; blk++) {                  // kdf_core.h: the pad states and U_1, then the chain of two compressions per round
        KdfPbkdf2Start ps; kdf_pbkdf2_start(password, password_len, salt, salt_len, blk, ps);
        uint32_t tw[8]; uint8_t t[32];
        kdf_pbkdf2_chain(ps.istate, ps.ostate, ps.u1, rounds, tw); kdf_words_be(tw, t);
        const size_t k = std::min<size_t>(key_len, 32);
        memcpy(key, t, k); key += k; key_len -= k;
    }
    if (phsf) {                                                // PasswordHash::to_string() after hash.take(): "$pbkdf2-sha256$i=<rounds>,l=<len>$<salt>"
        const std::string s = "$pbkdf2-sha256$i=" + std::to_string(rounds) + ",l=32$" + b64_nopad((const uint8_t *)salt, salt_len);
        if (s.size() + 1 > phsf_cap) return PNA_E_DSTSIZE;
        memcpy(phsf, s.c_str(), s.size() + 1);
    }
    return PNA_OK;
}


// ---------------------------------------------------------------------------------------------------------
// Argon2 (RFC 9106, version 0x13, no secret / associated data) on the C++ host: the reference's default password hash
// (hash::argon2_with_salt / derive_password_hash, lib/src/hash.rs:6-33,47-70; argon2 0.5.3).  The read side needs it to open archives
// the reference wrote; the key is the raw hash output of key_size() bytes (lib/src/entry/write.rs:146-151).
// kind: 0 Argon2d, 1 Argon2i, 2 Argon2id
extern "C" int pna_kdf_argon2(int kind, const void *password, size_t password_len, const void *salt, size_t salt_len,
                              uint32_t t_cost, uint32_t m_cost_kib, uint32_t lanes, uint8_t *key, size_t key_len) {
    if ((!password && password_len) || (!salt && salt_len) || !key || kind < 0 || kind > 2) return PNA_E_INVAL;
    if (lanes < 1 || lanes > 0xFFFFFF || t_cost < 1 || m_cost_kib < 8 * lanes || key_len < 4 || key_len > 1024 || m_cost_kib > (1u << 24)) return PNA_E_INVAL;
    const KdfArgonGeom g = kdf_argon_geom(kind, t_cost, m_cost_kib, lanes);      // kdf_core.h: the whole of the algorithm
    std::vector<uint64_t> mem;
    try { mem.resize((size_t)g.blocks * 128); } catch (...) { return PNA_E_NOMEM; }
    uint8_t h0[72];
    kdf_argon_h0(g, m_cost_kib, (uint32_t)key_len, password, password_len, salt, salt_len, h0);
    for (uint32_t l = 0; l < lanes; l++) for (uint32_t j = 0; j < 2; j++) kdf_argon_seed(h0, l, j, mem.data() + ((size_t)l * g.lane_len + j) * 128);
    for (uint32_t pass = 0; pass < t_cost; pass++)
        for (uint32_t slice = 0; slice < 4; slice++)
            for (uint32_t lane = 0; lane < lanes; lane++) kdf_argon_fill_segment(mem.data(), g, pass, slice, lane);
    uint64_t fin[128];
    memcpy(fin, mem.data() + ((size_t)g.lane_len - 1) * 128, sizeof fin);
    for (uint32_t l = 1; l < lanes; l++) for (int i = 0; i < 128; i++) fin[i] ^= mem[((size_t)l * g.lane_len + g.lane_len - 1) * 128 + i];
    kdf_argon_tag(fin, key, (uint32_t)key_len);
    return PNA_OK;
}

// `pna create --aes [ctr|cbc] --password ... --pbkdf2`: one key derivation per archive (WriteOptions caches it, lib/src/entry/options.rs),
// a fresh IV per entry; non-solid zstd / deflate archives on the device path.
extern "C" int pna_create_archive_encrypted(pna_gpu_ctx *ctx, int algo, int level, size_t n, const char *const *names,
                                            const void *const *src, const size_t *src_len, const void *password, size_t password_len,
                                            int cipher_mode, uint32_t rounds, pna_sink_fn sink, void *user) {
    if (!ctx) return PNA_E_NODEVICE;
    if (!sink || (!password && password_len)) return PNA_E_INVAL;
    uint8_t salt[16];
    if (getrandom(salt, sizeof salt, 0) != (ssize_t)sizeof salt) return PNA_E_INVAL;
    pna_gpu_cipher ci{};
    ci.encryption = PNA_ENC_AES; ci.cipher_mode = cipher_mode; ci.ivs = nullptr;
    char phsf[128];
    int rc = pna_kdf_pbkdf2_sha256(password, password_len, salt, sizeof salt, rounds ? rounds : 600000u, ci.key, 32, phsf, sizeof phsf);
    if (rc) return rc;
    ci.phsf = phsf;
    return pna_gpu_create_archive_enc_host(ctx, algo, level, n, names, src, src_len, &ci, sink, user);
}

// The password hash of WriteOptions (hash(), lib/src/entry/write.rs:153-186): Argon2id by default (lib/src/entry/options.rs:164) with the argon2
// crate's default parameters (m = 19456 KiB, t = 2, p = 1), or PBKDF2-SHA256; the PHSF is the PHC string without the hash,
// "$argon2id$v=19$m=19456,t=2,p=1$<salt B64, no padding>" / "$pbkdf2-sha256$i=<rounds>,l=32$<salt>".
extern "C" int pna_kdf_derive(int kdf, const void *password, size_t password_len, const void *salt, size_t salt_len, uint32_t rounds,
                              uint8_t *key, char *phsf, size_t phsf_cap) {
    if ((!password && password_len) || !salt || !salt_len || !key || !phsf) return PNA_E_INVAL;
    if (kdf == PNA_KDF_PBKDF2_SHA256) return pna_kdf_pbkdf2_sha256(password, password_len, salt, salt_len, rounds ? rounds : 600000u, key, 32, phsf, phsf_cap);
    if (kdf != PNA_KDF_ARGON2ID) return PNA_E_INVAL;
    const std::string s = "$argon2id$v=19$m=19456,t=2,p=1$" + b64_nopad((const uint8_t *)salt, salt_len);
    if (s.size() + 1 > phsf_cap) return PNA_E_DSTSIZE;
    int rc = pna_kdf_argon2(2, password, password_len, salt, salt_len, 2, 19456, 1, key, 32);
    if (rc) return rc;
    memcpy(phsf, s.c_str(), s.size() + 1);
    return PNA_OK;
}

// `pna create [--solid] --aes [ctr|cbc|gcm] --password ... [--argon2 | --pbkdf2]`: one key per archive over a fresh 16-byte salt
// (SaltString::generate).  Solid archives: pna_gpu_create_solid_archive_enc_host; others: pna_gpu_create_archive_enc_host.
extern "C" int pna_create_archive_encrypted_ex(pna_gpu_ctx *ctx, int algo, int level, int solid, size_t n, const char *const *names,
                                               const void *const *src, const size_t *src_len, const void *password, size_t password_len,
                                               int cipher_mode, int kdf, uint32_t rounds, pna_sink_fn sink, void *user) {
    return pna_create_archive_encrypted_with(ctx, algo, level, solid, n, names, src, src_len, password, password_len, PNA_ENC_AES, cipher_mode, kdf, rounds, sink, user);
}
// ... with the block cipher named too: `--aes` or `--camellia` (PNA_ENC_CAMELLIA: on a context with option "camellia" = 1)
extern "C" int pna_create_archive_encrypted_with(pna_gpu_ctx *ctx, int algo, int level, int solid, size_t n, const char *const *names,
                                                 const void *const *src, const size_t *src_len, const void *password, size_t password_len,
                                                 int encryption, int cipher_mode, int kdf, uint32_t rounds, pna_sink_fn sink, void *user) {
    if (!ctx) return PNA_E_NODEVICE;
    if (!sink || (!password && password_len)) return PNA_E_INVAL;
    uint8_t salt[16];
    if (getrandom(salt, sizeof salt, 0) != (ssize_t)sizeof salt) return PNA_E_INVAL;
    pna_gpu_cipher ci{};
    ci.encryption = encryption; ci.cipher_mode = cipher_mode; ci.ivs = nullptr;
    char phsf[128];
    int rc = pna_kdf_derive(kdf, password, password_len, salt, sizeof salt, rounds, ci.key, phsf, sizeof phsf);
    if (rc) return rc;
    ci.phsf = phsf;
    if (solid) return pna_gpu_create_solid_archive_enc_host(ctx, algo, level, n, names, src, src_len, &ci, sink, user);
    return pna_gpu_create_archive_enc_host(ctx, algo, level, n, names, src, src_len, &ci, sink, user);
}

// ---------------------------------------------------------------------------------------------------------
// Multipart archives (`pna create --split`): SplitParts, lib/src/archive/split_parts.rs.  The device paths produce ONE archive image;
// this re-frames its chunk stream into parts of at most max_part_bytes: every part opens with the signature + AHED(archive number),
// closes with [ANXT] AEND; a chunk that fits goes out untouched (its CRC is reused), a non-stream chunk that does not fit opens the next
// part, an FDAT / SDAT chunk is cut at the budget boundary and only its fragments get new CRCs (put_chunk / put_stream, :140-173).
namespace {
struct PartOut {
    pna_part_sink_fn sink; void *user; uint32_t part = 0; int err = 0;
    void emit(const void *p, size_t n) { if (!err && n && sink(user, part, p, n) != 0) err = PNA_E_SINK; }
    void header() {
        uint8_t c[20]; put_be32(c, 8); memcpy(c + 4, "AHED", 4); memset(c + 8, 0, 4); put_be32(c + 12, part);
        put_be32(c + 16, pna_crc32(0, c + 4, 12));
        emit(PNA_SIGNATURE, 8); emit(c, 20);
    }
    void empty_chunk(const char ty[4]) { uint8_t c[12]; chunk_frame(ty, nullptr, 0, c, c + 8); emit(c, 12); }
    void fresh_chunk(const uint8_t *ty, const uint8_t *data, size_t n) {
        uint8_t h[8], t[4]; chunk_frame(ty, data, n, h, t);
        emit(h, 8); emit(data, n); emit(t, 4);
    }
};
}

extern "C" int pna_split_archive(const void *archive, size_t len, size_t max_part_bytes, pna_part_sink_fn sink, void *user, uint32_t *n_parts) {
    if (!archive || !sink) return PNA_E_INVAL;
    const size_t MINC = 12, OVER = 8 + 20 + 2 * MINC;          // MIN_CHUNK_BYTES_SIZE, SPLIT_ARCHIVE_OVERHEAD_BYTES (split_parts.rs:14-23)
    if (max_part_bytes < OVER + MINC) return PNA_E_INVAL;      // MIN_SPLIT_PART_BYTES
    const uint8_t *a = (const uint8_t *)archive;
    if (len < 8 + 20 + 12 || memcmp(a, PNA_SIGNATURE, 8) != 0 || memcmp(a + 12, "AHED", 4) != 0) return PNA_E_INVAL;
    const size_t budget = max_part_bytes - OVER;
    size_t remaining = budget;
    PartOut o{sink, user};
    o.header();
    auto roll_over = [&]() -> int {
        if (o.part == 0xFFFFFFFFu) return PNA_E_INVAL;          // part_number_overflow_error
        o.empty_chunk("ANXT"); o.empty_chunk("AEND");
        o.part++; o.header(); remaining = budget;
        return o.err;
    };
    size_t pos = 8 + 20; bool ended = false;
    while (pos < len && !o.err) {
        PnaChunk ch;
        if (next_chunk(a, len, pos, ch)) return PNA_E_INVAL;
        const size_t clen = MINC + ch.len, at = ch.off;
        if (memcmp(ch.type, "AEND", 4) == 0) { ended = true; break; }
        if (memcmp(ch.type, "ANXT", 4) == 0) return PNA_E_INVAL;     // already a part of a multipart archive
        const bool stream = memcmp(ch.type, "FDAT", 4) == 0 || memcmp(ch.type, "SDAT", 4) == 0;
        if (clen <= remaining) { o.emit(a + at, clen); remaining -= clen; }
        else if (!stream) {
            if (clen > budget) return PNA_E_INVAL;              // chunk_does_not_fit_error
            int rc = roll_over(); if (rc) return rc;
            o.emit(a + at, clen); remaining -= clen;
        } else if (clen <= budget && remaining <= MINC) {
            int rc = roll_over(); if (rc) return rc;
            o.emit(a + at, clen); remaining -= clen;
        } else {
            const uint8_t *rest = ch.data; size_t rl = ch.len; bool first = true;
            for (;;) {
                if (MINC + rl <= remaining) {
                    if (first) o.emit(a + at, clen); else o.fresh_chunk(ch.type, rest, rl);   // (cannot be `first` here, kept for symmetry)
                    remaining -= MINC + rl; break;
                }
                if (remaining > MINC) {
                    const size_t take = remaining - MINC;
                    o.fresh_chunk(ch.type, rest, take); rest += take; rl -= take; remaining -= MINC + take; first = false;
                } else if (budget <= MINC) return PNA_E_INVAL;
                int rc = roll_over(); if (rc) return rc;
            }
        }
    }
    if (!ended) return o.err ? o.err : PNA_E_INVAL;
    o.empty_chunk("AEND");                                      // finalize_archive: the last part has no ANXT
    if (n_parts) *n_parts = o.part + 1;
    return o.err;
}

// The reading side (Archive::read_next_archive): parts in order -> ONE archive image (signature + AHED(0) + the concatenated chunk
// streams + AEND) that pna_gpu_extract_archive_host and every other reader take; FDAT / SDAT fragments stay separate chunks (their
// bodies are concatenated by the entry reader anyway).
extern "C" int pna_join_parts(const void *const *parts, const size_t *part_len, size_t n, pna_sink_fn sink, void *user) {
    if (!parts || !part_len || !sink || n == 0) return PNA_E_INVAL;
    auto out = [&](const void *p, size_t k) { return k == 0 || sink(user, p, k) == 0; };
    for (size_t k = 0; k < n; k++) {
        const uint8_t *a = (const uint8_t *)parts[k]; const size_t len = part_len[k];
        if (!a || len < 8 + 20 + 12 || memcmp(a, PNA_SIGNATURE, 8) != 0 || memcmp(a + 12, "AHED", 4) != 0) return PNA_E_INVAL;
        if (rd_be32(a + 20) != k || pna_crc32(0, a + 12, 12) != rd_be32(a + 24)) return PNA_E_INVAL;      // AHED body: major, minor, 0, 0, archive number
        if (k == 0 && !out(a, 28)) return PNA_E_SINK;
        size_t pos = 28; bool has_next = false, ended = false;
        while (pos < len) {
            PnaChunk ch;
            if (next_chunk(a, len, pos, ch)) return PNA_E_INVAL;
            if (memcmp(ch.type, "AEND", 4) == 0) { ended = true; break; }
            if (memcmp(ch.type, "ANXT", 4) == 0) has_next = true;
            else { if (has_next) return PNA_E_INVAL; if (!out(a + ch.off, 12 + (size_t)ch.len)) return PNA_E_SINK; }
        }
        if (!ended || has_next != (k + 1 < n)) return PNA_E_INVAL;
    }
    uint8_t c[12]; chunk_frame("AEND", nullptr, 0, c, c + 8);
    return out(c, 12) ? PNA_OK : PNA_E_SINK;
}


// ---- `pna append` / `pna update` plumbing on the host (include/pna_archive.h)
static bool pna_image_header_ok(const uint8_t *a, size_t len) {
    // signature, then AHED as the first chunk (Archive::read_header, lib/src/archive/read.rs:26-44)
    return len >= 8 + 12 + 8 && memcmp(a, PNA_SIGNATURE, 8) == 0 && memcmp(a + 12, "AHED", 4) == 0 && a[8] == 0 && a[9] == 0 && a[10] == 0 && a[11] == 8;
}
extern "C" int pna_archive_seek_to_end(const void *archive, size_t len, uint64_t *aend_off, int *has_next) {
    if (!archive || !aend_off) return PNA_E_INVAL;
    const uint8_t *a = (const uint8_t *)archive;
    if (!pna_image_header_ok(a, len)) return PNA_E_INVAL;
    if (has_next) *has_next = 0;
    size_t pos = 8;
    for (;;) {
        PnaChunk ch;
        if (next_chunk(a, len, pos, ch)) return PNA_E_INVAL;                 // truncated: UnexpectedEof
        if (memcmp(ch.type, "AEND", 4) == 0) { *aend_off = ch.off; return PNA_OK; }
        if (memcmp(ch.type, "ANXT", 4) == 0 && has_next) *has_next = 1;
    }
}
extern "C" int pna_archive_list_entries(const void *archive, size_t len, pna_raw_entry_fn cb, void *user) {
    if (!archive || !cb) return PNA_E_INVAL;
    const uint8_t *a = (const uint8_t *)archive;
    if (!pna_image_header_ok(a, len)) return PNA_E_INVAL;
    size_t pos = 8, idx = 0, start = 0, name_off = 0, name_len = 0;
    int open = 0, kind = 0;                                                       // 1: inside FHED..FEND, 2: inside SHED..SEND
    for (;;) {
        PnaChunk ch;
        if (next_chunk(a, len, pos, ch)) return PNA_E_INVAL;
        const uint8_t *ty = ch.type;
        if (!open) {
            if (memcmp(ty, "AEND", 4) == 0) return PNA_OK;
            if (memcmp(ty, "FHED", 4) == 0) { if (ch.len < 6) return PNA_E_INVAL; open = 1; start = ch.off; kind = ch.data[2]; name_off = ch.off + 8 + 6; name_len = (size_t)ch.len - 6; }
            else if (memcmp(ty, "SHED", 4) == 0) { open = 2; start = ch.off; kind = -1; name_off = ch.off; name_len = 0; }
        } else if ((open == 1 && memcmp(ty, "FEND", 4) == 0) || (open == 2 && memcmp(ty, "SEND", 4) == 0)) {
            if (cb(user, idx++, (const char *)a + name_off, name_len, kind, start, pos - start) != 0) return PNA_E_SINK;
            open = 0;
        }
    }
}
