// pna_extract.cpp -- the read-side driver of libpna_gpu.so: `pna extract` / `pna verify` over archives in host memory.
#include "pna_ctx.h"
// ---------------------------------------------------------------------------------------------------------
// Read side driver: `pna extract` / `pna verify` for non-solid archives (cli/src/command/extract.rs:594-640, verify.rs:140-188;
// Archive::read_header + next_raw_item, lib/src/archive/read.rs:22-66; TryFrom<RawEntry>, lib/src/entry.rs:757-885; read_chunk with its
// mandatory CRC check, lib/src/io.rs:117-149; decrypt_reader / decompress_reader, lib/src/entry/read.rs:59-104,171-190).
// The chunk walk and the small chunks' CRCs are host work; the data chunks' CRC-32 (k_frame in verify mode), the gather of every
// entry's data pieces into one stream (k_gather), AES-CTR decryption and the zstd / deflate decoding run on the device.
// The name an entry is handed out under: EntryHeader::path() (lib/src/entry/header.rs:91-94,143-147) -- the FHED bytes must be UTF-8
// (InvalidData otherwise), and what callers see is the SANITISED form (EntryName::sanitize: no root, no "." / "..", so a crafted
// "../../etc/x" or "/abs" cannot leave the extraction directory).  The callback takes a C string, so an embedded NUL is rejected too.
static bool utf8_ok(const uint8_t *p, size_t n) {
    for (size_t i = 0; i < n;) {
        const uint8_t b = p[i];
        size_t k; uint32_t cp;
        if (b < 0x80) { i++; continue; }
        else if ((b & 0xE0) == 0xC0) { k = 1; cp = b & 0x1F; }
        else if ((b & 0xF0) == 0xE0) { k = 2; cp = b & 0x0F; }
        else if ((b & 0xF8) == 0xF0) { k = 3; cp = b & 0x07; }
        else return false;
        for (size_t j = 1; j <= k; j++) { if (i + j >= n || (p[i + j] & 0xC0) != 0x80) return false; cp = (cp << 6) | (p[i + j] & 0x3F); }
        if ((k == 1 && cp < 0x80) || (k == 2 && cp < 0x800) || (k == 3 && (cp < 0x10000 || cp > 0x10FFFF)) || (cp >= 0xD800 && cp <= 0xDFFF)) return false;
        i += k + 1;
    }
    return true;
}
static int entry_path(pna_gpu_ctx *c, const std::string &raw, std::string &out) {
    if (memchr(raw.data(), 0, raw.size())) return fail(c, PNA_E_INVAL, "entry name contains a NUL byte");
    if (!utf8_ok((const uint8_t *)raw.data(), raw.size())) return fail(c, PNA_E_INVAL, "entry name is not valid UTF-8");
    out = pna::pna_sanitize_name(raw.data(), raw.size());
    return PNA_OK;
}
namespace {
struct XPiece { uint64_t off; uint32_t len; };
// a data stream of the archive, a normal entry's (FDAT) or a solid entry's (SDAT), with what its header chunk says about it
struct XStream {
    int compression = 0, encryption = 0, cipher_mode = 0; std::string phsf;
    std::vector<XPiece> pieces; uint64_t stream_len = 0;
    uint64_t pk_off = 0, pay_len = 0;                          // payload (cipher prefix and tags stripped) in the packed buffer
    const char *htype = "FHED"; std::vector<uint8_t> hdr;      // the header chunk: a GCM stream key is bound to it (entry_context, lib/src/cipher/aead.rs:167-190)
    uint32_t gcm_seg = 0;                                      // GCM STREAM: segment size of the stream header
    uint8_t iv[16] = {0};                                      // CTR / CBC: the IV in front of the ciphertext
    uint64_t lo = 0, hi = 0;                                   // archive bytes [lo, hi) that hold the entry
    // verdict mode (`pna verify`): what the host found (a PNA_VERIFY_* status, 0 = nothing yet), the record's flags, its GCM segments [g0, g1) and
    // CBC padding unit in the window's verdict arrays
    int vst = 0; uint32_t vfl = 0, g0 = 0, g1 = 0, cbc_unit = 0xFFFFFFFFu;
};
struct XEntry : XStream {
    std::string name; int kind = 0;
    bool has_size = false; uint64_t raw_size = 0, raw_off = 0; // fSIZ; decoded bytes in the raw buffer
    bool noname = false, odd_size = false;                     // verdict mode: FHED unreadable (the record has no name); fSIZ out of proportion (decoded as without one)
    size_t d0 = 0, d1 = 0;                                     // its FDAT chunks in the descriptor list
    bool nodecode = false;                                     // `pna diff`: settled without its bytes (missing, type, size, not compared) -- its chunks' CRCs are checked, nothing is gathered or decoded
};
struct XSolid : XStream {                                      // SHED [PHSF] SDAT* SEND -- lib/src/entry.rs:465-484,567-583
    size_t order = 0;                                          // number of normal entries in front of it
    size_t s0 = 0, s1 = 0;                                     // its SDAT chunks in the descriptor list
};
struct Inner { std::string name; int kind; std::vector<XPiece> pieces; uint64_t len; bool has_size = false; uint64_t raw_size = 0; };     // an entry of a decoded solid stream (its fSIZ: `pna diff`)
// one call of the driver: the caller's arguments, the keys derived so far (one derivation per distinct PHSF string), the next entry's index
struct XCall {
    pna_gpu_ctx *c; const void *password; size_t password_len; pna_entry_fn cb; void *user;
    std::vector<std::pair<std::string, std::vector<uint8_t>>> keys; size_t index = 0;
    bool verdict = false, fast = false;                        // `pna verify` (pna_gpu_verify_archive_host): failures become records; --fast: chunk structure and CRCs only
    uint64_t kdf_runs = 0;                                     // key derivations of the call (one per distinct PHSF string that a stream needed)
    bool kdf_counted = false;                                  // option kdf_device: the context's batch counters were set to zero for this call
};
// a window's layout: packed payloads and decoded bytes, the gather of the data streams, the streams each cipher stage takes
struct XPlan {
    uint64_t pk_total = 0, raw_total = 0;
    std::vector<PlaceDescH> places; std::vector<XStream *> enc_list, gcm_list; std::vector<size_t> nosize_idx;
};
// what a window hands out, in archive order
struct XOut {
    std::vector<XEntry> ents; std::vector<size_t> solid_order; std::vector<std::vector<Inner>> inner; std::vector<std::vector<uint8_t>> plain, nosize_data;
    size_t index0 = 0;
};
// The archive as the driver reads it: one image, or the parts of a split archive laid end to end (part k at virtual offset vb[k]) and read in place --
// a chunk never crosses a part, so every chunk, data piece, IV and tag is contiguous in host memory; a window's span may take bytes from two parts.
struct ArcParts {
    const uint8_t *const *p; const size_t *len; size_t n; std::vector<uint64_t> vb;
    const uint8_t *at(uint64_t v) const { const size_t k = (size_t)(std::upper_bound(vb.begin(), vb.end(), v) - vb.begin()) - 1; return p[k] + (v - vb[k]); }
};
struct XRun { uint64_t dev, arc, len; };                       // a run of a sparse window (pna_gpu_extract_select_host): archive bytes [arc, arc + len) lie at window offset dev
struct WinSrc {                                                // a window's bytes: `a + o` is the byte at window offset o
    const ArcParts *ap; uint64_t base; const std::vector<XRun> *runs = nullptr;      // runs: the window holds these runs of the archive only, packed (base unused)
    const uint8_t *operator+(uint64_t o) const {
        if (!runs) return ap->at(base + o);
        const XRun &r = *(std::upper_bound(runs->begin(), runs->end(), o, [](uint64_t v, const XRun &q) { return v < q.dev; }) - 1);
        return ap->at(r.arc + (o - r.dev));
    }
};
uint32_t max_chunk_len(const std::vector<FrameDesc> &v) {      // the longest data chunk of a list (0: none below 16 380 bytes, the wave-per-chunk CRC kernel's limit)
    uint32_t m = 1;
    for (const FrameDesc &d : v) { if (d.payload_len > 16380u) return 0u; m = std::max(m, d.payload_len); }
    return m;
}
// bytes [lo, lo + n) of a data stream whose pieces lie in `a` (a prefix or a tag may span pieces: prepend_data_prefix makes the prefix a piece of its own)
void stream_read(const WinSrc &a, const std::vector<XPiece> &pieces, uint64_t lo, uint64_t n, uint8_t *out) {
    uint64_t at = 0;
    for (const XPiece &p : pieces) {
        if (!n) break;
        if (lo < at + p.len) { const uint64_t k = lo - at, m = std::min<uint64_t>(n, p.len - k); memcpy(out, a + p.off + k, m); out += m; lo += m; n -= m; }
        at += p.len;
    }
}
}

// A PHSF string as a key derivation job: "$argon2id$v=19$m=<KiB>,t=<passes>,p=<lanes>$<salt>" (argon2 0.5: Params::try_from(&PasswordHash),
// lib/src/hash.rs:56-70) or "$pbkdf2-sha256$i=<rounds>,l=<len>$<salt>" (derive_password_hash, lib/src/hash.rs:47-88).  *why: what the caller's error text says
static int phsf_parse(const std::string &phsf, pna_kdf_job &job, std::vector<uint8_t> &salt, const char **why) {
    auto bad = [&](int code, const char *what) { *why = what; return code; };
    int kind = -1; size_t p1 = 15, p2 = 0;                        // kind: the argon2 variant, -1 for pbkdf2-sha256
    uint32_t m = 19456, t = 2, lanes = 1, rounds = 600000;      // argon2 0.5 and pbkdf2 0.12 defaults
    if (phsf.rfind("$argon2", 0) == 0) {
        if (phsf.rfind("$argon2id$", 0) == 0) { kind = 2; p1 = 10; } else if (phsf.rfind("$argon2i$", 0) == 0) { kind = 1; p1 = 9; } else if (phsf.rfind("$argon2d$", 0) == 0) { kind = 0; p1 = 9; }
        if (kind < 0) return bad(PNA_E_INVAL, "malformed PHSF");
        if (phsf.compare(p1, 2, "v=") == 0) { const size_t q = phsf.find('$', p1); if (q == std::string::npos || strtoul(phsf.c_str() + p1 + 2, nullptr, 10) != 19) return bad(PNA_E_UNSUPPORTED, "argon2 version other than 0x13"); p1 = q + 1; }
        p2 = phsf.find('$', p1);
        if (p2 == std::string::npos) return bad(PNA_E_INVAL, "malformed PHSF");
        const std::string prm = phsf.substr(p1, p2 - p1);
        for (size_t q = 0; q < prm.size();) {
            const size_t e2 = prm.find(',', q); const std::string kv = prm.substr(q, e2 == std::string::npos ? std::string::npos : e2 - q);
            if (kv.size() > 2 && kv[1] == '=') {
                char *endp = nullptr; const unsigned long long v = strtoull(kv.c_str() + 2, &endp, 10);
                if (!endp || *endp || endp == kv.c_str() + 2) return bad(PNA_E_INVAL, "malformed argon2 parameter in PHSF");
                // the parameters come from an untrusted archive: refuse costs that only serve to stall / exhaust the host
                if ((kv[0] == 'm' && v > (4ull << 20)) || (kv[0] == 't' && v > 64) || (kv[0] == 'p' && v > 256)) return bad(PNA_E_UNSUPPORTED, "argon2 cost beyond the accepted maximum (m <= 4 GiB, t <= 64, p <= 256)");
                if (kv[0] == 'm') m = (uint32_t)v; else if (kv[0] == 't') t = (uint32_t)v; else if (kv[0] == 'p') lanes = (uint32_t)v;
            }
            if (e2 == std::string::npos) break; q = e2 + 1;
        }
    } else {
        if (phsf.rfind("$pbkdf2-sha256$", 0) != 0) return bad(PNA_E_UNSUPPORTED, "password hash other than argon2 / pbkdf2-sha256");
        p2 = phsf.find('$', p1);
        if (p2 == std::string::npos) return bad(PNA_E_INVAL, "malformed PHSF");
        const std::string prm = phsf.substr(p1, p2 - p1);
        const size_t ip = prm.find("i=");
        if (ip != std::string::npos) {
            char *endp = nullptr; const unsigned long long v = strtoull(prm.c_str() + ip + 2, &endp, 10);
            if (!endp || (*endp && *endp != ',') || v == 0) return bad(PNA_E_INVAL, "malformed pbkdf2 round count in PHSF");
            if (v > 10000000ull) return bad(PNA_E_UNSUPPORTED, "pbkdf2 round count beyond the accepted maximum (10 000 000)");
            rounds = (uint32_t)v;
        }
    }
    std::string sb = phsf.substr(p2 + 1); const size_t p3 = sb.find('$'); if (p3 != std::string::npos) sb.resize(p3);
    salt.clear();
    if (!b64_decode_nopad(sb, salt)) return bad(PNA_E_INVAL, "malformed PHSF");
    job = pna_kdf_job{kind >= 0 ? kind : PNA_KDF_PBKDF2_SHA256_JOB, t, m, lanes, rounds, salt.data(), salt.size()};
    return PNA_OK;
}
extern "C" int pna_phsf_parse(const char *phsf, size_t len, pna_kdf_job *job, uint8_t *salt_buf, size_t salt_cap, size_t *salt_len) {
    if ((!phsf && len) || !job || (!salt_buf && salt_cap)) return PNA_E_INVAL;
    std::vector<uint8_t> salt; const char *why = nullptr; pna_kdf_job j{};
    const int rc = phsf_parse(std::string(phsf ? phsf : "", len), j, salt, &why);
    if (rc) return rc;
    if (salt_len) *salt_len = salt.size();
    if (salt.size() > salt_cap) return PNA_E_DSTSIZE;
    if (!salt.empty()) memcpy(salt_buf, salt.data(), salt.size());
    j.salt = salt_buf; *job = j;
    return PNA_OK;
}
// The key of a PHSF string, derived once per call: the cache, or -- for a string that derive_ahead did not take -- one derivation on the host
static int phsf_key(XCall &x, const std::string &phsf, const uint8_t **out) {
    pna_gpu_ctx *c = x.c;
    for (auto &k : x.keys) if (k.first == phsf) { *out = k.second.data(); return PNA_OK; }
    pna_kdf_job j{}; std::vector<uint8_t> key(32), salt; const char *why = nullptr;
    int rc = phsf_parse(phsf, j, salt, &why);
    if (rc) return fail(c, rc, why);
    const bool argon = j.kind != PNA_KDF_PBKDF2_SHA256_JOB;
    rc = argon ? pna_kdf_argon2(j.kind, x.password, x.password_len, salt.data(), salt.size(), j.t_cost, j.m_cost_kib, j.lanes, key.data(), 32)
               : pna_kdf_pbkdf2_sha256(x.password, x.password_len, salt.data(), salt.size(), j.rounds, key.data(), 32, nullptr, 0);
    if (rc) return fail(c, rc, argon ? "key derivation failed (argon2 parameters)" : "key derivation failed");
    x.keys.emplace_back(phsf, std::move(key)); *out = x.keys.back().second.data(); x.kdf_runs++;
    return PNA_OK;
}
// Option kdf_device = N >= 1: the distinct PHSF strings that the streams of `need` will ask phsf_key for and that the call has not derived yet, as ONE
// batch of pna_gpu_kdf_batch's -- if there are at least N of them.  A string that does not parse, or a job the algorithm refuses, is left out of the
// cache: phsf_key meets it where its key is asked for and reports it as it always did.
static int derive_ahead(XCall &x, const std::vector<const XStream *> &need) {
    pna_gpu_ctx *c = x.c;
    if (c->tun.kdf_device < 1 || !kdf_batch || need.empty()) return PNA_OK;
    std::vector<const std::string *> todo; std::vector<pna_kdf_job> jobs; std::vector<std::vector<uint8_t>> salts;
    {
        std::vector<const std::string *> seen;
        for (auto &k : x.keys) seen.push_back(&k.first);
        auto less = [](const std::string *a, const std::string *b) { return *a < *b; };
        std::sort(seen.begin(), seen.end(), less);
        std::vector<const std::string *> cand;
        for (const XStream *s : need) cand.push_back(&s->phsf);
        std::stable_sort(cand.begin(), cand.end(), less);
        for (size_t i = 0; i < cand.size(); i++) {
            if (i && *cand[i] == *cand[i - 1]) continue;
            if (std::binary_search(seen.begin(), seen.end(), cand[i], less)) continue;
            pna_kdf_job j{}; std::vector<uint8_t> salt; const char *why = nullptr;
            if (phsf_parse(*cand[i], j, salt, &why)) continue;
            todo.push_back(cand[i]); jobs.push_back(j); salts.push_back(std::move(salt));
        }
    }
    if (todo.empty()) return PNA_OK;
    if (!x.kdf_counted) { c->kdf_dev_jobs = c->kdf_host_jobs = c->kdf_rounds = 0; c->kdf_ms = 0; x.kdf_counted = true; }      // pna_gpu_debug_kdf_stats: the batches of this call
    if (todo.size() < (size_t)c->tun.kdf_device) return PNA_OK;     // below the threshold: phsf_key derives them on the host
    for (size_t i = 0; i < jobs.size(); i++) jobs[i].salt = salts[i].data();
    std::vector<uint8_t> keys(32 * jobs.size()); std::vector<int> status(jobs.size(), PNA_OK);
    const int rc = kdf_batch(c, x.password, x.password_len, jobs.size(), jobs.data(), keys.data(), status.data(), c->stream, true);
    if (rc) return rc;
    for (size_t i = 0; i < jobs.size(); i++) {
        if (status[i]) continue;
        x.keys.emplace_back(*todo[i], std::vector<uint8_t>(keys.begin() + 32 * i, keys.begin() + 32 * i + 32)); x.kdf_runs++;
    }
    return PNA_OK;
}
// ... for the streams a window's cipher stages will take (every mode but verdict, where plan_window has derived them already)
static int derive_ahead_plan(XCall &x, const std::vector<XStream *> &enc_list, const std::vector<XStream *> &gcm_list) {
    std::vector<const XStream *> need(enc_list.begin(), enc_list.end());
    need.insert(need.end(), gcm_list.begin(), gcm_list.end());
    return derive_ahead(x, need);
}

// ---- 1. the chunk walk (host): structure, small-chunk CRCs, data-chunk descriptors.  Verdict mode (`pna verify`, x.verdict) goes on after damage:
// a chunk that fails its CRC is consumed (its length field trusted, as io::read_chunk does) and marks the entry that holds it BAD_CRC -- a bad FHED, or
// damage between entries, opens a KIND_BROKEN record that runs to the next FEND / SEND --; structural faults mark their entry; the parts of a split
// archive are walked one after the other (ANXT: the next part, its signature and AHED).  Where the walk cannot go on (a truncated chunk, no AEND)
// *broken is set and what was complete before the break is kept.  `multipart` (pna_gpu_extract_select_host): the strict walk over the parts of a split
// archive -- a missing part or a part without its signature fails the call.
static int walk_archive(pna_gpu_ctx *c, const ArcParts &ap, bool verdict, std::vector<XEntry> &ents, std::vector<FrameDesc> &dchunks,
                        std::vector<FrameDesc> &schunks, std::vector<XSolid> &solids, bool *broken, bool multipart = false) {
    XSolid scur; bool in_solid = false;
    XEntry cur; bool in_entry = false, ended = false;
    auto mark = [](XStream &s, int st) { if (!s.vst) s.vst = st; };
    auto close_entry = [&](uint64_t hi) { cur.d1 = dchunks.size(); cur.hi = hi; ents.push_back(std::move(cur)); in_entry = false; };
    auto close_solid = [&](uint64_t hi) { scur.s1 = schunks.size(); scur.hi = hi; solids.push_back(std::move(scur)); in_solid = false; };
    auto open_broken = [&](uint64_t off, int st) { cur = XEntry(); in_entry = true; cur.d0 = dchunks.size(); cur.lo = off; cur.kind = PNA_VERIFY_KIND_BROKEN; cur.noname = true; cur.vst = st; };
    // verdict mode: a record still open where a new header (or AEND) stands ends there -- it, not what follows, is marked (it lost its FEND / SEND)
    auto close_open = [&](uint64_t off) {
        if (in_entry) { mark(cur, PNA_VERIFY_BAD_STRUCTURE); close_entry(off); }
        if (in_solid) { mark(scur, PNA_VERIFY_BAD_STRUCTURE); close_solid(off); }
    };
    for (size_t part = 0; part < ap.n && !ended; part++) {
        const uint8_t *a = ap.p[part]; const size_t archive_len = ap.len[part]; const uint64_t vb = ap.vb[part];
        if (part > 0 && (archive_len < 8 || memcmp(a, PNA_SIGNATURE, 8) != 0)) { if (!verdict) return fail(c, PNA_E_INVAL, "a part is not a PNA archive"); *broken = true; return PNA_OK; }
        bool seen_ahed = false, next_part = false;
        size_t pos = 8;
        while (pos < archive_len) {
            PnaChunk ch;
            const int r = next_chunk(a, archive_len, pos, ch);          // (pos moves behind the chunk)
            if (r && verdict) { *broken = true; return PNA_OK; }
            if (r) return fail(c, PNA_E_INVAL, r == CHUNK_SHORT_HEADER ? "truncated chunk header" : "truncated chunk body");
            const uint64_t off = vb + ch.off;                              // the chunk's position in the parts laid end to end
            const bool is_fdat = memcmp(ch.type, "FDAT", 4) == 0, is_sdat = memcmp(ch.type, "SDAT", 4) == 0;
            const bool is_fend = memcmp(ch.type, "FEND", 4) == 0, is_send = memcmp(ch.type, "SEND", 4) == 0;
            const bool is_head = memcmp(ch.type, "FHED", 4) == 0 || memcmp(ch.type, "SHED", 4) == 0;
            const bool ends_broken = in_entry && cur.kind == PNA_VERIFY_KIND_BROKEN && (is_fend || is_send);   // (verdict mode only: kind is a byte otherwise)
            if (is_fdat || is_sdat) {
                if (ch.len > 0xFFFFFFFBu) {
                    if (!verdict) return fail(c, PNA_E_INVAL, "data chunk too long");
                    if (in_solid) mark(scur, PNA_VERIFY_BAD_STRUCTURE); else if (in_entry) mark(cur, PNA_VERIFY_BAD_STRUCTURE);
                    continue;
                }
                if (verdict && !in_entry && !in_solid && seen_ahed) open_broken(off, PNA_VERIFY_BAD_STRUCTURE);     // a data chunk of no entry
                (is_fdat ? dchunks : schunks).push_back(FrameDesc{off, ch.len, 0, 8, 0});
            }
            else if (!chunk_crc_ok(ch)) {
                if (!verdict) return fail(c, PNA_E_INVAL, "chunk CRC mismatch");
                if (!seen_ahed || memcmp(ch.type, "AEND", 4) == 0 || memcmp(ch.type, "ANXT", 4) == 0) { *broken = true; return PNA_OK; }
                if (is_head) { close_open(off); open_broken(off, PNA_VERIFY_BAD_CRC); }     // an unreadable header: its chunks up to the next FEND / SEND
                else if (in_solid) { mark(scur, PNA_VERIFY_BAD_CRC); if (is_send) close_solid(off + 12 + ch.len); }
                else if (in_entry) { mark(cur, PNA_VERIFY_BAD_CRC); if (is_fend || ends_broken) close_entry(off + 12 + ch.len); }
                else if (!is_fend && !is_send) open_broken(off, PNA_VERIFY_BAD_CRC);      // a damaged chunk between entries
                continue;
            }
            if (verdict && in_solid && memcmp(ch.type, "FHED", 4) == 0) close_open(off);     // a solid entry that lost its SEND ends at the next header
            if (!seen_ahed) {
                if (memcmp(ch.type, "AHED", 4) != 0 || ch.len != 8 || ch.data[0] != 0) {
                    if (verdict) { *broken = true; return PNA_OK; }
                    return fail(c, PNA_E_INVAL, "first chunk must be AHED (major version 0)");
                }
                seen_ahed = true;
            } else if (memcmp(ch.type, "AEND", 4) == 0) { if (verdict) close_open(off); ended = true; break; }
            else if (memcmp(ch.type, "ANXT", 4) == 0) {
                if (!verdict && !multipart) return fail(c, PNA_E_UNSUPPORTED, "multipart archives are not read by this driver");
                if (part + 1 == ap.n) { if (!verdict) return fail(c, PNA_E_INVAL, "the archive goes on in a part that was not given"); *broken = true; return PNA_OK; }
                next_part = true; break;
            }
            else if (memcmp(ch.type, "SHED", 4) == 0) {
                const bool bad = ch.len != 5 || ch.data[0] != 0 || ch.data[1] != 0;
                if ((bad || in_entry || in_solid) && !verdict) return fail(c, PNA_E_INVAL, "bad solid header");
                close_open(off);                                              // (verdict mode: a record without FEND / SEND ends here)
                scur = XSolid(); in_solid = true; scur.order = ents.size(); scur.s0 = schunks.size(); scur.lo = off;
                if (ch.len >= 5) { scur.compression = ch.data[2]; scur.encryption = ch.data[3]; scur.cipher_mode = ch.data[4]; }
                scur.htype = "SHED"; scur.hdr.assign(ch.data, ch.data + ch.len);
                if (bad) scur.vst = PNA_VERIFY_BAD_STRUCTURE;
            } else if (in_solid) {
                if (is_sdat) { scur.pieces.push_back(XPiece{off + 8, ch.len}); scur.stream_len += ch.len; }
                else if (memcmp(ch.type, "PHSF", 4) == 0) scur.phsf.assign((const char *)ch.data, ch.len);
                else if (is_send) close_solid(off + 12);
                else if (!(ch.type[0] & 0x20)) { if (!verdict) return fail(c, PNA_E_INVAL, "unknown critical chunk in a solid entry"); mark(scur, PNA_VERIFY_BAD_STRUCTURE); }
            }
            else if (memcmp(ch.type, "FHED", 4) == 0) {
                const bool bad = ch.len < 6 || ch.data[0] != 0 || ch.data[1] != 0;
                if ((bad || in_entry) && !verdict) return fail(c, PNA_E_INVAL, "bad entry header");
                close_open(off);
                cur = XEntry(); in_entry = true; cur.d0 = dchunks.size(); cur.lo = off;
                if (ch.len >= 6) {
                    cur.kind = ch.data[2]; cur.compression = ch.data[3]; cur.encryption = ch.data[4]; cur.cipher_mode = ch.data[5];
                    cur.name.assign((const char *)ch.data + 6, ch.len - 6);
                } else cur.noname = true;
                cur.hdr.assign(ch.data, ch.data + ch.len);
                if (bad) cur.vst = PNA_VERIFY_BAD_STRUCTURE;
            } else if (!in_entry) {
                if (!(ch.type[0] & 0x20)) {
                    if (!verdict) return fail(c, PNA_E_INVAL, "unknown critical chunk between entries");
                    if (!is_fend && !is_send) open_broken(off, PNA_VERIFY_BAD_STRUCTURE);
                }
            }
            else if (is_fdat) { cur.pieces.push_back(XPiece{off + 8, ch.len}); cur.stream_len += ch.len; }
            else if (memcmp(ch.type, "fSIZ", 4) == 0) {
                if (ch.len > 8) { if (!verdict) return fail(c, PNA_E_UNSUPPORTED, "entry beyond 2^64 bytes"); mark(cur, PNA_VERIFY_UNSUPPORTED); continue; }
                cur.has_size = true; cur.raw_size = 0; for (uint32_t i = 0; i < ch.len; i++) cur.raw_size = (cur.raw_size << 8) | ch.data[i];
            }
            else if (memcmp(ch.type, "PHSF", 4) == 0) cur.phsf.assign((const char *)ch.data, ch.len);
            else if (is_fend || ends_broken) close_entry(off + 12);
            else if (!(ch.type[0] & 0x20)) { if (!verdict) return fail(c, PNA_E_INVAL, "unknown critical chunk"); mark(cur, PNA_VERIFY_BAD_STRUCTURE); }   // chunk/types.rs: bit 5 of byte 0 clear = critical
        }
        if (!next_part) break;
    }
    if (!ended || in_entry || in_solid) {
        if (verdict) { *broken = true; return PNA_OK; }
        return fail(c, PNA_E_INVAL, "archive not terminated by AEND");
    }
    return PNA_OK;
}
// the streams of a window and their data chunks, moved to offsets relative to the window's first byte `base`
template <class S>
static void rebase(std::vector<S> &streams, const std::vector<FrameDesc> &all, size_t c0, size_t c1, std::vector<FrameDesc> &chunks, uint64_t base) {
    chunks.assign(all.begin() + c0, all.begin() + c1);
    for (auto &f : chunks) f.arc_off -= base;
    for (auto &s : streams) for (auto &p : s.pieces) p.off -= base;
}

// what a window leaves behind for later: `issue` starts the D2H copy of its decoded entries (called by the NEXT window once its own bytes
// are on the device, so the copy runs next to that window's kernels), `deliver` waits for it and hands the entries out
struct XDeferred { std::function<int()> issue, deliver; bool issued = false; explicit operator bool() const { return (bool)deliver; } };
// A data stream (the concatenated FDAT / SDAT bodies) is laid into the packed buffer at pk_off with its cipher prefix stripped: CTR / CBC lose the
// IV, a GCM STREAM its header and the segments' tags (only the ciphertext is gathered).  Sets pay_len (and gcm_seg) and registers the stream
// with the cipher stage.
static int plan_stream(XCall &x, const WinSrc &a, XStream &s, XPlan &P) {
    pna_gpu_ctx *c = x.c;
    s.pk_off = P.pk_total;
    // verdict mode: a stream this stage cannot take becomes its record's status (the pieces it placed so far are taken back) instead of the call's error
    const size_t places0 = P.places.size();
    auto fail = [&](pna_gpu_ctx *cc, int code, const char *what) {
        if (!x.verdict) return ::fail(cc, code, what);
        P.places.resize(places0);
        s.vst = code == PNA_E_UNSUPPORTED ? PNA_VERIFY_UNSUPPORTED : (s.cipher_mode == PNA_MODE_GCM ? PNA_VERIFY_BAD_STRUCTURE : PNA_VERIFY_BAD_DECRYPT);
        return PNA_OK;
    };
    if (x.verdict && s.encryption != PNA_ENC_NONE) {
        if (s.encryption != PNA_ENC_AES && !(s.encryption == PNA_ENC_CAMELLIA && camellia_on(c))) { s.vst = PNA_VERIFY_UNSUPPORTED; return PNA_OK; }
        if (!x.password) { s.vst = PNA_VERIFY_SKIPPED; return PNA_OK; }
        if (s.phsf.empty()) { s.vst = PNA_VERIFY_BAD_STRUCTURE; return PNA_OK; }
        const uint8_t *k = nullptr;                                   // derived here, once per PHSF string: a PHSF the reader cannot use is this record's fault
        const int rk = phsf_key(x, s.phsf, &k);
        if (rk == PNA_E_UNSUPPORTED) { s.vst = PNA_VERIFY_UNSUPPORTED; return PNA_OK; }
        if (rk == PNA_E_INVAL) { s.vst = PNA_VERIFY_BAD_STRUCTURE; return PNA_OK; }
        if (rk) return rk;
    }
    auto place = [&](uint64_t lo, uint64_t hi, uint64_t dst) {
        uint64_t at = 0;
        for (const XPiece &p : s.pieces) {
            const uint64_t s0 = std::max<uint64_t>(lo, at), s1 = std::min<uint64_t>(hi, at + p.len);
            for (uint64_t k = s0; k < s1; k += (1u << 20)) P.places.push_back(PlaceDescH{p.off + (k - at), dst + (k - lo), (uint32_t)std::min<uint64_t>(1u << 20, s1 - k), 0});
            at += p.len;
        }
    };
    if (s.encryption == PNA_ENC_NONE) { s.pay_len = s.stream_len; place(0, s.stream_len, s.pk_off); }
    else {
        if (s.encryption != PNA_ENC_AES && !(s.encryption == PNA_ENC_CAMELLIA && camellia_on(c))) return fail(c, PNA_E_UNSUPPORTED, "only AES entries are decrypted by this driver");
        if (!x.password) return fail(c, PNA_E_INVAL, "encrypted entry and no password");
        if (s.phsf.empty()) return fail(c, PNA_E_INVAL, "`PHSF` chunk not found");
        if (s.cipher_mode == PNA_MODE_CTR || s.cipher_mode == PNA_MODE_CBC) {
            if (s.stream_len < 16) return fail(c, PNA_E_INVAL, "data stream shorter than the IV");
            stream_read(a, s.pieces, 0, 16, s.iv);
            s.pay_len = s.stream_len - 16;
            place(16, s.stream_len, s.pk_off);
            P.enc_list.push_back(&s);
            s.vfl |= PNA_VERIFY_UNAUTHENTICATED;                       // (read only in verdict mode)
        } else if (s.cipher_mode == PNA_MODE_GCM) {
            // stream header, then segments of (segment size + 16-byte tag), the last one shorter: only the ciphertext is gathered
            if (s.stream_len < 75 + 16) return fail(c, PNA_E_INVAL, "datastream shorter than the stream header");
            uint8_t seg[4]; stream_read(a, s.pieces, 39, 4, seg);
            s.gcm_seg = rd_be32(seg);
            if (s.gcm_seg == 0 || s.gcm_seg > (64u << 20)) return fail(c, PNA_E_INVAL, "GCM segment size out of range");
            uint64_t rest = s.stream_len - 75, at = 75, outp = s.pk_off;
            while (rest) {
                const uint64_t segl = std::min<uint64_t>(rest, (uint64_t)s.gcm_seg + 16);
                if (segl < 16) return fail(c, PNA_E_INVAL, "GCM segment shorter than a tag");
                if (x.verdict && segl != rest && segl != (uint64_t)s.gcm_seg + 16) return fail(c, PNA_E_INVAL, "GCM STREAM: short non-final segment");
                place(at, at + segl - 16, outp);
                outp += segl - 16; at += segl; rest -= segl;
            }
            s.pay_len = outp - s.pk_off;
            P.gcm_list.push_back(&s);
        } else return fail(c, PNA_E_UNSUPPORTED, "unknown cipher mode");
        if (s.vst) return PNA_OK;
    }
    P.pk_total = (P.pk_total + s.pay_len + 15) & ~(uint64_t)15;
    return PNA_OK;
}
static bool decoded_here(int compression) {
    return compression == PNA_ALGO_STORE || compression == PNA_ALGO_ZSTD || compression == PNA_ALGO_DEFLATE || (compression == PNA_ALGO_XZ && xz_kernels_present());
}
// the window plan: packed payloads, decoded entries, the gather, the cipher stages' stream lists, the entries without fSIZ
static int plan_window(XCall &x, const WinSrc &a, std::vector<XEntry> &ents, std::vector<XSolid> &solids, XPlan &P) {
    pna_gpu_ctx *c = x.c;
    if (x.fast) return PNA_OK;                                        // verify --fast: chunk structure and CRCs, nothing gathered, decrypted or decoded
    if (x.verdict && x.password) {                                    // plan_stream asks for every encrypted stream's key: those it will ask for, derived as one batch (option kdf_device)
        std::vector<const XStream *> need;
        auto want = [&](const XStream &s) {
            if (s.vst || !decoded_here(s.compression) || s.encryption == PNA_ENC_NONE || s.phsf.empty()) return;
            if (s.encryption == PNA_ENC_AES || (s.encryption == PNA_ENC_CAMELLIA && camellia_on(c))) need.push_back(&s);
        };
        for (const XEntry &e : ents) if (!e.nodecode) want(e);
        for (const XSolid &so : solids) want(so);
        const int r = derive_ahead(x, need); if (r) return r;
    }
    for (size_t i = 0; i < ents.size(); i++) {
        XEntry &e = ents[i];
        if (x.verdict && (e.vst || e.nodecode)) continue;              // (a structural fault found by the walk, or `pna diff` needs no byte of it: nothing to decode)
        if (!decoded_here(e.compression)) { if (x.verdict) { e.vst = PNA_VERIFY_UNSUPPORTED; continue; } return fail(c, PNA_E_UNSUPPORTED, "compression method not decoded on the device (xz)"); }
        const int r = plan_stream(x, a, e, P); if (r) return r;
        if (e.vst) continue;
        if (e.compression == PNA_ALGO_STORE) continue;
        // verdict mode: an fSIZ no payload of this length can decode to is a wrong size hint -- the entry is decoded as one without fSIZ
        if (x.verdict && e.has_size && (e.raw_size > (1ull << 40) || e.raw_size / 65536 > e.pay_len + 1)) e.odd_size = true;
        if (e.odd_size) { P.nosize_idx.push_back(i); continue; }
        // fSIZ is optional (older writers omit it): the payload is then decoded like a solid stream, its size found by the decoder
        if (!e.has_size) { P.nosize_idx.push_back(i); continue; }
        // fSIZ comes from the archive: a size no payload of this length can decode to (deflate tops out at 1032 : 1, zstd at a few
        // thousand : 1 through RLE blocks) is damage, not a reason to ask the device for exabytes
        if (e.raw_size > (1ull << 40) || e.raw_size / 65536 > e.pay_len + 1) return fail(c, PNA_E_INVAL, "fSIZ is out of proportion to the entry's data");
        e.raw_off = P.raw_total; P.raw_total = (P.raw_total + e.raw_size + 15) & ~(uint64_t)15;
        if (P.raw_total > (1ull << 42)) return fail(c, PNA_E_NOMEM, "archive decodes to more than this driver takes in one call");
    }
    for (XSolid &so : solids) {
        if (x.verdict && so.vst) continue;
        if (!decoded_here(so.compression)) { if (x.verdict) { so.vst = PNA_VERIFY_UNSUPPORTED; continue; } return fail(c, PNA_E_UNSUPPORTED, "solid stream: compression method not decoded on the device (xz)"); }
        const int r = plan_stream(x, a, so, P); if (r) return r;
    }
    return PNA_OK;
}
static void verify_chunks(pna_gpu_ctx *c, const DevBuf &desc, const std::vector<FrameDesc> &v, const DevBuf &buf, const char *ty, hipStream_t st) {
    launch_frame_verify((const FrameDesc *)desc.p, (uint32_t)v.size(), (const CrcTabs *)c->crc_tabs.p, (const uint8_t *)buf.p, (uint64_t)buf.cap & ~(uint64_t)15,
                        ty, (uint32_t *)c->x_flag.p, st, max_chunk_len(v));
}
static const uint32_t flag0[2] = {0u, 0xFFFFFFFFu};
static int read_back(pna_gpu_ctx *c, void *dst, const void *src, size_t n, hipStream_t st) {      // a result of the kernels to the host, the stream drained
    HIPCHK(c, hipMemcpyAsync(dst, src, n, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(st));
    return PNA_OK;
}
// ---- 3. device: the window's bytes in, the data chunks' CRCs, the gather of the data streams into the packed buffer
// Verdict mode (`pna verify`): one CRC verdict word per data chunk into c->v_crc (a window holds FDAT or SDAT chunks, never both) instead of the shared
// flag, and nothing is decoded into the raw buffer's host side.  The window's bytes come from one part, or from two where it spans a part's end.
static int upload_window(pna_gpu_ctx *c, const WinSrc &a, size_t archive_len, const std::vector<FrameDesc> &dchunks, const std::vector<FrameDesc> &schunks,
                         const XPlan &P, int slot, uint32_t flag[2], hipStream_t st, bool verdict = false) {
    int rc = ensure_crc(c); if (rc) return rc;
    if (c->x_arc.ensure(archive_len + 64) || c->x_pk.ensure(P.pk_total + 8192) || c->x_raw[slot].ensure(P.raw_total + 64) || c->x_flag.ensure(64) ||
        c->x_desc.ensure(dchunks.size() * sizeof(FrameDesc) + 16) || c->x_place.ensure(P.places.size() * sizeof(PlaceDescH) + 16) ||
        (verdict && c->v_crc.ensure((dchunks.size() + schunks.size()) * 4 + 16))) return fail(c, PNA_E_NOMEM, "extract workspace");
    auto copy_in = [&](uint64_t arc, uint64_t n, uint64_t dev) -> int {      // archive bytes [arc, arc + n) to window offset dev, from the parts that hold them
        for (size_t k = 0; k < a.ap->n; k++) {
            const uint64_t p0 = a.ap->vb[k], p1 = p0 + a.ap->len[k], lo = std::max<uint64_t>(p0, arc), hi = std::min<uint64_t>(p1, arc + n);
            if (lo < hi) HIPCHK(c, hipMemcpyAsync((uint8_t *)c->x_arc.p + dev + (lo - arc), a.ap->p[k] + (lo - p0), hi - lo, hipMemcpyHostToDevice, st));
        }
        c->xs_uploaded += n;
        return PNA_OK;
    };
    if (a.runs) { for (const XRun &r : *a.runs) { rc = copy_in(r.arc, r.len, r.dev); if (rc) return rc; } }      // a sparse window: its runs, one copy each
    else { rc = copy_in(a.base, archive_len, 0); if (rc) return rc; }
    HIPCHK(c, hipMemcpyAsync(c->x_flag.p, flag0, 8, hipMemcpyHostToDevice, st));
    auto check = [&](const DevBuf &desc, const std::vector<FrameDesc> &v, const char *ty) {
        if (verdict) launch_frame_verdict((const FrameDesc *)desc.p, (uint32_t)v.size(), (const CrcTabs *)c->crc_tabs.p, (const uint8_t *)c->x_arc.p,
                                          (uint64_t)c->x_arc.cap & ~(uint64_t)15, ty, (uint32_t *)c->v_crc.p, st, max_chunk_len(v));
        else verify_chunks(c, desc, v, c->x_arc, ty, st);
    };
    if (!dchunks.empty()) {
        HIPCHK(c, hipMemcpyAsync(c->x_desc.p, dchunks.data(), dchunks.size() * sizeof(FrameDesc), hipMemcpyHostToDevice, st));
        check(c->x_desc, dchunks, "FDAT");
    }
    if (!schunks.empty()) {
        if (c->solid_desc.ensure(schunks.size() * sizeof(FrameDesc) + 16)) return fail(c, PNA_E_NOMEM, "extract workspace");
        HIPCHK(c, hipMemcpyAsync(c->solid_desc.p, schunks.data(), schunks.size() * sizeof(FrameDesc), hipMemcpyHostToDevice, st));
        check(c->solid_desc, schunks, "SDAT");
    }
    if (!P.places.empty()) {
        HIPCHK(c, hipMemcpyAsync(c->x_place.p, P.places.data(), P.places.size() * sizeof(PlaceDescH), hipMemcpyHostToDevice, st));
        launch_gather(c->x_place.p, (uint32_t)P.places.size(), (const uint8_t *)c->x_arc.p, (uint8_t *)c->x_pk.p, st);
    }
    return read_back(c, flag, c->x_flag.p, 8, st);
}
// CBC of one key group (DecryptCbcAes256Reader, lib/src/entry/read.rs:77-82): a block's plaintext needs its own and the previous ciphertext block
// only, so a long stream -- a solid one -- is cut into units of 16 MiB whose IV is the ciphertext block in front; the padding is read at the end of
// the stream's last unit
// Verdict mode (`verdict`): a bad length marks its stream, the padding's verdict stays on the device for k_verdict (CBC units from unit0 on: the
// window's CBC groups share x_plen), and no stream fails the call.
static constexpr uint64_t CBC_UNIT = 16u << 20;
static int decrypt_cbc(pna_gpu_ctx *c, int encryption, const uint8_t *key, const std::vector<XStream *> &grp_in, hipStream_t st, bool verdict = false, uint32_t *unit0 = nullptr) {
    std::vector<XStream *> grp;
    for (XStream *s : grp_in) { if (verdict && (s->pay_len == 0 || (s->pay_len & 15))) s->vst = PNA_VERIFY_BAD_DECRYPT; else grp.push_back(s); }
    if (grp.empty()) return PNA_OK;
    const uint32_t u0 = unit0 ? *unit0 : 0u;
    std::vector<CipherUnit> units; std::vector<size_t> last_unit(grp.size());
    for (size_t q = 0; q < grp.size(); q++) {
        const XStream &s = *grp[q];
        if (s.pay_len == 0 || (s.pay_len & 15)) return fail(c, PNA_E_INVAL, "CBC: bad length or padding (wrong password or damaged data)");
        for (uint64_t o = 0; o < s.pay_len; o += CBC_UNIT) {
            units.push_back(CipherUnit{s.pk_off + o, 0, (uint32_t)std::min<uint64_t>(CBC_UNIT, s.pay_len - o), (uint32_t)units.size()});
            last_unit[q] = units.size() - 1;
        }
    }
    if (c->ci_units.ensure(units.size() * sizeof(CipherUnit) + 16) || c->ci_ivs.ensure(units.size() * 16 + 16) || c->x_plen.ensure((u0 + units.size()) * 4 + 16)) return fail(c, PNA_E_NOMEM, "cipher workspace");
    // the units' IVs: the stream's own for its first unit, else the 16 ciphertext bytes in front of the unit (copied on the device BEFORE the
    // kernel overwrites them: the decryption is in place)
    { size_t u = 0;
      for (const XStream *e : grp)
          for (uint64_t o = 0; o < e->pay_len; o += CBC_UNIT, u++) {
              if (o == 0) HIPCHK(c, hipMemcpyAsync((uint8_t *)c->ci_ivs.p + 16 * u, e->iv, 16, hipMemcpyHostToDevice, st));
              else HIPCHK(c, hipMemcpyAsync((uint8_t *)c->ci_ivs.p + 16 * u, (const uint8_t *)c->x_pk.p + e->pk_off + o - 16, 16, hipMemcpyDeviceToDevice, st));
          } }
    std::vector<uint32_t> plen(units.size());
    HIPCHK(c, hipMemcpyAsync(c->ci_units.p, units.data(), units.size() * sizeof(CipherUnit), hipMemcpyHostToDevice, st));
    BlockKey ek; ek.expand(encryption, key);
    int rc = cipher_cbc_dec(c, (const CipherUnit *)c->ci_units.p, (uint32_t)units.size(), (const uint8_t *)c->ci_ivs.p, (uint8_t *)c->x_pk.p, ek.dec(), (uint32_t *)c->x_plen.p + u0, st);
    if (rc) return rc;
    rc = read_back(c, plen.data(), (uint32_t *)c->x_plen.p + u0, units.size() * 4, st); if (rc) return rc;
    if (unit0) *unit0 += (uint32_t)units.size();
    for (size_t q = 0; q < grp.size(); q++) {
        const uint32_t pl = plen[last_unit[q]];
        if (verdict) { grp[q]->cbc_unit = u0 + (uint32_t)last_unit[q]; if (pl == 0xFFFFFFFFu) continue; }     // (k_verdict reads the padding's verdict)
        if (pl == 0xFFFFFFFFu) return fail(c, PNA_E_INVAL, "CBC: bad length or padding (wrong password or damaged data)");
        grp[q]->pay_len = (grp[q]->pay_len - 1) / CBC_UNIT * CBC_UNIT + pl;
    }
    return PNA_OK;
}
// CTR and CBC, in place in the packed buffer: streams sharing a PHSF string and a mode share the key, one cipher call per group
static int decrypt_ctr_cbc(XCall &x, const std::vector<XStream *> &enc_list, hipStream_t st) {
    pna_gpu_ctx *c = x.c;
    std::vector<bool> done(enc_list.size(), false);
    uint32_t cbc_units = 0;                                           // verdict mode: the window's CBC units, one x_plen word each
    if (x.verdict) {                                                  // ... sized once for the window: the groups' verdicts stay side by side until k_verdict reads them
        uint64_t all = 0;
        for (const XStream *s : enc_list) if (s->cipher_mode == PNA_MODE_CBC) all += (s->pay_len + CBC_UNIT - 1) / CBC_UNIT;
        if (c->x_plen.ensure(all * 4 + 16)) return fail(c, PNA_E_NOMEM, "cipher workspace");
    }
    for (size_t j = 0; j < enc_list.size(); j++) {
        if (done[j]) continue;
        const XStream &s0 = *enc_list[j];
        const uint8_t *key = nullptr;
        int rc = phsf_key(x, s0.phsf, &key); if (rc) return rc;
        std::vector<XStream *> grp;
        for (size_t k = j; k < enc_list.size(); k++)
            if (!done[k] && enc_list[k]->phsf == s0.phsf && enc_list[k]->cipher_mode == s0.cipher_mode && enc_list[k]->encryption == s0.encryption) { done[k] = true; grp.push_back(enc_list[k]); }
        if (s0.cipher_mode == PNA_MODE_CTR) {
            std::vector<uint64_t> off, len; std::vector<uint8_t> ivs;
            for (const XStream *e : grp) { off.push_back(e->pk_off); len.push_back(e->pay_len); ivs.insert(ivs.end(), e->iv, e->iv + 16); }
            pna_gpu_cipher ci{}; ci.encryption = s0.encryption; ci.cipher_mode = PNA_MODE_CTR; memcpy(ci.key, key, 32); ci.phsf = ""; ci.ivs = ivs.data();
            rc = pna_gpu_cipher_apply_device(c, &ci, 1, off.size(), c->x_pk.p, off.data(), len.data(), st);
        } else rc = decrypt_cbc(c, s0.encryption, key, grp, st, x.verdict, x.verdict ? &cbc_units : nullptr);
        if (rc) return rc;
    }
    return PNA_OK;
}
// GCM STREAM (decrypt_reader, (_, CipherMode::GCM): lib/src/entry/read.rs:105-140): key confirmation first -- a wrong password is told apart from
// tampering --, then every segment's tag (k_gcm_tag in verify mode), then the CTR keystream with the stream keys
// Verdict mode: a failed key confirmation marks its stream BAD_AUTH, every segment's tag verdict goes to c->v_seg (the stream's segments [g0, g1))
// for k_verdict, and the keystream is applied to every segment all the same (a record that failed is not decoded).
static int decrypt_gcm(XCall &x, const WinSrc &a, const std::vector<XStream *> &gcm_list, uint32_t flag[2], hipStream_t st) {
    pna_gpu_ctx *c = x.c;
    int rc;
    // a window may hold AES and Camellia streams together: one segment list (tags, IVs, verdict words, keys), one unit list that the key list sorts by
    // cipher for cipher_ctr
    std::vector<GcmEntry> gents; std::vector<uint8_t> tags, giv; SegKeys gkeys; std::vector<CipherUnit> units;
    for (XStream *e : gcm_list) {
        XStream &s = *e;
        const uint8_t *km = nullptr;
        rc = phsf_key(x, s.phsf, &km); if (rc) return rc;
        GcmMaterial m; stream_read(a, s.pieces, 0, 75, m.header);
        const GcmCallKeys ck = gcm_call_keys(km, s.phsf.data(), s.phsf.size());
        { uint8_t diff = 0; for (int b = 0; b < 32; b++) diff |= (uint8_t)(ck.kc[b] ^ m.header[43 + b]);      // constant time, like the reference's ct_eq
          if (diff && x.verdict) { s.vst = PNA_VERIFY_BAD_AUTH; continue; }
          if (diff) return fail(c, PNA_E_INVAL, "GCM STREAM: key confirmation failed (wrong password)"); }
        s.g0 = (uint32_t)gents.size();
        gcm_stream_key(km, m.header, s.htype, s.hdr, ck.phsf_hash, s.encryption, m);
        uint64_t rest = s.stream_len - 75, at = 75, outp = s.pk_off; uint32_t counter = 0;
        while (rest) {
            const uint64_t segl = std::min<uint64_t>(rest, (uint64_t)s.gcm_seg + 16), ctl = segl - 16;
            const bool fin = segl == rest;
            GcmEntry ge{outp, (uint32_t)ctl, 0, {0, 0, 0, 0}, {0, 0, 0, 0}};
            uint8_t iv[16], tag[16];
            gcm_segment(m, counter, fin, ge, iv);
            stream_read(a, s.pieces, at + ctl, 16, tag);             // the stored tag, wherever the chunk boundaries fall
            const uint32_t idx = (uint32_t)gents.size();
            gents.push_back(ge); tags.insert(tags.end(), tag, tag + 16);
            gkeys.push(idx, m.key);
            giv.insert(giv.end(), iv, iv + 16);
            for (uint64_t o = 0; o < ctl; o += CTR_UNIT) units.push_back(CipherUnit{outp + o, o, (uint32_t)std::min<uint64_t>(CTR_UNIT, ctl - o), idx});
            outp += ctl; at += segl; rest -= segl; counter++;
            if (!fin && segl != (uint64_t)s.gcm_seg + 16) return fail(c, PNA_E_INVAL, "GCM STREAM: short non-final segment");
        }
        s.g1 = (uint32_t)gents.size();
    }
    if (gents.empty()) return PNA_OK;                                  // (verdict mode: every stream failed its key confirmation)
    gkeys.sort_units(units);
    if (c->ci_gcm.ensure(gents.size() * sizeof(GcmEntry) + 16) || c->x_tags.ensure(tags.size() + 16) ||
        c->ci_ivs.ensure(giv.size() + 16) || c->ci_units.ensure(units.size() * sizeof(CipherUnit) + 16)) return fail(c, PNA_E_NOMEM, "cipher workspace");
    HIPCHK(c, hipMemcpyAsync(c->x_flag.p, flag0, 8, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(c->ci_gcm.p, gents.data(), gents.size() * sizeof(GcmEntry), hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(c->x_tags.p, tags.data(), tags.size(), hipMemcpyHostToDevice, st));
    rc = gkeys.upload(c, st); if (rc) return rc;
    HIPCHK(c, hipMemcpyAsync(c->ci_ivs.p, giv.data(), giv.size(), hipMemcpyHostToDevice, st));
    if (!units.empty()) HIPCHK(c, hipMemcpyAsync(c->ci_units.p, units.data(), units.size() * sizeof(CipherUnit), hipMemcpyHostToDevice, st));
    if (x.verdict) {
        if (c->v_seg.ensure(gents.size() * 4 + 16)) return fail(c, PNA_E_NOMEM, "cipher workspace");
        launch_gcm_verdict((const GcmEntry *)c->ci_gcm.p, (uint32_t)gents.size(), (const uint8_t *)c->x_pk.p, (const uint8_t *)c->x_tags.p, (uint32_t *)c->v_seg.p, st);
    } else {
        launch_gcm_verify((const GcmEntry *)c->ci_gcm.p, (uint32_t)gents.size(), (const uint8_t *)c->x_pk.p, (const uint8_t *)c->x_tags.p, (uint32_t *)c->x_flag.p, st);
        rc = read_back(c, flag, c->x_flag.p, 8, st); if (rc) return rc;
        if (flag[0]) return fail(c, PNA_E_INVAL, "GCM STREAM: authentication failure (a segment tag does not match)");
    }
    rc = cipher_ctr(c, (const CipherUnit *)c->ci_units.p, (uint32_t)units.size(), (const uint8_t *)c->ci_ivs.p, (uint8_t *)c->x_pk.p, BlockKey{}, &gkeys, st);
    if (rc) return rc;
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(st));
    return PNA_OK;
}
// the entries with fSIZ: one decode call per codec into the raw buffer
// who a stream is, in an error's text
static std::string stream_label(const XStream &s) { return s.htype[0] == 'S' ? std::string("solid stream") : "entry '" + static_cast<const XEntry &>(s).name + "'"; }
// an xz stream of this driver's choosing failed for `reason`: the decoder numbers the streams of its call, the archive's reader knows them by name
static int xz_named_error(pna_gpu_ctx *c, int rc, const XStream &s, const std::string &reason) {
    if (rc == PNA_E_INVAL || rc == PNA_E_UNSUPPORTED) c->err = stream_label(s) + ": " + reason;
    return rc;
}
// the entries of one codec that `pick` chooses, as the lists of a decode call: (pk_off, pay_len, raw_off, raw_size), and which entries they are
struct SizedLists { std::vector<uint64_t> so, sl, dof, rl; std::vector<size_t> idx; };
template <class Pick> static SizedLists gather_sized(const std::vector<XEntry> &ents, int algo, Pick pick) {
    SizedLists l;
    for (size_t i = 0; i < ents.size(); i++) {
        const XEntry &e = ents[i];
        if (e.compression == algo && e.has_size && pick(i)) { l.so.push_back(e.pk_off); l.sl.push_back(e.pay_len); l.dof.push_back(e.raw_off); l.rl.push_back(e.raw_size); l.idx.push_back(i); }
    }
    return l;
}
static int decode_sized(pna_gpu_ctx *c, const std::vector<XEntry> &ents, int slot, hipStream_t st) {
    for (int algo : {PNA_ALGO_ZSTD, PNA_ALGO_DEFLATE, PNA_ALGO_XZ}) {
        const SizedLists l = gather_sized(ents, algo, [](size_t) { return true; });
        XzFail why;
        const int rc = decode_batch(c, algo, DecodeBatch{l.idx.size(), c->x_pk.p, l.so.data(), l.sl.data(), c->x_raw[slot].p, l.dof.data(), l.rl.data(), false, nullptr, nullptr, st}, &why);
        if (rc) return why.index < l.idx.size() ? xz_named_error(c, rc, ents[l.idx[why.index]], why.reason) : rc;
    }
    return PNA_OK;
}
// A stream whose decoded size is recorded nowhere -- an entry without fSIZ, a solid stream -- measured on the device (pna_gpu_open_size_device: the exact
// size, or a proven bound), decoded into c->solid_plain of that size and copied to `out` (a stored one is copied from the packed buffer as it is)
// (out == NULL: `pna verify` -- decoded on the device and dropped; *size_out receives the size found)
static int decode_open(pna_gpu_ctx *c, const XStream &s, const char *what, std::vector<uint8_t> *out, hipStream_t st, uint64_t *size_out = nullptr) {
    uint64_t got = s.pay_len; const void *d = (const uint8_t *)c->x_pk.p + s.pk_off;
    if (s.compression != PNA_ALGO_STORE) {
        OpenSize m;
        int rc = open_size(c, s.compression, c->x_pk.p, s.pk_off, s.pay_len, &m, st);
        if (rc) return s.compression == PNA_ALGO_XZ ? xz_named_error(c, rc, s, std::string(c->err)) : rc;      // (the measurement's text carries no stream number)
        XzFail why;
        const uint64_t cap = m.size, at0 = 0; const int exact = m.exact;      // (at0: the stream is decoded into solid_plain[0 ..]; zstd plans its frames from the measurement)
        auto nomem = [&]() {
            char msg[192];
            snprintf(msg, sizeof msg, "%s: the stream decodes to %s%llu bytes, more than the device's free memory takes (with the decoder's workspace)", what,
                     exact ? "" : "at most ", (unsigned long long)cap);
            return fail(c, PNA_E_NOMEM, msg);
        };
        if (c->solid_plain.ensure(cap + 8192)) return nomem();
        rc = decode_batch(c, s.compression, DecodeBatch{1, c->x_pk.p, &s.pk_off, &s.pay_len, c->solid_plain.p, &at0, &cap, true, &got, nullptr, st, &m}, &why);
        if (rc == PNA_E_NOMEM) return nomem();
        if (rc) return why.index == 0 ? xz_named_error(c, rc, s, why.reason) : rc;
        d = c->solid_plain.p;
    }
    if (size_out) *size_out = got;
    if (!out) return PNA_OK;
    out->resize((size_t)got);
    if (got) HIPCHK(c, hipMemcpy(out->data(), d, got, hipMemcpyDeviceToHost));
    return PNA_OK;
}
// A solid entry: its stream decoded, then read_next_normal_entry_from_stream over it (lib/src/entry.rs:401-424): small chunks checked here, the
// inner FDAT CRCs on the device over the decoded stream where it stands
// Verdict mode (vst != NULL): what fails marks the whole block (*vst, a PNA_VERIFY_* status) instead of failing the call.
static int walk_solid(pna_gpu_ctx *c, const XSolid &so, std::vector<uint8_t> &plain, std::vector<Inner> &inner, uint32_t flag[2], hipStream_t st, int *vst = nullptr) {
    auto vfail = [&](int code, int status, const char *what) { if (!vst) return fail(c, code, what); *vst = status; inner.clear(); return (int)PNA_OK; };
    int rc = decode_open(c, so, "solid stream buffer", &plain, st);
    if (rc && vst && (rc == PNA_E_INVAL || rc == PNA_E_UNSUPPORTED)) return vfail(rc, rc == PNA_E_INVAL ? PNA_VERIFY_BAD_STREAM : PNA_VERIFY_UNSUPPORTED, "");
    if (rc) return rc;
    std::vector<FrameDesc> ichunks; Inner ic; bool in_i = false;
    for (size_t q = 0; q < plain.size();) {
        PnaChunk ch;
        const int r = next_chunk(plain.data(), plain.size(), q, ch);
        if (r) return vfail(PNA_E_INVAL, PNA_VERIFY_BAD_STRUCTURE, r == CHUNK_SHORT_HEADER ? "solid stream: truncated chunk header" : "solid stream: truncated chunk body");
        const bool fd = memcmp(ch.type, "FDAT", 4) == 0;
        if (fd) { if (ch.len > 0xFFFFFFFBu) return vfail(PNA_E_INVAL, PNA_VERIFY_BAD_STRUCTURE, "data chunk too long"); ichunks.push_back(FrameDesc{ch.off, ch.len, 0, 8, 0}); }
        else if (!chunk_crc_ok(ch)) return vfail(PNA_E_INVAL, PNA_VERIFY_BAD_CRC, "solid stream: chunk CRC mismatch");
        if (memcmp(ch.type, "FHED", 4) == 0) {
            if (in_i || ch.len < 6 || ch.data[0] != 0 || ch.data[1] != 0) return vfail(PNA_E_INVAL, PNA_VERIFY_BAD_STRUCTURE, "solid stream: bad entry header");
            if (ch.data[3] != PNA_ALGO_STORE || ch.data[4] != PNA_ENC_NONE) return vfail(PNA_E_UNSUPPORTED, PNA_VERIFY_UNSUPPORTED, "solid stream: inner entry that is not stored");
            ic = Inner(); in_i = true; ic.kind = ch.data[2]; ic.len = 0; ic.name.assign((const char *)ch.data + 6, ch.len - 6);
        } else if (!in_i) { if (!(ch.type[0] & 0x20)) return vfail(PNA_E_INVAL, PNA_VERIFY_BAD_STRUCTURE, "solid stream: unknown critical chunk"); }
        else if (fd) { ic.pieces.push_back(XPiece{ch.off + 8, ch.len}); ic.len += ch.len; }
        else if (memcmp(ch.type, "FEND", 4) == 0) { inner.push_back(std::move(ic)); in_i = false; }
        else if (memcmp(ch.type, "fSIZ", 4) == 0 && ch.len <= 8) { ic.has_size = true; ic.raw_size = 0; for (uint32_t i = 0; i < ch.len; i++) ic.raw_size = (ic.raw_size << 8) | ch.data[i]; }
        else if (memcmp(ch.type, "fSIZ", 4) != 0 && !(ch.type[0] & 0x20)) return vfail(PNA_E_INVAL, PNA_VERIFY_BAD_STRUCTURE, "solid stream: unknown critical chunk");
    }
    if (in_i) return vfail(PNA_E_INVAL, PNA_VERIFY_BAD_STRUCTURE, "solid stream: dangling chunks");
    if (ichunks.empty()) return PNA_OK;
    if (c->solid_desc.ensure(ichunks.size() * sizeof(FrameDesc) + 16)) return fail(c, PNA_E_NOMEM, "extract workspace");
    HIPCHK(c, hipMemcpyAsync(c->x_flag.p, flag0, 8, hipMemcpyHostToDevice, st));
    const bool stored = so.compression == PNA_ALGO_STORE;            // a stored stream is checked where it stands in the packed buffer
    if (stored) for (auto &f : ichunks) f.arc_off += so.pk_off;
    HIPCHK(c, hipMemcpyAsync(c->solid_desc.p, ichunks.data(), ichunks.size() * sizeof(FrameDesc), hipMemcpyHostToDevice, st));
    verify_chunks(c, c->solid_desc, ichunks, stored ? c->x_pk : c->solid_plain, "FDAT", st);
    rc = read_back(c, flag, c->x_flag.p, 8, st); if (rc) return rc;
    if (flag[0]) return vfail(PNA_E_INVAL, PNA_VERIFY_BAD_CRC, "solid stream: inner FDAT CRC mismatch");
    return PNA_OK;
}
// ---- 4. the hand-out: entries in archive order, solid entries' inner entries in front of the normal entry that followed them
static int deliver_entries(pna_gpu_ctx *c, pna_entry_fn cb, void *user, const XOut &D, const uint8_t *raw_host, const uint8_t *pk_host, hipEvent_t wait_ev) {
    const auto dt0 = std::chrono::steady_clock::now();
    if (wait_ev && hipEventSynchronize(wait_ev) != hipSuccess) return fail(c, PNA_E_HIP, "D2H copy failed");
    const double dwait = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - dt0).count();
    struct Tr { double w; std::chrono::steady_clock::time_point t; ~Tr() { if (getenv("PNA_EXTRACT_TRACE")) fprintf(stderr, "[pna extract hand-out] waited %.1f ms for the D2H copy, callbacks %.1f ms\n", w, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t).count()); } } tr{dwait, std::chrono::steady_clock::now()};
    size_t idx = D.index0, si = 0;
    const size_t n = D.ents.size();
    std::vector<uint8_t> joined;
    auto deliver_solids = [&](size_t upto) -> int {
        for (; si < D.solid_order.size() && D.solid_order[si] <= upto; si++)
            for (const Inner &ie : D.inner[si]) {
                const uint8_t *d = D.plain[si].data();
                if (ie.pieces.size() == 1) d += ie.pieces[0].off;
                else { joined.clear(); for (const XPiece &p : ie.pieces) joined.insert(joined.end(), d + p.off, d + p.off + p.len); d = joined.data(); }
                std::string path; { const int rp = entry_path(c, ie.name, path); if (rp) return rp; }
                if (cb(user, idx++, path.c_str(), ie.kind, ie.len ? d : nullptr, (size_t)ie.len) != 0) return fail(c, PNA_E_SINK, "entry callback failed");
            }
        return PNA_OK;
    };
    for (size_t i = 0; i < n; i++) {
        int rc = deliver_solids(i); if (rc) return rc;
        const XEntry &e = D.ents[i];
        const uint8_t *d = e.compression == PNA_ALGO_STORE ? pk_host + e.pk_off
                         : (e.has_size ? raw_host + e.raw_off : D.nosize_data[(size_t)e.raw_off].data());
        const size_t l = e.compression == PNA_ALGO_STORE ? (size_t)e.pay_len : (size_t)e.raw_size;
        if (e.compression == PNA_ALGO_STORE && e.has_size && e.raw_size != e.pay_len) return fail(c, PNA_E_INVAL, "stored entry: fSIZ differs from the data length");
        std::string path; { const int rp = entry_path(c, e.name, path); if (rp) return rp; }
        if (cb(user, idx++, path.c_str(), e.kind, d, l) != 0) return fail(c, PNA_E_SINK, "entry callback failed");
    }
    return deliver_solids(n);
}
// Back to the host.  Deferred form (no stored entries in the window): the D2H copy runs on its own stream behind the window's kernels and the
// hand-out happens later (see the driver); everything it needs is in `D`.
static int hand_out(XCall &x, std::shared_ptr<XOut> D, const XPlan &P, bool any_store, bool defer, int slot, XDeferred *later, hipStream_t st) {
    pna_gpu_ctx *c = x.c;
    if (c->hp_out[slot].ensure(P.raw_total + 64) || (any_store && c->hp_in[0].ensure(P.pk_total + 64))) return fail(c, PNA_E_NOMEM, "staging allocation failed");
    auto issue = [c, slot, raw_bytes = P.raw_total]() -> int {                      // the window's kernels are complete on c->stream when this runs or are ordered before it by x_done
        if (raw_bytes && hipMemcpyAsync(c->hp_out[slot].p, c->x_raw[slot].p, raw_bytes, hipMemcpyDeviceToHost, c->x_cp) != hipSuccess) return fail(c, PNA_E_HIP, "D2H copy failed");
        return hipEventRecord(c->x_ev[slot], c->x_cp) == hipSuccess ? PNA_OK : fail(c, PNA_E_HIP, "D2H copy failed");
    };
    if (defer) {
        if (!c->x_cp) {
            HIPCHK(c, hipStreamCreateWithFlags(&c->x_cp, hipStreamNonBlocking));
            for (auto &e : c->x_ev) HIPCHK(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
            HIPCHK(c, hipEventCreateWithFlags(&c->x_done, hipEventDisableTiming));
        }
        HIPCHK(c, hipEventRecord(c->x_done, st));
        HIPCHK(c, hipStreamWaitEvent(c->x_cp, c->x_done, 0));
    } else {
        if (P.raw_total) HIPCHK(c, hipMemcpyAsync(c->hp_out[slot].p, c->x_raw[slot].p, P.raw_total, hipMemcpyDeviceToHost, st));
        if (any_store) HIPCHK(c, hipMemcpyAsync(c->hp_in[0].p, c->x_pk.p, P.pk_total, hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipStreamSynchronize(st));
    }
    D->index0 = x.index;
    x.index += D->ents.size(); for (const auto &v : D->inner) x.index += v.size();
    const uint8_t *raw_host = (const uint8_t *)c->hp_out[slot].p, *pk_host = (const uint8_t *)c->hp_in[0].p;
    hipEvent_t wait_ev = defer ? c->x_ev[slot] : nullptr;
    auto deliver = [c, cb = x.cb, user = x.user, D, raw_host, pk_host, wait_ev]() -> int { return deliver_entries(c, cb, user, *D, raw_host, pk_host, wait_ev); };
    if (defer) { later->issue = issue; later->deliver = deliver; later->issued = false; return PNA_OK; }
    return deliver();
}

// One window of the driver above: `a` / archive_len are the window's bytes, every offset in ents / dchunks / schunks / solids is relative to it.
static int extract_window(XCall &x, const WinSrc &a, size_t archive_len, std::vector<XEntry> &ents, std::vector<FrameDesc> &dchunks, std::vector<FrameDesc> &schunks,
                          std::vector<XSolid> &solids, int slot, XDeferred *later, XDeferred *prev) {
    pna_gpu_ctx *c = x.c;
    XPlan P;
    int rc = plan_window(x, a, ents, solids, P); if (rc) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    static const bool xtrace = getenv("PNA_EXTRACT_TRACE") != nullptr;   // per-window phase times on stderr
    const auto xt0 = std::chrono::steady_clock::now();
    auto xms = [&]() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - xt0).count(); };
    uint32_t flag[2] = {0, 0};
    rc = upload_window(c, a, archive_len, dchunks, schunks, P, slot, flag, st); if (rc) return rc;
    const double x_in = xms();
    // This window's bytes are on the device: now the previous window's decoded entries start their way back, next to this window's
    // decryption and decoding.  (Issued earlier, the two copies share the link -- H2D of 1 GiB next to D2H of 2.5 GiB took 67 ms, as long
    // as one after the other -- and the kernels would again run with the link idle.)
    if (prev && *prev && !prev->issued) { prev->issued = true; const int r = prev->issue(); if (r) return r; }
    if (flag[0]) { c->err = "data chunk CRC mismatch (" + std::to_string(flag[0]) + " FDAT / SDAT chunks)"; return PNA_E_INVAL; }
    rc = derive_ahead_plan(x, P.enc_list, P.gcm_list); if (rc) return rc;
    if (!P.enc_list.empty()) { rc = decrypt_ctr_cbc(x, P.enc_list, st); if (rc) return rc; }
    if (!P.gcm_list.empty()) { rc = decrypt_gcm(x, a, P.gcm_list, flag, st); if (rc) return rc; }
    rc = decode_sized(c, ents, slot, st); if (rc) return rc;
    auto D = std::make_shared<XOut>();
    for (size_t i : P.nosize_idx) {                                   // compatibility path, one decode call per entry
        XEntry &e = ents[i];
        D->nosize_data.emplace_back();
        rc = decode_open(c, e, "entry buffer", &D->nosize_data.back(), st); if (rc) return rc;
        e.raw_size = D->nosize_data.back().size(); e.raw_off = D->nosize_data.size() - 1;      // index into nosize_data
    }
    D->inner.resize(solids.size()); D->plain.resize(solids.size());
    for (size_t si = 0; si < solids.size(); si++) {                   // (an encrypted stream has been decrypted in place by the cipher stages above)
        rc = walk_solid(c, solids[si], D->plain[si], D->inner[si], flag, st); if (rc) return rc;
        D->solid_order.push_back(solids[si].order);
    }
    bool any_store = false; for (const XEntry &e : ents) any_store |= e.compression == PNA_ALGO_STORE && e.pay_len;
    const bool defer = later != nullptr && !any_store;
    if (xtrace) { (void)hipStreamSynchronize(st); fprintf(stderr, "[pna extract window] %zu entries, %.0f MiB in -> %.0f MiB out: H2D + CRC + gather %.1f ms, decrypt + decode %.1f ms (slot %d, %s)\n", ents.size(), archive_len / 1048576.0, P.raw_total / 1048576.0, x_in, xms() - x_in, slot, defer ? "deferred hand-out" : "immediate"); }
    D->ents = std::move(ents);
    return hand_out(x, D, P, any_store, defer, slot, later, st);
}

// ---- 2. windows: a run of entries whose archive bytes, packed payloads and decoded bytes stay within a few GiB each goes through the device at a time
// (an archive of any size in host memory against a bounded footprint in HBM); a solid entry is a window of its own.  Moves the next window's entries,
// chunks and solid entry out of the walk's lists, offsets relative to its first byte `base`.
struct XWindow { std::vector<XEntry> we; std::vector<FrameDesc> wd, ws; std::vector<XSolid> wso; uint64_t base = 0, span = 0; };
static void next_window(pna_gpu_ctx *c, std::vector<XEntry> &ents, const std::vector<FrameDesc> &dchunks, const std::vector<FrameDesc> &schunks,
                        std::vector<XSolid> &solids, size_t &w0, size_t &si, XWindow &W) {
    const size_t n_all = ents.size();
    const uint64_t WIN = (uint64_t)c->tun.extract_win_mib << 20;  // 1 GiB of archive (and at most 3 GiB decoded) per window by default: small enough to pipeline, large enough for the kernels
    if (si < solids.size() && solids[si].order <= w0) {
        W.wso.push_back(std::move(solids[si++])); W.wso[0].order = 0;
        W.base = W.wso[0].lo; W.span = W.wso[0].hi - W.base;
        rebase(W.wso, schunks, W.wso[0].s0, W.wso[0].s1, W.ws, W.base);
    } else {
        size_t w1 = w0; uint64_t raw = 0, pk = 0;
        const size_t stop = si < solids.size() ? std::min(n_all, solids[si].order) : n_all;
        while (w1 < stop) {
            const XEntry &e = ents[w1];
            const uint64_t r = e.has_size ? e.raw_size : 0;
            if (w1 > w0 && (e.hi - ents[w0].lo > WIN || raw + r > 3 * WIN || pk + e.stream_len > WIN)) break;
            raw += r; pk += e.stream_len; w1++;
        }
        W.we.assign(std::make_move_iterator(ents.begin() + w0), std::make_move_iterator(ents.begin() + w1));
        W.base = W.we.front().lo; W.span = W.we.back().hi - W.base;
        rebase(W.we, dchunks, W.we.front().d0, W.we.back().d1, W.wd, W.base);
        w0 = w1;
    }
}

extern "C" int pna_gpu_extract_archive_host(pna_gpu_ctx *c, const void *archive, size_t archive_len, const void *password, size_t password_len,
                                            pna_entry_fn cb, void *user) {
    if (!c || !archive || !cb || (!password && password_len)) return fail(c, PNA_E_INVAL, "null argument");
    const uint8_t *a = (const uint8_t *)archive;
    if (archive_len < 8 + 20 + 12 || memcmp(a, PNA_SIGNATURE, 8) != 0) return fail(c, PNA_E_INVAL, "not a PNA archive");
    const ArcParts ap{&a, &archive_len, 1, {0}};
    std::vector<XEntry> ents; std::vector<FrameDesc> dchunks, schunks; std::vector<XSolid> solids;
    bool broken = false;
    int rc = walk_archive(c, ap, false, ents, dchunks, schunks, solids, &broken);
    if (rc) return rc;
    XCall x{c, password, password_len, cb, user, {}, 0};
    size_t si = 0, w0 = 0;
    const size_t n_all = ents.size();
    // Windows are pipelined against each other: the decoded entries of window k travel to the host (their own stream, their own pair of
    // buffers) while window k + 1 is copied in and decoded; window k's entries are handed out once k + 1 has been launched, before k + 1's.
    XDeferred pending; int slot = 0;
    auto finish_pending = [&]() -> int {
        if (!pending) return PNA_OK;
        XDeferred f = std::move(pending); pending = XDeferred();
        if (!f.issued) { const int r = f.issue(); if (r) return r; }
        return f.deliver();
    };
    while (w0 < n_all || si < solids.size()) {
        XWindow W;
        next_window(c, ents, dchunks, schunks, solids, w0, si, W);
        XDeferred cur;
        rc = extract_window(x, WinSrc{&ap, W.base}, (size_t)W.span, W.we, W.wd, W.ws, W.wso, slot, &cur, pending ? &pending : nullptr);
        const int rc2 = finish_pending();
        if (rc == PNA_OK) rc = rc2;
        if (rc != PNA_OK) { (void)hipDeviceSynchronize(); return rc; }
        pending = std::move(cur); slot ^= 1;
    }
    return finish_pending();
}

// ---- `pna verify` (pna_gpu_verify_archive_host): the same stages in verdict mode.  One window: its bytes and the data chunks' CRC verdicts (one word per
// chunk), CTR / CBC / GCM with their verdicts kept on the device (CBC plaintext lengths, one word per GCM segment), k_verdict folding them with the walk's
// findings into one status word per record -- the only read-back besides the decoders' own --, then the records that passed are decoded into the device's
// raw buffer and dropped: nothing decoded goes to the host (solid streams excepted: their inner entries are walked on the host, as extract does).
struct VCall {
    pna_verify_fn cb; void *user; pna_verify_summary sum{};
};
static int emit(XCall &x, VCall &v, const char *name, int kind, int status, uint32_t flags, uint64_t size) {
    static const char *const what[] = {"", "encrypted, no password given", "chunk CRC mismatch", "broken chunk structure", "authentication failed (wrong password or tampering)",
                                       "bad CBC length or padding (wrong password or damaged data)", "corrupt stream", "not decoded by this build"};
    const char *detail = status >= 0 && status <= PNA_VERIFY_UNSUPPORTED ? what[status] : "";
    v.sum.total++;
    if (status == PNA_VERIFY_OK) v.sum.ok++;
    else if (status == PNA_VERIFY_SKIPPED) v.sum.skipped++;
    else if (status == PNA_VERIFY_UNSUPPORTED) v.sum.unsupported++;
    else { v.sum.failed++; if (flags & PNA_VERIFY_UNAUTHENTICATED) v.sum.unauthenticated_failure = 1; }
    if (v.cb(v.user, x.index++, name, kind, status, flags, size, detail) != 0) return fail(x.c, PNA_E_SINK, "verify callback failed");
    return PNA_OK;
}
static uint32_t fail_flags(const XStream &s, int status) {     // CTR / CBC: a failure after the CRC check may be a wrong password (verify.rs is_unauthenticated)
    return (status == PNA_VERIFY_BAD_DECRYPT || status == PNA_VERIFY_BAD_STREAM || status == PNA_VERIFY_BAD_AUTH) ? (s.vfl & PNA_VERIFY_UNAUTHENTICATED) : 0u;
}
// plan, upload, decryption and the fold of a window in verdict mode: vs receives one status word per record (the window's entries, or its solid entry)
static int window_verdicts(XCall &x, const WinSrc &a, size_t span, std::vector<XEntry> &ents, std::vector<FrameDesc> &dchunks, std::vector<FrameDesc> &schunks,
                           std::vector<XSolid> &solids, XPlan &P, std::vector<uint32_t> &vs, uint32_t flag[2], hipStream_t st) {
    pna_gpu_ctx *c = x.c;
    int rc = plan_window(x, a, ents, solids, P); if (rc) return rc;
    rc = upload_window(c, a, span, dchunks, schunks, P, 0, flag, st, true); if (rc) return rc;
    rc = derive_ahead_plan(x, P.enc_list, P.gcm_list); if (rc) return rc;
    if (!P.enc_list.empty()) { rc = decrypt_ctr_cbc(x, P.enc_list, st); if (rc) return rc; }
    if (!P.gcm_list.empty()) { rc = decrypt_gcm(x, a, P.gcm_list, flag, st); if (rc) return rc; }
    // the fold: one VerdictEnt per record (the window's entries, or its solid entry), one status word back per record
    std::vector<VerdictEnt> ve;
    const size_t d_base = ents.empty() ? 0 : ents.front().d0;
    for (const XEntry &e : ents) ve.push_back(VerdictEnt{(uint32_t)(e.d0 - d_base), (uint32_t)(e.d1 - d_base), e.g0, e.g1, e.cbc_unit, (uint32_t)e.vst});
    for (const XSolid &so : solids) ve.push_back(VerdictEnt{0u, (uint32_t)schunks.size(), so.g0, so.g1, so.cbc_unit, (uint32_t)so.vst});
    vs.assign(ve.size(), 0);
    if (!ve.empty()) {
        if (c->v_ent.ensure(ve.size() * sizeof(VerdictEnt) + 16) || c->v_out.ensure(ve.size() * 4 + 16)) return fail(c, PNA_E_NOMEM, "verify workspace");
        HIPCHK(c, hipMemcpyAsync(c->v_ent.p, ve.data(), ve.size() * sizeof(VerdictEnt), hipMemcpyHostToDevice, st));
        launch_verdict((const VerdictEnt *)c->v_ent.p, (uint32_t)ve.size(), (const uint32_t *)c->v_crc.p, (const uint32_t *)c->v_seg.p, (const uint32_t *)c->x_plen.p,
                       (uint32_t *)c->v_out.p, st);
        rc = read_back(c, vs.data(), c->v_out.p, vs.size() * 4, st); if (rc) return rc;
    }
    return PNA_OK;
}
// the entries with fSIZ that passed so far: one decode call per codec into the raw buffer, a status per entry; a stream whose size disagrees with its
// fSIZ (status 3) goes to `retry` (decoded once more without it: the reference reads an entry to its end and only warns about a wrong fSIZ), a corrupt
// one does not.  Returns the number of streams handed to the decoders in *streams.
static int decode_sized_status(pna_gpu_ctx *c, const std::vector<XEntry> &ents, std::vector<uint32_t> &vs, std::vector<uint64_t> &size, std::vector<size_t> &retry,
                               hipStream_t st, uint64_t *streams = nullptr) {
    for (int algo : {PNA_ALGO_ZSTD, PNA_ALGO_DEFLATE, PNA_ALGO_XZ}) {
        const SizedLists l = gather_sized(ents, algo, [&](size_t i) { return !vs[i] && !ents[i].nodecode && !ents[i].odd_size; });
        if (streams) *streams += l.idx.size();
        std::vector<uint32_t> es(l.idx.size(), 0);
        const int rc = decode_batch(c, algo, DecodeBatch{l.idx.size(), c->x_pk.p, l.so.data(), l.sl.data(), c->x_raw[0].p, l.dof.data(), l.rl.data(), false, nullptr, es.data(), st}); if (rc) return rc;
        for (size_t k = 0; k < l.idx.size(); k++) {
            const size_t i = l.idx[k];
            if (es[k] == 0) size[i] = ents[i].raw_size;
            else if (es[k] == 2) vs[i] = PNA_VERIFY_UNSUPPORTED;
            else if (es[k] == 3) retry.push_back(i);                     // the stream does not hold fSIZ bytes: measured and decoded without it
            else vs[i] = PNA_VERIFY_BAD_STREAM;
        }
    }
    return PNA_OK;
}
static int verify_window(XCall &x, VCall &v, const WinSrc &a, size_t span, std::vector<XEntry> &ents, std::vector<FrameDesc> &dchunks,
                         std::vector<FrameDesc> &schunks, std::vector<XSolid> &solids) {
    pna_gpu_ctx *c = x.c;
    XPlan P;
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    uint32_t flag[2] = {0, 0};
    std::vector<uint32_t> vs;
    int rc = window_verdicts(x, a, span, ents, dchunks, schunks, solids, P, vs, flag, st); if (rc) return rc;
    if (!solids.empty()) {                                             // a solid entry: one record for the block, or one per inner entry
        const XSolid &so = solids[0];
        int status = (int)vs[0];
        if (!x.fast && status == PNA_VERIFY_OK) {
            std::vector<uint8_t> plain; std::vector<Inner> inner; int vst = 0;
            rc = walk_solid(c, so, plain, inner, flag, st, &vst); if (rc) return rc;
            if (!vst) {
                for (const Inner &ie : inner) {
                    std::string path;
                    const bool named = entry_path(c, ie.name, path) == PNA_OK;
                    rc = emit(x, v, named ? path.c_str() : nullptr, ie.kind, named ? PNA_VERIFY_OK : PNA_VERIFY_BAD_STRUCTURE, 0u, ie.len); if (rc) return rc;
                }
                return PNA_OK;
            }
            status = vst;
        }
        return emit(x, v, nullptr, PNA_VERIFY_KIND_SOLID, status, fail_flags(so, status), 0);
    }
    std::vector<uint64_t> size(ents.size(), 0); std::vector<uint32_t> flags(ents.size(), 0);
    for (size_t i = 0; i < ents.size(); i++) {
        XEntry &e = ents[i];
        if (x.fast || vs[i]) continue;
        if (e.compression == PNA_ALGO_STORE) { size[i] = e.pay_len; if (e.has_size && e.raw_size != e.pay_len) flags[i] |= PNA_VERIFY_SIZE_HINT; }
    }
    std::vector<size_t> retry;
    if (!x.fast) { rc = decode_sized_status(c, ents, vs, size, retry, st); if (rc) return rc; }
    for (size_t i : P.nosize_idx) if (!vs[i]) retry.push_back(i);   // (entries without fSIZ, or with one out of proportion to their data)
    for (size_t i : retry) {
        XEntry &e = ents[i];
        uint64_t got = 0;
        rc = decode_open(c, e, "entry buffer", nullptr, st, &got);
        if (rc == PNA_E_INVAL || rc == PNA_E_UNSUPPORTED) { vs[i] = rc == PNA_E_INVAL ? PNA_VERIFY_BAD_STREAM : PNA_VERIFY_UNSUPPORTED; continue; }
        if (rc) return rc;
        size[i] = got;
        if (e.has_size && got != e.raw_size) flags[i] |= PNA_VERIFY_SIZE_HINT;
    }
    for (size_t i = 0; i < ents.size(); i++) {
        const XEntry &e = ents[i];
        int status = (int)vs[i];
        std::string path; const char *name = nullptr;
        if (!e.noname) {
            if (entry_path(c, e.name, path) == PNA_OK) name = path.c_str();
            else if (status == PNA_VERIFY_OK) status = PNA_VERIFY_BAD_STRUCTURE;      // a name that is not UTF-8 (InvalidData in the reference)
        }
        if (status != PNA_VERIFY_OK) size[i] = 0;
        rc = emit(x, v, name, e.kind, status, status == PNA_VERIFY_OK ? flags[i] : fail_flags(e, status), size[i]); if (rc) return rc;
    }
    return PNA_OK;
}

extern "C" int pna_gpu_verify_archive_host(pna_gpu_ctx *c, const void *const *parts, const size_t *part_len, size_t n_parts, const void *password,
                                           size_t password_len, uint32_t vflags, pna_verify_fn cb, void *user, pna_verify_summary *summary) {
    if (!c || !parts || !part_len || !n_parts || !cb || (!password && password_len)) return fail(c, PNA_E_INVAL, "null argument");
    if (vflags & ~(uint32_t)PNA_VERIFY_FAST) return fail(c, PNA_E_INVAL, "unknown verify flag");
    for (size_t k = 0; k < n_parts; k++) if (!parts[k]) return fail(c, PNA_E_INVAL, "null argument");
    if (part_len[0] < 8 || memcmp(parts[0], PNA_SIGNATURE, 8) != 0) return fail(c, PNA_E_INVAL, "not a PNA archive");
    if (!launch_frame_verdict || !launch_verdict || !launch_gcm_verdict) return fail(c, PNA_E_UNSUPPORTED, "this build has no verdict kernels");
    ArcParts ap{(const uint8_t *const *)parts, part_len, n_parts, {}};
    uint64_t at = 0;
    for (size_t k = 0; k < n_parts; k++) { ap.vb.push_back(at); at += part_len[k]; }
    const bool fast = (vflags & PNA_VERIFY_FAST) != 0;
    XCall x{c, fast ? nullptr : password, fast ? 0 : password_len, nullptr, nullptr, {}, 0};
    x.verdict = true; x.fast = fast;
    VCall v{cb, user};
    std::vector<XEntry> ents; std::vector<FrameDesc> dchunks, schunks; std::vector<XSolid> solids;
    bool broken = false;
    int rc = walk_archive(c, ap, true, ents, dchunks, schunks, solids, &broken);
    size_t si = 0, w0 = 0;
    while (rc == PNA_OK && (w0 < ents.size() || si < solids.size())) {
        XWindow W;
        next_window(c, ents, dchunks, schunks, solids, w0, si, W);
        rc = verify_window(x, v, WinSrc{&ap, W.base}, (size_t)W.span, W.we, W.wd, W.ws, W.wso);
    }
    if (rc) (void)hipDeviceSynchronize();
    if (rc == PNA_OK && broken) { v.sum.broken = 1; rc = fail(c, PNA_E_INVAL, "archive structure is broken; verification aborted"); }
    if (summary) *summary = v.sum;
    return rc;
}

// ---- `pna experimental diff` (pna_gpu_diff_archive_host; cli/src/command/diff.rs diff_archive -> compare_entry): the verify driver with a second input.
// Per window: the host is asked for every record's filesystem side and settles what needs no byte (missing, type, size, not compared: left out of the
// decode lists); the rest is uploaded, decrypted, folded and decoded exactly as verify does; the files' bytes travel through two page-locked slots into
// two device slots on a stream of their own (DiffFeed) and k_diff compares them with the decoded bytes where the decoders left them -- the raw buffer,
// the packed buffer (stored entries) or the open-decode buffer (entries without fSIZ, solid streams) --; one read-back of first[] per window.
namespace {
struct DCall { pna_diff_source_fn src; pna_diff_fn cb; void *user; pna_diff_summary sum{}; };
// one record of a window: what the host said, what was settled without bytes (status, -1: the bytes are compared), where its decoded bytes lie
struct DRec {
    pna_diff_file f{PNA_DIFF_FS_MISSING, nullptr, 0};
    std::string path; bool named = false, want_link = false; int status = -1;
    int a_buf = 0; uint64_t a_off = 0, a_len = 0; bool a_ready = false;      // a_buf: 0 raw buffer, 1 packed buffer, 2 open-decode buffer; a_off is a multiple of 16
    std::string link;
};
// a run of a file's bytes in a slot: bytes [base, base + len) of record `rec`, their decoded side at the record's a_off + a_rel, the file's at `src`;
// slot number q of the window (device slot q & 1) at b_off, which is congruent to a_rel mod 16
struct FPiece { uint32_t rec; uint64_t a_rel, base, len; const uint8_t *src; uint64_t q, b_off; };
// compare_entry's match (diff.rs:353-419) as far as it is decided without the entry's bytes; -1: they are compared
int settle(int kind, const pna_diff_file &f, bool has_size, uint64_t raw_size, bool *want_link) {
    if (f.fs_kind == PNA_DIFF_FS_IGNORE) return PNA_DIFF_NOT_COMPARED;
    if (f.fs_kind == PNA_DIFF_FS_MISSING) return PNA_DIFF_MISSING;
    switch (kind) {
        case 0: if (f.fs_kind != PNA_DIFF_FS_FILE) return PNA_DIFF_TYPE_MISMATCH; return has_size && raw_size != f.len ? PNA_DIFF_SIZE_DIFFERS : -1;
        case 1: return f.fs_kind == PNA_DIFF_FS_DIR ? PNA_DIFF_NOT_COMPARED : PNA_DIFF_TYPE_MISMATCH;
        case 2: return f.fs_kind == PNA_DIFF_FS_SYMLINK ? -1 : PNA_DIFF_TYPE_MISMATCH;
        case 3: if (f.fs_kind != PNA_DIFF_FS_FILE) return PNA_DIFF_TYPE_MISMATCH; *want_link = true; return PNA_DIFF_NOT_COMPARED;
        default: return PNA_DIFF_NOT_COMPARED;
    }
}
constexpr uint64_t LINK_MAX = 65536;                            // a hard link's target handed to the host: at most this many bytes
// The files' side of a window.  add() plans where every byte goes (in record order, slot after slot, each run placed congruent to its decoded side
// mod 16); stage(q) fills slot q -- page-locked copy, then one H2D on the copy stream; bytes in a pna_gpu_host_alloc buffer go straight from there --;
// run(r) launches k_diff for the runs of the records up to r, slot by slot, staging slot q + 1 as soon as slot q - 1's launches are queued, so that
// its copy runs beside the kernels of slot q.  A slot is reused when the launches that read it are done (df_ev_k) and its copy has left (df_ev_cp).
struct DiffFeed {
    pna_gpu_ctx *c; hipStream_t st; std::vector<DRec> &recs; uint64_t cap;
    std::vector<FPiece> fp; size_t next = 0, stage_i = 0;
    uint64_t fill_q = 0, fill_pos = 0; int64_t staged = -1, cur_q = -1;
    std::vector<DiffPiece> pend[3]; uint32_t ptiles[3] = {0, 0, 0};
    DiffFeed(pna_gpu_ctx *ctx, hipStream_t s, std::vector<DRec> &r) : c(ctx), st(s), recs(r), cap((uint64_t)ctx->tun.diff_slot_mib << 20) {}
    int init(size_t nrec) {
        if (!c->df_cp) {
            HIPCHK(c, hipStreamCreateWithFlags(&c->df_cp, hipStreamNonBlocking));
            for (auto &e : c->df_ev_cp) HIPCHK(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
            for (auto &e : c->df_ev_k) HIPCHK(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
        }
        if (c->df_first.ensure(nrec * 8 + 16)) return fail(c, PNA_E_NOMEM, "diff workspace");
        HIPCHK(c, hipMemsetAsync(c->df_first.p, 0xFF, nrec * 8 + 16, st));
        return PNA_OK;
    }
    void add(uint32_t rec, uint64_t a_rel, uint64_t base, uint64_t len, const uint8_t *src) {
        while (len) {
            const uint64_t b = fill_pos + ((a_rel - fill_pos) & 15);
            if (b >= cap) { fill_q++; fill_pos = 0; continue; }
            const uint64_t n = std::min(len, cap - b);
            fp.push_back(FPiece{rec, a_rel, base, n, src, fill_q, b});
            fill_pos = b + n; a_rel += n; base += n; src += n; len -= n;
        }
    }
    bool lent(const uint8_t *p, uint64_t n, size_t &hint) const {       // (under lent_mu)
        for (size_t k = 0; k < c->lent.size(); k++) {
            const auto &bf = c->lent[(hint + k) % c->lent.size()];
            if (p >= bf.first && p + n <= bf.first + bf.second) { hint = (hint + k) % c->lent.size(); return true; }
        }
        return false;
    }
    int stage(uint64_t q) {
        const int s = (int)(q & 1);
        size_t i1 = stage_i; uint64_t extent = 0;
        while (i1 < fp.size() && fp[i1].q == q) { extent = std::max(extent, fp[i1].b_off + fp[i1].len); i1++; }
        if (c->df_pin[s].ensure_exact(cap) || c->df_dev[s].ensure(cap + 64)) return fail(c, PNA_E_NOMEM, "diff slots");
        if (q >= 2) {
            HIPCHK(c, hipEventSynchronize(c->df_ev_cp[s]));                          // the slot's previous bytes have left the page-locked buffer
            HIPCHK(c, hipStreamWaitEvent(c->df_cp, c->df_ev_k[s], 0));               // ... and the launches that read them on the device are done
        }
        struct Job { uint8_t *dst; const uint8_t *src; uint64_t n; };
        std::vector<Job> jobs; std::vector<size_t> direct; uint64_t bytes = 0;
        {
            std::lock_guard<std::mutex> lk(c->lent_mu);
            size_t hint = 0;
            for (size_t i = stage_i; i < i1; i++) {
                const FPiece &p = fp[i];
                if (!c->lent.empty() && lent(p.src, p.len, hint)) { direct.push_back(i); continue; }
                for (uint64_t o = 0; o < p.len; o += 1u << 20) jobs.push_back(Job{(uint8_t *)c->df_pin[s].p + p.b_off + o, p.src + o, std::min<uint64_t>(1u << 20, p.len - o)});
                bytes += p.len;
            }
        }
        if (!jobs.empty()) {
            const unsigned nt = (unsigned)std::min<uint64_t>(staging_threads(c), std::max<uint64_t>(1, bytes >> 22));
            par_ranges(jobs.size(), nt, [&](unsigned, size_t a0, size_t a1) { for (size_t j = a0; j < a1; j++) memcpy(jobs[j].dst, jobs[j].src, jobs[j].n); });
            HIPCHK(c, hipMemcpyAsync(c->df_dev[s].p, c->df_pin[s].p, extent, hipMemcpyHostToDevice, c->df_cp));
        }
        for (size_t i : direct) HIPCHK(c, hipMemcpyAsync((uint8_t *)c->df_dev[s].p + fp[i].b_off, fp[i].src, fp[i].len, hipMemcpyHostToDevice, c->df_cp));
        HIPCHK(c, hipEventRecord(c->df_ev_cp[s], c->df_cp));
        stage_i = i1; staged = (int64_t)q;
        return PNA_OK;
    }
    int prefill() {                                                   // the first two slots, before the window's own bytes are decoded: their copies run beside that
        for (uint64_t q = 0; q < 2 && !fp.empty() && q <= fp.back().q; q++) { const int rc = stage(q); if (rc) return rc; }
        return PNA_OK;
    }
    int flush() {                                                     // the pending runs to k_diff, one launch per buffer of decoded bytes
        const uint8_t *abuf[3] = {(const uint8_t *)c->x_raw[0].p, (const uint8_t *)c->x_pk.p, (const uint8_t *)c->solid_plain.p};
        for (int k = 0; k < 3; k++) {
            if (pend[k].empty()) continue;
            if (c->df_pieces.ensure(pend[k].size() * sizeof(DiffPiece) + 16)) return fail(c, PNA_E_NOMEM, "diff workspace");
            while (c->df_tev.size() < c->df_tused + 2) { hipEvent_t e; HIPCHK(c, hipEventCreate(&e)); c->df_tev.push_back(e); }
            HIPCHK(c, hipMemcpyAsync(c->df_pieces.p, pend[k].data(), pend[k].size() * sizeof(DiffPiece), hipMemcpyHostToDevice, st));
            HIPCHK(c, hipEventRecord(c->df_tev[c->df_tused], st));
            launch_diff((const DiffPiece *)c->df_pieces.p, (uint32_t)pend[k].size(), ptiles[k], abuf[k], (const uint8_t *)c->df_dev[cur_q & 1].p, (unsigned long long *)c->df_first.p, st);
            HIPCHK(c, hipEventRecord(c->df_tev[c->df_tused + 1], st));
            HIPCHK(c, hipGetLastError());
            c->df_tused += 2;
            pend[k].clear(); ptiles[k] = 0;
        }
        return PNA_OK;
    }
    int finish_slot() {
        if (cur_q < 0) return PNA_OK;
        const int rc = flush(); if (rc) return rc;
        HIPCHK(c, hipEventRecord(c->df_ev_k[cur_q & 1], st));
        return PNA_OK;
    }
    int run(uint32_t upto) {                                          // the runs of the records up to `upto` (whose decoded bytes are where the records say)
        while (next < fp.size() && fp[next].rec <= upto) {
            const FPiece &p = fp[next];
            if ((int64_t)p.q != cur_q) {
                int rc = finish_slot(); if (rc) return rc;
                cur_q = (int64_t)p.q;
                if (staged < cur_q) { rc = stage((uint64_t)cur_q); if (rc) return rc; }
                HIPCHK(c, hipStreamWaitEvent(st, c->df_ev_cp[cur_q & 1], 0));
                if (staged < cur_q + 1 && (uint64_t)cur_q + 1 <= fp.back().q) { rc = stage((uint64_t)cur_q + 1); if (rc) return rc; }
            }
            const DRec &r = recs[p.rec];
            if (r.a_ready && p.base < r.a_len) {                     // (the decoded side may be shorter than the file: the rest is a length difference)
                const uint64_t n = std::min(p.len, r.a_len - p.base);
                const uint64_t tiles = (n + DIFF_TILE - 1) / DIFF_TILE;
                if ((uint64_t)ptiles[r.a_buf] + tiles > 0x7FFFFFFFu) { const int rc = flush(); if (rc) return rc; }
                pend[r.a_buf].push_back(DiffPiece{r.a_off + p.a_rel, p.b_off, n, p.base, p.rec, ptiles[r.a_buf]});
                ptiles[r.a_buf] += (uint32_t)tiles;
                c->df_bytes += n;
            }
            next++;
        }
        return PNA_OK;
    }
    int finish(std::vector<uint64_t> &first) {                        // everything launched: first[] back (the stream drained), k_diff's time
        int rc = run(0xFFFFFFFFu); if (rc) return rc;
        rc = finish_slot(); if (rc) return rc;
        rc = read_back(c, first.data(), c->df_first.p, first.size() * 8, st); if (rc) return rc;
        for (size_t k = 0; k + 1 < c->df_tused; k += 2) { float ms = 0; if (hipEventElapsedTime(&ms, c->df_tev[k], c->df_tev[k + 1]) == hipSuccess) c->df_ms += ms; }
        c->df_tused = 0;
        return PNA_OK;
    }
};
int emit_diff(XCall &x, DCall &d, const char *name, int kind, int status, int vstatus, uint32_t flags, uint64_t size, uint64_t first, const char *link) {
    d.sum.total++;
    if (status == PNA_DIFF_SAME) d.sum.same++;
    else if (status == PNA_DIFF_NOT_COMPARED) d.sum.not_compared++;
    else if (status == PNA_DIFF_SKIPPED) d.sum.skipped++;
    else if (status == PNA_DIFF_DAMAGED) d.sum.damaged++;
    else d.sum.differ++;
    if (d.cb(d.user, x.index++, name, kind, status, vstatus, flags, size, first, link) != 0) return fail(x.c, PNA_E_SINK, "diff callback failed");
    return PNA_OK;
}
// a record whose bytes were compared: SAME, or where the sides part
void compared(const DRec &r, int kind, uint64_t first, int *status, uint64_t *at) {
    const int differ = kind == 2 ? PNA_DIFF_SYMLINK_DIFFERS : PNA_DIFF_CONTENTS_DIFFER;
    *status = PNA_DIFF_SAME; *at = UINT64_MAX;
    if (first != UINT64_MAX) { *status = differ; *at = first; }
    else if (r.a_len != r.f.len) { *status = differ; *at = std::min<uint64_t>(r.a_len, r.f.len); }     // one side is a strict prefix of the other
}
int ask(XCall &x, DCall &d, size_t index, const std::string &raw_name, int kind, bool has_size, uint64_t raw_size, DRec &r) {
    r.named = entry_path(x.c, raw_name, r.path) == PNA_OK;
    if (!r.named) return PNA_OK;
    if (d.src(d.user, index, r.path.c_str(), kind, has_size ? raw_size : UINT64_MAX, &r.f) != 0) return fail(x.c, PNA_E_SINK, "diff source callback failed");
    if (r.f.fs_kind < PNA_DIFF_FS_MISSING || r.f.fs_kind > PNA_DIFF_FS_IGNORE) return fail(x.c, PNA_E_INVAL, "diff source callback: unknown fs_kind");
    if (r.f.len && !r.f.data && (r.f.fs_kind == PNA_DIFF_FS_FILE || r.f.fs_kind == PNA_DIFF_FS_SYMLINK)) return fail(x.c, PNA_E_INVAL, "diff source callback: bytes announced, none given");
    r.status = settle(kind, r.f, has_size, raw_size, &r.want_link);
    return PNA_OK;
}
// a solid block: one record for a block that is skipped or fails, else its inner entries against the decoded stream where it lies
int diff_solid(XCall &x, DCall &d, const XSolid &so, int status, uint32_t flag[2], hipStream_t st) {
    pna_gpu_ctx *c = x.c;
    std::vector<uint8_t> plain; std::vector<Inner> inner;
    if (status == PNA_VERIFY_OK) {
        int vst = 0;
        c->df_streams++;
        const int rc = walk_solid(c, so, plain, inner, flag, st, &vst); if (rc) return rc;
        status = vst;
    }
    if (status) return emit_diff(x, d, nullptr, PNA_VERIFY_KIND_SOLID, status == PNA_VERIFY_SKIPPED ? PNA_DIFF_SKIPPED : PNA_DIFF_DAMAGED, status, fail_flags(so, status), 0, UINT64_MAX, nullptr);
    std::vector<DRec> recs(inner.size());
    DiffFeed feed(c, st, recs);
    const bool stored = so.compression == PNA_ALGO_STORE;            // (a stored stream lies in the packed buffer)
    for (size_t k = 0; k < inner.size(); k++) {
        const Inner &ie = inner[k]; DRec &r = recs[k];
        int rc = ask(x, d, x.index + k, ie.name, ie.kind, ie.has_size, ie.raw_size, r); if (rc) return rc;
        if (!r.named) continue;
        if (r.want_link) for (const XPiece &p : ie.pieces) { if (r.link.size() < LINK_MAX) r.link.append((const char *)plain.data() + p.off, (size_t)std::min<uint64_t>(p.len, LINK_MAX - r.link.size())); }
        if (r.status != -1) continue;
        r.a_buf = stored ? 1 : 2; r.a_off = stored ? so.pk_off : 0; r.a_len = ie.len; r.a_ready = true;
        uint64_t base = 0;
        for (const XPiece &p : ie.pieces) {
            if (base < r.f.len) feed.add((uint32_t)k, p.off, base, std::min<uint64_t>(p.len, r.f.len - base), (const uint8_t *)r.f.data + base);
            base += p.len;
        }
    }
    std::vector<uint64_t> first(recs.size(), UINT64_MAX);
    if (!recs.empty()) {
        int rc = feed.init(recs.size()); if (rc) return rc;
        rc = feed.finish(first); if (rc) return rc;
    }
    for (size_t k = 0; k < inner.size(); k++) {
        const DRec &r = recs[k];
        int rc;
        if (!r.named) rc = emit_diff(x, d, nullptr, inner[k].kind, PNA_DIFF_DAMAGED, PNA_VERIFY_BAD_STRUCTURE, 0, 0, UINT64_MAX, nullptr);
        else if (r.status != -1) rc = emit_diff(x, d, r.path.c_str(), inner[k].kind, r.status, 0, 0, 0, UINT64_MAX, r.want_link ? r.link.c_str() : nullptr);
        else { int stt; uint64_t at; compared(r, inner[k].kind, first[k], &stt, &at); rc = emit_diff(x, d, r.path.c_str(), inner[k].kind, stt, 0, 0, inner[k].len, at, nullptr); }
        if (rc) return rc;
    }
    return PNA_OK;
}
int diff_window(XCall &x, DCall &d, const WinSrc &a, size_t span, std::vector<XEntry> &ents, std::vector<FrameDesc> &dchunks, std::vector<FrameDesc> &schunks,
                std::vector<XSolid> &solids) {
    pna_gpu_ctx *c = x.c;
    XPlan P;
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    uint32_t flag[2] = {0, 0};
    std::vector<uint32_t> vs;
    // 1. the filesystem side of every record, and what is settled without the entry's bytes
    std::vector<DRec> recs(ents.size());
    DiffFeed feed(c, st, recs);
    for (size_t i = 0; i < ents.size(); i++) {
        XEntry &e = ents[i]; DRec &r = recs[i];
        if (e.noname || e.kind == PNA_VERIFY_KIND_BROKEN) continue;
        int rc = ask(x, d, x.index + i, e.name, e.kind, e.has_size, e.raw_size, r); if (rc) return rc;
        if (!r.named) continue;
        e.nodecode = r.status != -1 && !r.want_link;
        if (r.status == -1 && r.f.len) feed.add((uint32_t)i, 0, 0, r.f.len, (const uint8_t *)r.f.data);     // (every normal entry's decoded bytes start at a multiple of 16)
    }
    int rc = PNA_OK;
    if (!ents.empty()) { rc = feed.init(ents.size()); if (rc) return rc; rc = feed.prefill(); if (rc) return rc; }
    // 2. upload, decryption, the fold, the sized decode: as verify
    rc = window_verdicts(x, a, span, ents, dchunks, schunks, solids, P, vs, flag, st); if (rc) return rc;
    if (!solids.empty()) return diff_solid(x, d, solids[0], (int)vs[0], flag, st);
    std::vector<uint64_t> size(ents.size(), 0); std::vector<size_t> open;
    rc = decode_sized_status(c, ents, vs, size, open, st, &c->df_streams); if (rc) return rc;
    for (size_t i : P.nosize_idx) if (!vs[i]) open.push_back(i);     // (entries without fSIZ, or with one out of proportion to their data)
    std::sort(open.begin(), open.end());
    // 3. the compare, in record order: an entry without a usable fSIZ is decoded into the open-decode buffer when its turn comes and compared before the next one overwrites it
    size_t oi = 0;
    for (size_t i = 0; i < ents.size(); i++) {
        XEntry &e = ents[i]; DRec &r = recs[i];
        if (vs[i] || e.nodecode || !r.named) continue;
        if (oi < open.size() && open[oi] == i) {
            oi++;
            rc = feed.flush(); if (rc) return rc;
            uint64_t got = 0;
            c->df_streams++;
            rc = decode_open(c, e, "entry buffer", nullptr, st, &got);
            if (rc == PNA_E_INVAL || rc == PNA_E_UNSUPPORTED) { vs[i] = rc == PNA_E_INVAL ? PNA_VERIFY_BAD_STREAM : PNA_VERIFY_UNSUPPORTED; continue; }
            if (rc) return rc;
            size[i] = got; r.a_buf = 2; r.a_off = 0;
        } else if (e.compression == PNA_ALGO_STORE) { size[i] = e.pay_len; r.a_buf = 1; r.a_off = e.pk_off; }
        else { r.a_buf = 0; r.a_off = e.raw_off; }                  // (decoded by decode_sized_status: size[i] = fSIZ)
        r.a_len = size[i]; r.a_ready = true;
        if (r.want_link && r.a_len) {
            r.link.resize((size_t)std::min<uint64_t>(r.a_len, LINK_MAX));
            const uint8_t *src = (const uint8_t *)(r.a_buf == 0 ? c->x_raw[0].p : r.a_buf == 1 ? c->x_pk.p : c->solid_plain.p) + r.a_off;
            rc = read_back(c, &r.link[0], src, r.link.size(), st); if (rc) return rc;
        }
        rc = feed.run((uint32_t)i); if (rc) return rc;
    }
    std::vector<uint64_t> first(ents.size(), UINT64_MAX);
    if (!ents.empty()) { rc = feed.finish(first); if (rc) return rc; }
    // 4. the records
    for (size_t i = 0; i < ents.size(); i++) {
        const XEntry &e = ents[i]; const DRec &r = recs[i];
        const int v = (int)vs[i];
        const char *name = r.named ? r.path.c_str() : nullptr;
        if (!r.named) rc = emit_diff(x, d, nullptr, e.kind, v == PNA_VERIFY_SKIPPED ? PNA_DIFF_SKIPPED : PNA_DIFF_DAMAGED, v ? v : PNA_VERIFY_BAD_STRUCTURE, v ? fail_flags(e, v) : 0u, 0, UINT64_MAX, nullptr);
        else if (e.nodecode) rc = emit_diff(x, d, name, e.kind, r.status, v, 0, 0, UINT64_MAX, nullptr);                 // (v: what the chunk CRCs and the walk found)
        else if (v) rc = emit_diff(x, d, name, e.kind, v == PNA_VERIFY_SKIPPED ? PNA_DIFF_SKIPPED : PNA_DIFF_DAMAGED, v, fail_flags(e, v), 0, UINT64_MAX, nullptr);
        else if (r.want_link) rc = emit_diff(x, d, name, e.kind, PNA_DIFF_NOT_COMPARED, 0, 0, size[i], UINT64_MAX, r.link.c_str());
        else { int stt; uint64_t at; compared(r, e.kind, first[i], &stt, &at); rc = emit_diff(x, d, name, e.kind, stt, 0, 0, size[i], at, nullptr); }
        if (rc) return rc;
    }
    return PNA_OK;
}
}

extern "C" int pna_gpu_diff_archive_host(pna_gpu_ctx *c, const void *const *parts, const size_t *part_len, size_t n_parts, const void *password,
                                         size_t password_len, pna_diff_source_fn source, pna_diff_fn cb, void *user, pna_diff_summary *summary) {
    if (!c || !parts || !part_len || !n_parts || !source || !cb || (!password && password_len)) return fail(c, PNA_E_INVAL, "null argument");
    for (size_t k = 0; k < n_parts; k++) if (!parts[k]) return fail(c, PNA_E_INVAL, "null argument");
    if (part_len[0] < 8 || memcmp(parts[0], PNA_SIGNATURE, 8) != 0) return fail(c, PNA_E_INVAL, "not a PNA archive");
    if (!launch_frame_verdict || !launch_verdict || !launch_gcm_verdict || !launch_diff) return fail(c, PNA_E_UNSUPPORTED, "this build has no verdict / diff kernels");
    ArcParts ap{(const uint8_t *const *)parts, part_len, n_parts, {}};
    uint64_t at = 0;
    for (size_t k = 0; k < n_parts; k++) { ap.vb.push_back(at); at += part_len[k]; }
    XCall x{c, password, password_len, nullptr, nullptr, {}, 0};
    x.verdict = true;
    DCall d{source, cb, user};
    c->df_streams = 0; c->df_bytes = 0; c->df_ms = 0; c->df_tused = 0;
    std::vector<XEntry> ents; std::vector<FrameDesc> dchunks, schunks; std::vector<XSolid> solids;
    bool broken = false;
    int rc = walk_archive(c, ap, true, ents, dchunks, schunks, solids, &broken);
    size_t si = 0, w0 = 0;
    while (rc == PNA_OK && (w0 < ents.size() || si < solids.size())) {
        XWindow W;
        next_window(c, ents, dchunks, schunks, solids, w0, si, W);
        rc = diff_window(x, d, WinSrc{&ap, W.base}, (size_t)W.span, W.we, W.wd, W.ws, W.wso);
    }
    if (rc) (void)hipDeviceSynchronize();                               // (nothing of a window that failed is left in flight: the host's buffers are its own again)
    if (rc == PNA_OK && broken) { d.sum.broken = 1; rc = fail(c, PNA_E_INVAL, "archive structure is broken; diff aborted"); }
    if (summary) *summary = d.sum;
    return rc;
}
extern "C" int pna_gpu_debug_diff_stats(pna_gpu_ctx *c, uint64_t *decoded_streams, uint64_t *compared_bytes, double *ms_k_diff) {
    if (!c) return PNA_E_INVAL;
    if (decoded_streams) *decoded_streams = c->df_streams;
    if (compared_bytes) *compared_bytes = c->df_bytes;
    if (ms_k_diff) *ms_k_diff = c->df_ms;
    return PNA_OK;
}

// ---- pna_gpu_extract_select_host: extract for the entries the host chooses, to host memory or to device memory of the caller's.  The stages above in
// extract's (strict) mode over windows of its own making: `select` is asked for every entry in archive order, and a window holds the selected entries
// only -- its H2D copies are the runs pna_extract_plan_runs makes of their records (all records that have data chunks under PNA_EXTRACT_CHECK_ALL), laid
// one behind the other in the window buffer, and it is cut by the bytes it uploads, packs and decodes, not by the archive span it reaches over.  The
// decoders write into the window buffers as ever; k_pick carries DEVICE entries from there to their destinations (one launch per window and source
// buffer: the raw buffer, the packed buffer for stored entries; an entry without fSIZ is decoded into the open-decode buffer and picked from there
// before the next one overwrites it), HOST entries travel through page-locked memory, and the window's records follow once the stream has drained.
// A solid block is a window of its own, uploaded and decoded whole BEFORE anything is known to be wanted from it -- its inner entries' names lie in
// the decoded stream -- and copied to the host once for its header walk (walk_solid); HOST records point into that copy, DEVICE records are picked
// from the decoded stream where it lies.  Windows are not pipelined against each other here (extract's deferred hand-out): a callback may use d_dst,
// so a window's records wait for its kernels anyway.
constexpr uint64_t EXTRACT_GAP_MAX = PNA_EXTRACT_GAP_MAX;      // see include/pna_gpu.h
extern "C" int pna_extract_plan_runs(const uint64_t *rec_off, const uint64_t *rec_len, const uint8_t *wanted, size_t n, uint64_t gap_max,
                                     uint64_t *run_off, uint64_t *run_len, size_t *n_runs) {
    if (!n_runs || (n && (!rec_off || !rec_len || !wanted))) return PNA_E_INVAL;
    size_t k = 0; uint64_t start = 0, end = 0;
    for (size_t i = 0; i < n; i++) {
        if (rec_off[i] + rec_len[i] < rec_off[i] || (i && rec_off[i] < rec_off[i - 1] + rec_len[i - 1])) return PNA_E_INVAL;      // records in archive order, none inside another
        if (!wanted[i] || !rec_len[i]) continue;
        if (k && rec_off[i] - end <= gap_max) end = rec_off[i] + rec_len[i];                 // the gap travels with its neighbours
        else { start = rec_off[i]; end = start + rec_len[i]; k++; if (run_off) run_off[k - 1] = start; }
        if (run_len) run_len[k - 1] = end - start;
    }
    *n_runs = k;
    return PNA_OK;
}
namespace {
struct SCall { pna_extract_select_fn sel; pna_extract_record_fn cb; void *user; bool check_all; pna_extract_summary sum{}; };
// a record of a window: what `select` said, where the entry's bytes are handed out
struct SRec {
    size_t index = 0; std::string path; int kind = 0; pna_extract_dest d{PNA_EXTRACT_SKIP, nullptr, 0};
    int ei = -1;                                                 // its entry in the window's list (-1: a data-less record, or an inner entry of a solid stream)
    int status = PNA_EXTRACT_OK; uint64_t len = 0;
    const uint8_t *host = nullptr; bool staged = false; uint64_t hoff = 0; std::vector<uint8_t> own;      // HOST: bytes in the caller's view / in the page-locked slot at hoff / of its own
};
int ask_select(XCall &x, SCall &s, const std::string &raw_name, int kind, bool has_size, uint64_t raw_size, SRec &r) {
    int rc = entry_path(x.c, raw_name, r.path); if (rc) return rc;
    r.index = x.index++; r.kind = kind; r.d = pna_extract_dest{PNA_EXTRACT_SKIP, nullptr, 0};
    if (s.sel(s.user, r.index, r.path.c_str(), kind, has_size ? raw_size : UINT64_MAX, &r.d) != 0) return fail(x.c, PNA_E_SINK, "select callback failed");
    if (r.d.where < PNA_EXTRACT_SKIP || r.d.where > PNA_EXTRACT_DEVICE) return fail(x.c, PNA_E_INVAL, "select callback: unknown destination");
    if (r.d.where == PNA_EXTRACT_DEVICE && !r.d.d_dst && r.d.cap) return fail(x.c, PNA_E_INVAL, "select callback: device destination announced, none given");
    s.sum.total++;
    if (r.d.where != PNA_EXTRACT_SKIP) s.sum.selected++;
    return PNA_OK;
}
// k_pick's launches: pieces of one source buffer are collected and go out together
struct PickList {
    pna_gpu_ctx *c; hipStream_t st; const uint8_t *src = nullptr; std::vector<PickPiece> pend; uint32_t tiles = 0;
    int flush() {
        if (pend.empty()) return PNA_OK;
        if (c->xs_pieces.ensure(pend.size() * sizeof(PickPiece) + 16)) return fail(c, PNA_E_NOMEM, "extract workspace");
        while (c->xs_tev.size() < c->xs_tused + 2) { hipEvent_t e; HIPCHK(c, hipEventCreate(&e)); c->xs_tev.push_back(e); }
        HIPCHK(c, hipMemcpyAsync(c->xs_pieces.p, pend.data(), pend.size() * sizeof(PickPiece), hipMemcpyHostToDevice, st));
        HIPCHK(c, hipEventRecord(c->xs_tev[c->xs_tused], st));
        // every load of k_pick stays inside the source range rounded out to 16 bytes: the window buffers (x_raw, x_pk, solid_plain) start at a multiple of
        // 16 and are allocated with at least 64 bytes behind the last entry
        launch_pick((const PickPiece *)c->xs_pieces.p, (uint32_t)pend.size(), tiles, src, st);
        HIPCHK(c, hipEventRecord(c->xs_tev[c->xs_tused + 1], st));
        HIPCHK(c, hipGetLastError());
        c->xs_tused += 2;
        pend.clear(); tiles = 0;
        return PNA_OK;
    }
    int add(const void *buf, uint64_t off, void *dst, uint64_t len) {
        if (!len) return PNA_OK;
        const uint64_t t = (len + PICK_TILE - 1) / PICK_TILE;
        if (t > 0x7FFFFFFFu) return fail(c, PNA_E_UNSUPPORTED, "entry too large for one k_pick launch");
        if ((buf != src && !pend.empty()) || (uint64_t)tiles + t > 0x7FFFFFFFu) { const int rc = flush(); if (rc) return rc; }
        src = (const uint8_t *)buf;
        pend.push_back(PickPiece{off, (uint8_t *)dst, len, tiles, 0});
        tiles += (uint32_t)t; c->xs_picked += len;
        return PNA_OK;
    }
    int finish() {                                                  // the last launch, the stream drained, k_pick's time
        const int rc = flush(); if (rc) return rc;
        HIPCHK(c, hipStreamSynchronize(st));
        for (size_t k = 0; k + 1 < c->xs_tused; k += 2) { float ms = 0; if (hipEventElapsedTime(&ms, c->xs_tev[k], c->xs_tev[k + 1]) == hipSuccess) c->xs_ms += ms; }
        c->xs_tused = 0;
        return PNA_OK;
    }
};
// HOST entries on their way back: ranges of the device buffers into one page-locked slot, neighbours in one copy
struct HostCopies {
    struct Job { const uint8_t *buf; uint64_t off, len, hoff; };
    std::vector<Job> jobs; uint64_t total = 0;
    uint64_t add(const void *buf, uint64_t off, uint64_t len) {
        if (!jobs.empty()) {
            Job &j = jobs.back();
            if (j.buf == buf && off >= j.off + j.len && off <= ((j.off + j.len + 15) & ~(uint64_t)15)) { j.len = off + len - j.off; total = j.hoff + j.len; return j.hoff + (off - j.off); }
        }
        const uint64_t h = (total + 15) & ~(uint64_t)15;
        jobs.push_back(Job{(const uint8_t *)buf, off, len, h}); total = h + len;
        return h;
    }
    int issue(pna_gpu_ctx *c, hipStream_t st) {
        if (c->hp_out[0].ensure(total + 64)) return fail(c, PNA_E_NOMEM, "staging allocation failed");
        for (const Job &j : jobs) if (j.len) HIPCHK(c, hipMemcpyAsync((uint8_t *)c->hp_out[0].p + j.hoff, j.buf + j.off, j.len, hipMemcpyDeviceToHost, st));
        return PNA_OK;
    }
};
// where a selected entry's `size` decoded bytes at buf + off go: a pick, a copy to the host, or nowhere (TOO_SMALL)
int route(pna_gpu_ctx *c, SRec &r, const void *buf, uint64_t off, uint64_t size, PickList &picks, HostCopies &hc) {
    r.len = size;
    if (r.d.where == PNA_EXTRACT_DEVICE) {
        if (r.d.cap < size) { r.status = PNA_EXTRACT_TOO_SMALL; return PNA_OK; }
        return picks.add(buf, off, r.d.d_dst, size);
    }
    if (size) { r.hoff = hc.add(buf, off, size); r.staged = true; }
    return PNA_OK;
}
int emit_records(XCall &x, SCall &s, std::vector<SRec> &recs) {
    pna_gpu_ctx *c = x.c;
    for (SRec &r : recs) {
        const void *data = nullptr;
        if (r.d.where == PNA_EXTRACT_DEVICE) {
            if (r.status == PNA_EXTRACT_TOO_SMALL) s.sum.too_small++; else { s.sum.to_device++; data = r.d.d_dst; }
        } else {
            s.sum.to_host++;
            if (r.len) data = r.staged ? (const uint8_t *)c->hp_out[0].p + r.hoff : r.host;
        }
        if (s.cb(s.user, r.index, r.path.c_str(), r.kind, r.status, data, r.len) != 0) return fail(c, PNA_E_SINK, "record callback failed");
    }
    return PNA_OK;
}
// a window of selected normal entries: `ents` are the entries recs[].ei name, `chunks` the data chunks to check, offsets relative to the packed window
int select_window(XCall &x, SCall &s, const WinSrc &a, uint64_t win_len, std::vector<XEntry> &ents, std::vector<FrameDesc> &chunks, std::vector<SRec> &recs) {
    pna_gpu_ctx *c = x.c;
    XPlan P; std::vector<XSolid> no_solid; std::vector<FrameDesc> no_sdat;
    int rc = plan_window(x, a, ents, no_solid, P); if (rc) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    uint32_t flag[2] = {0, 0};
    rc = upload_window(c, a, (size_t)win_len, chunks, no_sdat, P, 0, flag, st); if (rc) return rc;
    if (flag[0]) { c->err = "data chunk CRC mismatch (" + std::to_string(flag[0]) + " FDAT chunks)"; return PNA_E_INVAL; }
    rc = derive_ahead_plan(x, P.enc_list, P.gcm_list); if (rc) return rc;
    if (!P.enc_list.empty()) { rc = decrypt_ctr_cbc(x, P.enc_list, st); if (rc) return rc; }
    if (!P.gcm_list.empty()) { rc = decrypt_gcm(x, a, P.gcm_list, flag, st); if (rc) return rc; }
    rc = decode_sized(c, ents, 0, st); if (rc) return rc;
    c->xs_streams += ents.size();                                     // (a stored entry's decode is the identity)
    PickList picks{c, st}; HostCopies hc;
    std::vector<bool> open(ents.size(), false);
    for (size_t i : P.nosize_idx) open[i] = true;
    for (int pass = 0; pass < 2; pass++)                              // the raw buffer's entries, then the packed buffer's: one k_pick launch each
        for (SRec &r : recs) {
            if (r.ei < 0 || open[(size_t)r.ei]) continue;
            const XEntry &e = ents[(size_t)r.ei];
            const bool stored = e.compression == PNA_ALGO_STORE;
            if (stored != (pass == 1)) continue;
            if (stored && e.has_size && e.raw_size != e.pay_len) return fail(c, PNA_E_INVAL, "stored entry: fSIZ differs from the data length");
            rc = stored ? route(c, r, c->x_pk.p, e.pk_off, e.pay_len, picks, hc) : route(c, r, c->x_raw[0].p, e.raw_off, e.raw_size, picks, hc);
            if (rc) return rc;
        }
    for (SRec &r : recs) {                                            // entries without fSIZ: measured and decoded one by one, as extract does
        if (r.ei < 0 || !open[(size_t)r.ei]) continue;
        const XEntry &e = ents[(size_t)r.ei];
        if (r.d.where == PNA_EXTRACT_HOST) { rc = decode_open(c, e, "entry buffer", &r.own, st); if (rc) return rc; r.len = r.own.size(); r.host = r.own.data(); continue; }
        uint64_t got = 0;
        rc = decode_open(c, e, "entry buffer", nullptr, st, &got); if (rc) return rc;
        rc = route(c, r, c->solid_plain.p, 0, got, picks, hc); if (rc) return rc;
        rc = picks.flush(); if (rc) return rc;                       // (before the next entry is decoded into the same buffer)
    }
    rc = hc.issue(c, st); if (rc) return rc;
    rc = picks.finish(); if (rc) return rc;
    return emit_records(x, s, recs);
}
// a solid block: uploaded, decrypted, decoded and walked as extract does; then the question for every inner entry
int select_solid(XCall &x, SCall &s, const WinSrc &a, size_t span, std::vector<FrameDesc> &schunks, std::vector<XSolid> &solids) {
    pna_gpu_ctx *c = x.c;
    XPlan P; std::vector<XEntry> no_ents; std::vector<FrameDesc> no_fdat;
    int rc = plan_window(x, a, no_ents, solids, P); if (rc) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    uint32_t flag[2] = {0, 0};
    rc = upload_window(c, a, span, no_fdat, schunks, P, 0, flag, st); if (rc) return rc;
    if (flag[0]) { c->err = "data chunk CRC mismatch (" + std::to_string(flag[0]) + " SDAT chunks)"; return PNA_E_INVAL; }
    rc = derive_ahead_plan(x, P.enc_list, P.gcm_list); if (rc) return rc;
    if (!P.enc_list.empty()) { rc = decrypt_ctr_cbc(x, P.enc_list, st); if (rc) return rc; }
    if (!P.gcm_list.empty()) { rc = decrypt_gcm(x, a, P.gcm_list, flag, st); if (rc) return rc; }
    const XSolid &so = solids[0];
    std::vector<uint8_t> plain; std::vector<Inner> inner;
    c->xs_streams++;
    rc = walk_solid(c, so, plain, inner, flag, st); if (rc) return rc;
    const bool stored = so.compression == PNA_ALGO_STORE;            // (a stored stream lies in the packed buffer)
    const void *buf = stored ? c->x_pk.p : c->solid_plain.p; const uint64_t base = stored ? so.pk_off : 0;
    PickList picks{c, st};
    std::vector<SRec> recs;
    for (const Inner &ie : inner) {
        SRec r;
        rc = ask_select(x, s, ie.name, ie.kind, ie.has_size, ie.raw_size, r); if (rc) return rc;
        if (r.d.where == PNA_EXTRACT_SKIP) continue;
        r.len = ie.len;
        if (r.d.where == PNA_EXTRACT_HOST) {
            if (ie.pieces.size() == 1) r.host = plain.data() + ie.pieces[0].off;
            else { for (const XPiece &p : ie.pieces) r.own.insert(r.own.end(), plain.data() + p.off, plain.data() + p.off + p.len); r.host = r.own.data(); }
        } else if (r.d.cap < ie.len) r.status = PNA_EXTRACT_TOO_SMALL;
        else {
            uint64_t at = 0;
            for (const XPiece &p : ie.pieces) { rc = picks.add(buf, base + p.off, (uint8_t *)r.d.d_dst + at, p.len); if (rc) return rc; at += p.len; }
        }
        recs.push_back(std::move(r));
    }
    rc = picks.finish(); if (rc) return rc;
    return emit_records(x, s, recs);
}
}

extern "C" int pna_gpu_extract_select_host(pna_gpu_ctx *c, const void *const *parts, const size_t *part_len, size_t n_parts, const void *password,
                                           size_t password_len, uint32_t xflags, pna_extract_select_fn select, pna_extract_record_fn cb, void *user,
                                           pna_extract_summary *summary) {
    if (!c || !parts || !part_len || !n_parts || !select || !cb || (!password && password_len)) return fail(c, PNA_E_INVAL, "null argument");
    if (xflags & ~(uint32_t)PNA_EXTRACT_CHECK_ALL) return fail(c, PNA_E_INVAL, "unknown extract flag");
    for (size_t k = 0; k < n_parts; k++) if (!parts[k]) return fail(c, PNA_E_INVAL, "null argument");
    if (part_len[0] < 8 || memcmp(parts[0], PNA_SIGNATURE, 8) != 0) return fail(c, PNA_E_INVAL, "not a PNA archive");
    if (!launch_pick) return fail(c, PNA_E_UNSUPPORTED, "this build has no pick kernel");
    ArcParts ap{(const uint8_t *const *)parts, part_len, n_parts, {}};
    uint64_t at = 0;
    for (size_t k = 0; k < n_parts; k++) { ap.vb.push_back(at); at += part_len[k]; }
    XCall x{c, password, password_len, nullptr, nullptr, {}, 0};
    SCall s{select, cb, user, (xflags & PNA_EXTRACT_CHECK_ALL) != 0};
    c->xs_uploaded = 0; c->xs_streams = 0; c->xs_kdf = 0; c->xs_picked = 0; c->xs_ms = 0; c->xs_tused = 0;
    std::vector<XEntry> ents; std::vector<FrameDesc> dchunks, schunks; std::vector<XSolid> solids;
    bool broken = false;
    int rc = walk_archive(c, ap, false, ents, dchunks, schunks, solids, &broken, true);
    const uint64_t WIN = (uint64_t)c->tun.extract_win_mib << 20;
    size_t si = 0, w0 = 0;
    SRec carry; bool carried = false;                                 // the entry that did not fit the previous window: asked already
    while (rc == PNA_OK && (w0 < ents.size() || si < solids.size())) {
        if (si < solids.size() && solids[si].order <= w0) {
            XWindow W;
            next_window(c, ents, dchunks, schunks, solids, w0, si, W);
            rc = select_solid(x, s, WinSrc{&ap, W.base}, (size_t)W.span, W.ws, W.wso);
            continue;
        }
        // the next window: entries are asked about in archive order until what is wanted of them fills it
        const size_t stop = si < solids.size() ? std::min(ents.size(), solids[si].order) : ents.size();
        std::vector<XEntry> we; std::vector<FrameDesc> wd; std::vector<SRec> recs;
        struct Need { uint64_t lo, len; size_t c0, c1; int ei; };      // a record that travels: its bytes, its chunks in wd, its entry in we (-1: checked only)
        std::vector<Need> need;
        uint64_t up = 0, raw = 0, pk = 0;
        while (rc == PNA_OK && w0 < stop) {
            XEntry &e = ents[w0];
            SRec r;
            if (carried) { r = std::move(carry); carried = false; }
            else { rc = ask_select(x, s, e.name, e.kind, e.has_size, e.raw_size, r); if (rc) break; }
            const bool sel = r.d.where != PNA_EXTRACT_SKIP, dataless = e.kind != 0 && e.pieces.empty();
            if ((sel && !dataless) || (s.check_all && e.d1 > e.d0)) {
                const bool dec = sel && !dataless;
                const uint64_t b = e.hi - e.lo, rr = dec && e.has_size ? e.raw_size : 0, pp = dec ? e.stream_len : 0;
                if (!need.empty() && (up + b > WIN || raw + rr > 3 * WIN || pk + pp > WIN)) { carry = std::move(r); carried = true; break; }
                up += b; raw += rr; pk += pp;
                need.push_back(Need{e.lo, b, wd.size(), wd.size() + (e.d1 - e.d0), dec ? (int)we.size() : -1});
                wd.insert(wd.end(), dchunks.begin() + e.d0, dchunks.begin() + e.d1);
                if (dec) { r.ei = (int)we.size(); we.push_back(std::move(e)); }
            }
            if (sel) recs.push_back(std::move(r));
            w0++;
        }
        if (rc) break;
        // the runs that travel, laid one behind the other (each at a multiple of 16), and everything of the window moved to where its run lies
        std::vector<uint64_t> ro, rl, run_off(need.size()), run_len(need.size()); size_t nr = 0;
        for (const Need &q : need) { ro.push_back(q.lo); rl.push_back(q.len); }
        const std::vector<uint8_t> all(need.size(), 1);
        rc = pna_extract_plan_runs(ro.data(), rl.data(), all.data(), need.size(), EXTRACT_GAP_MAX, run_off.data(), run_len.data(), &nr);
        if (rc) { rc = fail(c, PNA_E_INVAL, "entries out of order"); break; }
        std::vector<XRun> runs; uint64_t win_len = 0;
        for (size_t k = 0; k < nr; k++) { runs.push_back(XRun{win_len, run_off[k], run_len[k]}); win_len = (win_len + run_len[k] + 15) & ~(uint64_t)15; }
        size_t k = 0;
        for (const Need &q : need) {
            while (k + 1 < nr && q.lo >= runs[k + 1].arc) k++;
            const uint64_t delta = runs[k].arc - runs[k].dev;
            for (size_t j = q.c0; j < q.c1; j++) wd[j].arc_off -= delta;
            if (q.ei >= 0) for (XPiece &p : we[(size_t)q.ei].pieces) p.off -= delta;
        }
        if (need.empty() && recs.empty()) continue;
        rc = select_window(x, s, WinSrc{&ap, 0, &runs}, win_len, we, wd, recs);
    }
    c->xs_kdf = x.kdf_runs;
    if (rc) (void)hipDeviceSynchronize();                               // (nothing of a window that failed is left in flight)
    if (summary) *summary = s.sum;
    return rc;
}
extern "C" int pna_gpu_debug_extract_stats(pna_gpu_ctx *c, uint64_t *uploaded_bytes, uint64_t *decoded_streams, uint64_t *kdf_runs, uint64_t *picked_bytes,
                                           double *ms_k_pick) {
    if (!c) return PNA_E_INVAL;
    if (uploaded_bytes) *uploaded_bytes = c->xs_uploaded;
    if (decoded_streams) *decoded_streams = c->xs_streams;
    if (kdf_runs) *kdf_runs = c->xs_kdf;
    if (picked_bytes) *picked_bytes = c->xs_picked;
    if (ms_k_pick) *ms_k_pick = c->xs_ms;
    return PNA_OK;
}
extern "C" int pna_gpu_debug_pick_device(pna_gpu_ctx *c, size_t n, const void *d_src, const uint64_t *src_off, void *const *d_dst, const uint64_t *len,
                                         void *hip_stream) {
    if (!c || (n && (!d_src || !src_off || !d_dst || !len))) return fail(c, PNA_E_INVAL, "null argument");
    for (size_t i = 0; i < n; i++) if (len[i] && !d_dst[i]) return fail(c, PNA_E_INVAL, "null argument");
    if (!launch_pick) return fail(c, PNA_E_UNSUPPORTED, "this build has no pick kernel");
    HIPCHK(c, hipSetDevice(c->device));
    c->xs_picked = 0; c->xs_ms = 0; c->xs_tused = 0;
    PickList picks{c, hip_stream ? (hipStream_t)hip_stream : c->stream};
    for (size_t i = 0; i < n; i++) { const int rc = picks.add(d_src, src_off[i], d_dst[i], len[i]); if (rc) return rc; }
    return picks.finish();                                              // (drains the stream: the counters above hold this call's bytes and time)
}
