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
};
struct XEntry : XStream {
    std::string name; int kind = 0;
    bool has_size = false; uint64_t raw_size = 0, raw_off = 0; // fSIZ; decoded bytes in the raw buffer
    size_t d0 = 0, d1 = 0;                                     // its FDAT chunks in the descriptor list
};
struct XSolid : XStream {                                      // SHED [PHSF] SDAT* SEND -- lib/src/entry.rs:465-484,567-583
    size_t order = 0;                                          // number of normal entries in front of it
    size_t s0 = 0, s1 = 0;                                     // its SDAT chunks in the descriptor list
};
struct Inner { std::string name; int kind; std::vector<XPiece> pieces; uint64_t len; };     // an entry of a decoded solid stream
// one call of the driver: the caller's arguments, the keys derived so far (one derivation per distinct PHSF string), the next entry's index
struct XCall {
    pna_gpu_ctx *c; const void *password; size_t password_len; pna_entry_fn cb; void *user;
    std::vector<std::pair<std::string, std::vector<uint8_t>>> keys; size_t index = 0;
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
uint32_t max_chunk_len(const std::vector<FrameDesc> &v) {      // the longest data chunk of a list (0: none below 16 380 bytes, the wave-per-chunk CRC kernel's limit)
    uint32_t m = 1;
    for (const FrameDesc &d : v) { if (d.payload_len > 16380u) return 0u; m = std::max(m, d.payload_len); }
    return m;
}
// bytes [lo, lo + n) of a data stream whose pieces lie in `a` (a prefix or a tag may span pieces: prepend_data_prefix makes the prefix a piece of its own)
void stream_read(const uint8_t *a, const std::vector<XPiece> &pieces, uint64_t lo, uint64_t n, uint8_t *out) {
    uint64_t at = 0;
    for (const XPiece &p : pieces) {
        if (!n) break;
        if (lo < at + p.len) { const uint64_t k = lo - at, m = std::min<uint64_t>(n, p.len - k); memcpy(out, a + p.off + k, m); out += m; lo += m; n -= m; }
        at += p.len;
    }
}
}

// The key of a PHSF string, derived once per call: "$argon2id$v=19$m=<KiB>,t=<passes>,p=<lanes>$<salt>" (argon2 0.5: Params::try_from(&PasswordHash),
// lib/src/hash.rs:56-70) or "$pbkdf2-sha256$i=<rounds>,l=<len>$<salt>" (derive_password_hash, lib/src/hash.rs:47-88)
static int phsf_key(XCall &x, const std::string &phsf, const uint8_t **out) {
    pna_gpu_ctx *c = x.c;
    for (auto &k : x.keys) if (k.first == phsf) { *out = k.second.data(); return PNA_OK; }
    int kind = -1; size_t p1 = 15, p2 = 0;                        // kind: the argon2 variant, -1 for pbkdf2-sha256
    uint32_t m = 19456, t = 2, lanes = 1, rounds = 600000;      // argon2 0.5 and pbkdf2 0.12 defaults
    if (phsf.rfind("$argon2", 0) == 0) {
        if (phsf.rfind("$argon2id$", 0) == 0) { kind = 2; p1 = 10; } else if (phsf.rfind("$argon2i$", 0) == 0) { kind = 1; p1 = 9; } else if (phsf.rfind("$argon2d$", 0) == 0) { kind = 0; p1 = 9; }
        if (kind < 0) return fail(c, PNA_E_INVAL, "malformed PHSF");
        if (phsf.compare(p1, 2, "v=") == 0) { const size_t q = phsf.find('$', p1); if (q == std::string::npos || strtoul(phsf.c_str() + p1 + 2, nullptr, 10) != 19) return fail(c, PNA_E_UNSUPPORTED, "argon2 version other than 0x13"); p1 = q + 1; }
        p2 = phsf.find('$', p1);
        if (p2 == std::string::npos) return fail(c, PNA_E_INVAL, "malformed PHSF");
        const std::string prm = phsf.substr(p1, p2 - p1);
        for (size_t q = 0; q < prm.size();) {
            const size_t e2 = prm.find(',', q); const std::string kv = prm.substr(q, e2 == std::string::npos ? std::string::npos : e2 - q);
            if (kv.size() > 2 && kv[1] == '=') {
                char *endp = nullptr; const unsigned long long v = strtoull(kv.c_str() + 2, &endp, 10);
                if (!endp || *endp || endp == kv.c_str() + 2) return fail(c, PNA_E_INVAL, "malformed argon2 parameter in PHSF");
                // the parameters come from an untrusted archive: refuse costs that only serve to stall / exhaust the host
                if ((kv[0] == 'm' && v > (4ull << 20)) || (kv[0] == 't' && v > 64) || (kv[0] == 'p' && v > 256)) return fail(c, PNA_E_UNSUPPORTED, "argon2 cost beyond the accepted maximum (m <= 4 GiB, t <= 64, p <= 256)");
                if (kv[0] == 'm') m = (uint32_t)v; else if (kv[0] == 't') t = (uint32_t)v; else if (kv[0] == 'p') lanes = (uint32_t)v;
            }
            if (e2 == std::string::npos) break; q = e2 + 1;
        }
    } else {
        if (phsf.rfind("$pbkdf2-sha256$", 0) != 0) return fail(c, PNA_E_UNSUPPORTED, "password hash other than argon2 / pbkdf2-sha256");
        p2 = phsf.find('$', p1);
        if (p2 == std::string::npos) return fail(c, PNA_E_INVAL, "malformed PHSF");
        const std::string prm = phsf.substr(p1, p2 - p1);
        const size_t ip = prm.find("i=");
        if (ip != std::string::npos) {
            char *endp = nullptr; const unsigned long long v = strtoull(prm.c_str() + ip + 2, &endp, 10);
            if (!endp || (*endp && *endp != ',') || v == 0) return fail(c, PNA_E_INVAL, "malformed pbkdf2 round count in PHSF");
            if (v > 10000000ull) return fail(c, PNA_E_UNSUPPORTED, "pbkdf2 round count beyond the accepted maximum (10 000 000)");
            rounds = (uint32_t)v;
        }
    }
    std::string sb = phsf.substr(p2 + 1); const size_t p3 = sb.find('$'); if (p3 != std::string::npos) sb.resize(p3);
    std::vector<uint8_t> key(32), salt;
    if (!b64_decode_nopad(sb, salt)) return fail(c, PNA_E_INVAL, "malformed PHSF");
    const int rc = kind >= 0 ? pna_kdf_argon2(kind, x.password, x.password_len, salt.data(), salt.size(), t, m, lanes, key.data(), 32)
                             : pna_kdf_pbkdf2_sha256(x.password, x.password_len, salt.data(), salt.size(), rounds, key.data(), 32, nullptr, 0);
    if (rc) return fail(c, rc, kind >= 0 ? "key derivation failed (argon2 parameters)" : "key derivation failed");
    x.keys.emplace_back(phsf, std::move(key)); *out = x.keys.back().second.data();
    return PNA_OK;
}

// ---- 1. the chunk walk (host): structure, small-chunk CRCs, data-chunk descriptors
static int walk_archive(pna_gpu_ctx *c, const uint8_t *a, size_t archive_len, std::vector<XEntry> &ents, std::vector<FrameDesc> &dchunks,
                        std::vector<FrameDesc> &schunks, std::vector<XSolid> &solids) {
    XSolid scur; bool in_solid = false;
    XEntry cur; bool in_entry = false, seen_ahed = false, ended = false;
    size_t pos = 8;
    while (pos < archive_len) {
        PnaChunk ch;
        const int r = next_chunk(a, archive_len, pos, ch);          // (pos moves behind the chunk)
        if (r) return fail(c, PNA_E_INVAL, r == CHUNK_SHORT_HEADER ? "truncated chunk header" : "truncated chunk body");
        const bool is_fdat = memcmp(ch.type, "FDAT", 4) == 0, is_sdat = memcmp(ch.type, "SDAT", 4) == 0;
        if (is_fdat || is_sdat) { if (ch.len > 0xFFFFFFFBu) return fail(c, PNA_E_INVAL, "data chunk too long"); (is_fdat ? dchunks : schunks).push_back(FrameDesc{ch.off, ch.len, 0, 8, 0}); }
        else if (!chunk_crc_ok(ch)) return fail(c, PNA_E_INVAL, "chunk CRC mismatch");
        if (!seen_ahed) {
            if (memcmp(ch.type, "AHED", 4) != 0 || ch.len != 8 || ch.data[0] != 0) return fail(c, PNA_E_INVAL, "first chunk must be AHED (major version 0)");
            seen_ahed = true;
        } else if (memcmp(ch.type, "AEND", 4) == 0) { ended = true; break; }
        else if (memcmp(ch.type, "ANXT", 4) == 0) return fail(c, PNA_E_UNSUPPORTED, "multipart archives are not read by this driver");
        else if (memcmp(ch.type, "SHED", 4) == 0) {
            if (in_entry || in_solid || ch.len != 5 || ch.data[0] != 0 || ch.data[1] != 0) return fail(c, PNA_E_INVAL, "bad solid header");
            scur = XSolid(); in_solid = true; scur.order = ents.size(); scur.s0 = schunks.size(); scur.lo = ch.off;
            scur.compression = ch.data[2]; scur.encryption = ch.data[3]; scur.cipher_mode = ch.data[4]; scur.htype = "SHED"; scur.hdr.assign(ch.data, ch.data + ch.len);
        } else if (in_solid) {
            if (is_sdat) { scur.pieces.push_back(XPiece{ch.off + 8, ch.len}); scur.stream_len += ch.len; }
            else if (memcmp(ch.type, "PHSF", 4) == 0) scur.phsf.assign((const char *)ch.data, ch.len);
            else if (memcmp(ch.type, "SEND", 4) == 0) { scur.s1 = schunks.size(); scur.hi = ch.off + 12; solids.push_back(std::move(scur)); in_solid = false; }
            else if (!(ch.type[0] & 0x20)) return fail(c, PNA_E_INVAL, "unknown critical chunk in a solid entry");
        }
        else if (memcmp(ch.type, "FHED", 4) == 0) {
            if (in_entry || ch.len < 6 || ch.data[0] != 0 || ch.data[1] != 0) return fail(c, PNA_E_INVAL, "bad entry header");
            cur = XEntry(); in_entry = true; cur.d0 = dchunks.size(); cur.lo = ch.off;
            cur.kind = ch.data[2]; cur.compression = ch.data[3]; cur.encryption = ch.data[4]; cur.cipher_mode = ch.data[5];
            cur.name.assign((const char *)ch.data + 6, ch.len - 6); cur.hdr.assign(ch.data, ch.data + ch.len);
        } else if (!in_entry) { if (!(ch.type[0] & 0x20)) return fail(c, PNA_E_INVAL, "unknown critical chunk between entries"); }
        else if (is_fdat) { cur.pieces.push_back(XPiece{ch.off + 8, ch.len}); cur.stream_len += ch.len; }
        else if (memcmp(ch.type, "fSIZ", 4) == 0) { if (ch.len > 8) return fail(c, PNA_E_UNSUPPORTED, "entry beyond 2^64 bytes"); cur.has_size = true; cur.raw_size = 0; for (uint32_t i = 0; i < ch.len; i++) cur.raw_size = (cur.raw_size << 8) | ch.data[i]; }
        else if (memcmp(ch.type, "PHSF", 4) == 0) cur.phsf.assign((const char *)ch.data, ch.len);
        else if (memcmp(ch.type, "FEND", 4) == 0) { cur.d1 = dchunks.size(); cur.hi = ch.off + 12; ents.push_back(std::move(cur)); in_entry = false; }
        else if (!(ch.type[0] & 0x20)) return fail(c, PNA_E_INVAL, "unknown critical chunk");      // chunk/types.rs: bit 5 of byte 0 clear = critical
    }
    if (!ended || in_entry || in_solid) return fail(c, PNA_E_INVAL, "archive not terminated by AEND");
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
static int plan_stream(XCall &x, const uint8_t *a, XStream &s, XPlan &P) {
    pna_gpu_ctx *c = x.c;
    s.pk_off = P.pk_total;
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
        if (s.encryption != PNA_ENC_AES) return fail(c, PNA_E_UNSUPPORTED, "only AES entries are decrypted by this driver");
        if (!x.password) return fail(c, PNA_E_INVAL, "encrypted entry and no password");
        if (s.phsf.empty()) return fail(c, PNA_E_INVAL, "`PHSF` chunk not found");
        if (s.cipher_mode == PNA_MODE_CTR || s.cipher_mode == PNA_MODE_CBC) {
            if (s.stream_len < 16) return fail(c, PNA_E_INVAL, "data stream shorter than the IV");
            stream_read(a, s.pieces, 0, 16, s.iv);
            s.pay_len = s.stream_len - 16;
            place(16, s.stream_len, s.pk_off);
            P.enc_list.push_back(&s);
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
                place(at, at + segl - 16, outp);
                outp += segl - 16; at += segl; rest -= segl;
            }
            s.pay_len = outp - s.pk_off;
            P.gcm_list.push_back(&s);
        } else return fail(c, PNA_E_UNSUPPORTED, "unknown cipher mode");
    }
    P.pk_total = (P.pk_total + s.pay_len + 15) & ~(uint64_t)15;
    return PNA_OK;
}
static bool decoded_here(int compression) { return compression == PNA_ALGO_STORE || compression == PNA_ALGO_ZSTD || compression == PNA_ALGO_DEFLATE; }
// the window plan: packed payloads, decoded entries, the gather, the cipher stages' stream lists, the entries without fSIZ
static int plan_window(XCall &x, const uint8_t *a, std::vector<XEntry> &ents, std::vector<XSolid> &solids, XPlan &P) {
    pna_gpu_ctx *c = x.c;
    for (size_t i = 0; i < ents.size(); i++) {
        XEntry &e = ents[i];
        if (!decoded_here(e.compression)) return fail(c, PNA_E_UNSUPPORTED, "compression method not decoded on the device (xz)");
        const int r = plan_stream(x, a, e, P); if (r) return r;
        if (e.compression == PNA_ALGO_STORE) continue;
        // fSIZ is optional (older writers omit it): the payload is then decoded like a solid stream, its size found by the decoder
        if (!e.has_size) { P.nosize_idx.push_back(i); continue; }
        // fSIZ comes from the archive: a size no payload of this length can decode to (deflate tops out at 1032 : 1, zstd at a few
        // thousand : 1 through RLE blocks) is damage, not a reason to ask the device for exabytes
        if (e.raw_size > (1ull << 40) || e.raw_size / 65536 > e.pay_len + 1) return fail(c, PNA_E_INVAL, "fSIZ is out of proportion to the entry's data");
        e.raw_off = P.raw_total; P.raw_total = (P.raw_total + e.raw_size + 15) & ~(uint64_t)15;
        if (P.raw_total > (1ull << 42)) return fail(c, PNA_E_NOMEM, "archive decodes to more than this driver takes in one call");
    }
    for (XSolid &so : solids) {
        if (!decoded_here(so.compression)) return fail(c, PNA_E_UNSUPPORTED, "solid stream: compression method not decoded on the device (xz)");
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
static int upload_window(pna_gpu_ctx *c, const uint8_t *a, size_t archive_len, const std::vector<FrameDesc> &dchunks, const std::vector<FrameDesc> &schunks,
                         const XPlan &P, int slot, uint32_t flag[2], hipStream_t st) {
    int rc = ensure_crc(c); if (rc) return rc;
    if (c->x_arc.ensure(archive_len + 64) || c->x_pk.ensure(P.pk_total + 8192) || c->x_raw[slot].ensure(P.raw_total + 64) || c->x_flag.ensure(64) ||
        c->x_desc.ensure(dchunks.size() * sizeof(FrameDesc) + 16) || c->x_place.ensure(P.places.size() * sizeof(PlaceDescH) + 16)) return fail(c, PNA_E_NOMEM, "extract workspace");
    HIPCHK(c, hipMemcpyAsync(c->x_arc.p, a, archive_len, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(c->x_flag.p, flag0, 8, hipMemcpyHostToDevice, st));
    if (!dchunks.empty()) {
        HIPCHK(c, hipMemcpyAsync(c->x_desc.p, dchunks.data(), dchunks.size() * sizeof(FrameDesc), hipMemcpyHostToDevice, st));
        verify_chunks(c, c->x_desc, dchunks, c->x_arc, "FDAT", st);
    }
    if (!schunks.empty()) {
        if (c->solid_desc.ensure(schunks.size() * sizeof(FrameDesc) + 16)) return fail(c, PNA_E_NOMEM, "extract workspace");
        HIPCHK(c, hipMemcpyAsync(c->solid_desc.p, schunks.data(), schunks.size() * sizeof(FrameDesc), hipMemcpyHostToDevice, st));
        verify_chunks(c, c->solid_desc, schunks, c->x_arc, "SDAT", st);
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
static int decrypt_cbc(pna_gpu_ctx *c, const uint8_t *key, const std::vector<XStream *> &grp, hipStream_t st) {
    int rc = ensure_aes_dec(c); if (rc) return rc;
    constexpr uint64_t CBC_UNIT = 16u << 20;
    std::vector<CipherUnit> units; std::vector<size_t> last_unit(grp.size());
    for (size_t q = 0; q < grp.size(); q++) {
        const XStream &s = *grp[q];
        if (s.pay_len == 0 || (s.pay_len & 15)) return fail(c, PNA_E_INVAL, "CBC: bad length or padding (wrong password or damaged data)");
        for (uint64_t o = 0; o < s.pay_len; o += CBC_UNIT) {
            units.push_back(CipherUnit{s.pk_off + o, 0, (uint32_t)std::min<uint64_t>(CBC_UNIT, s.pay_len - o), (uint32_t)units.size()});
            last_unit[q] = units.size() - 1;
        }
    }
    if (c->ci_units.ensure(units.size() * sizeof(CipherUnit) + 16) || c->ci_ivs.ensure(units.size() * 16 + 16) || c->x_plen.ensure(units.size() * 4 + 16)) return fail(c, PNA_E_NOMEM, "cipher workspace");
    // the units' IVs: the stream's own for its first unit, else the 16 ciphertext bytes in front of the unit (copied on the device BEFORE the
    // kernel overwrites them: the decryption is in place)
    { size_t u = 0;
      for (const XStream *e : grp)
          for (uint64_t o = 0; o < e->pay_len; o += CBC_UNIT, u++) {
              if (o == 0) HIPCHK(c, hipMemcpyAsync((uint8_t *)c->ci_ivs.p + 16 * u, e->iv, 16, hipMemcpyHostToDevice, st));
              else HIPCHK(c, hipMemcpyAsync((uint8_t *)c->ci_ivs.p + 16 * u, (const uint8_t *)c->x_pk.p + e->pk_off + o - 16, 16, hipMemcpyDeviceToDevice, st));
          } }
    AesKey ek, dk; aes256_expand(key, ek); aes256_dec_key(ek, dk);
    std::vector<uint32_t> plen(units.size());
    HIPCHK(c, hipMemcpyAsync(c->ci_units.p, units.data(), units.size() * sizeof(CipherUnit), hipMemcpyHostToDevice, st));
    launch_aes_cbc_dec((const CipherUnit *)c->ci_units.p, (uint32_t)units.size(), (const uint8_t *)c->ci_ivs.p, (const AesDecTabs *)c->aes_dtabs.p,
                       (uint8_t *)c->x_pk.p, dk, (uint32_t *)c->x_plen.p, st);
    rc = read_back(c, plen.data(), c->x_plen.p, units.size() * 4, st); if (rc) return rc;
    for (size_t q = 0; q < grp.size(); q++) {
        const uint32_t pl = plen[last_unit[q]];
        if (pl == 0xFFFFFFFFu) return fail(c, PNA_E_INVAL, "CBC: bad length or padding (wrong password or damaged data)");
        grp[q]->pay_len = (grp[q]->pay_len - 1) / CBC_UNIT * CBC_UNIT + pl;
    }
    return PNA_OK;
}
// CTR and CBC, in place in the packed buffer: streams sharing a PHSF string and a mode share the key, one cipher call per group
static int decrypt_ctr_cbc(XCall &x, const std::vector<XStream *> &enc_list, hipStream_t st) {
    pna_gpu_ctx *c = x.c;
    std::vector<bool> done(enc_list.size(), false);
    for (size_t j = 0; j < enc_list.size(); j++) {
        if (done[j]) continue;
        const XStream &s0 = *enc_list[j];
        const uint8_t *key = nullptr;
        int rc = phsf_key(x, s0.phsf, &key); if (rc) return rc;
        std::vector<XStream *> grp;
        for (size_t k = j; k < enc_list.size(); k++)
            if (!done[k] && enc_list[k]->phsf == s0.phsf && enc_list[k]->cipher_mode == s0.cipher_mode) { done[k] = true; grp.push_back(enc_list[k]); }
        if (s0.cipher_mode == PNA_MODE_CTR) {
            std::vector<uint64_t> off, len; std::vector<uint8_t> ivs;
            for (const XStream *e : grp) { off.push_back(e->pk_off); len.push_back(e->pay_len); ivs.insert(ivs.end(), e->iv, e->iv + 16); }
            pna_gpu_cipher ci{}; ci.encryption = PNA_ENC_AES; ci.cipher_mode = PNA_MODE_CTR; memcpy(ci.key, key, 32); ci.phsf = ""; ci.ivs = ivs.data();
            rc = pna_gpu_cipher_apply_device(c, &ci, 1, off.size(), c->x_pk.p, off.data(), len.data(), st);
        } else rc = decrypt_cbc(c, key, grp, st);
        if (rc) return rc;
    }
    return PNA_OK;
}
// GCM STREAM (decrypt_reader, (_, CipherMode::GCM): lib/src/entry/read.rs:105-140): key confirmation first -- a wrong password is told apart from
// tampering --, then every segment's tag (k_gcm_tag in verify mode), then the CTR keystream with the stream keys
static int decrypt_gcm(XCall &x, const uint8_t *a, const std::vector<XStream *> &gcm_list, uint32_t flag[2], hipStream_t st) {
    pna_gpu_ctx *c = x.c;
    int rc = ensure_aes(c); if (rc) return rc;
    std::vector<GcmEntry> gents; std::vector<uint8_t> tags, giv; std::vector<AesKey> gkeys; std::vector<CipherUnit> units;
    for (const XStream *e : gcm_list) {
        const XStream &s = *e;
        const uint8_t *km = nullptr;
        rc = phsf_key(x, s.phsf, &km); if (rc) return rc;
        GcmMaterial m; stream_read(a, s.pieces, 0, 75, m.header);
        const GcmCallKeys ck = gcm_call_keys(km, s.phsf.data(), s.phsf.size());
        { uint8_t diff = 0; for (int b = 0; b < 32; b++) diff |= (uint8_t)(ck.kc[b] ^ m.header[43 + b]);      // constant time, like the reference's ct_eq
          if (diff) return fail(c, PNA_E_INVAL, "GCM STREAM: key confirmation failed (wrong password)"); }
        gcm_stream_key(km, m.header, s.htype, s.hdr, ck.phsf_hash, m.rk, m.h);
        uint64_t rest = s.stream_len - 75, at = 75, outp = s.pk_off; uint32_t counter = 0;
        while (rest) {
            const uint64_t segl = std::min<uint64_t>(rest, (uint64_t)s.gcm_seg + 16), ctl = segl - 16;
            const bool fin = segl == rest;
            GcmEntry ge{outp, (uint32_t)ctl, 0, {0, 0, 0, 0}, {0, 0, 0, 0}};
            uint8_t iv[16], tag[16];
            gcm_segment(m, counter, fin, ge, iv);
            stream_read(a, s.pieces, at + ctl, 16, tag);             // the stored tag, wherever the chunk boundaries fall
            const uint32_t idx = (uint32_t)gents.size();
            gents.push_back(ge); tags.insert(tags.end(), tag, tag + 16); gkeys.push_back(m.rk);
            giv.insert(giv.end(), iv, iv + 16);
            for (uint64_t o = 0; o < ctl; o += CTR_UNIT) units.push_back(CipherUnit{outp + o, o, (uint32_t)std::min<uint64_t>(CTR_UNIT, ctl - o), idx});
            outp += ctl; at += segl; rest -= segl; counter++;
            if (!fin && segl != (uint64_t)s.gcm_seg + 16) return fail(c, PNA_E_INVAL, "GCM STREAM: short non-final segment");
        }
    }
    if (c->ci_gcm.ensure(gents.size() * sizeof(GcmEntry) + 16) || c->x_tags.ensure(tags.size() + 16) || c->ci_keys.ensure(gkeys.size() * sizeof(AesKey) + 16) ||
        c->ci_ivs.ensure(giv.size() + 16) || c->ci_units.ensure(units.size() * sizeof(CipherUnit) + 16)) return fail(c, PNA_E_NOMEM, "cipher workspace");
    HIPCHK(c, hipMemcpyAsync(c->x_flag.p, flag0, 8, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(c->ci_gcm.p, gents.data(), gents.size() * sizeof(GcmEntry), hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(c->x_tags.p, tags.data(), tags.size(), hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(c->ci_keys.p, gkeys.data(), gkeys.size() * sizeof(AesKey), hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(c->ci_ivs.p, giv.data(), giv.size(), hipMemcpyHostToDevice, st));
    if (!units.empty()) HIPCHK(c, hipMemcpyAsync(c->ci_units.p, units.data(), units.size() * sizeof(CipherUnit), hipMemcpyHostToDevice, st));
    launch_gcm_verify((const GcmEntry *)c->ci_gcm.p, (uint32_t)gents.size(), (const uint8_t *)c->x_pk.p, (const uint8_t *)c->x_tags.p, (uint32_t *)c->x_flag.p, st);
    rc = read_back(c, flag, c->x_flag.p, 8, st); if (rc) return rc;
    if (flag[0]) return fail(c, PNA_E_INVAL, "GCM STREAM: authentication failure (a segment tag does not match)");
    AesKey k0{};
    launch_aes_ctr((const CipherUnit *)c->ci_units.p, (uint32_t)units.size(), (const uint8_t *)c->ci_ivs.p, (const AesTabs *)c->aes_tabs.p, (uint8_t *)c->x_pk.p, k0, (const AesKey *)c->ci_keys.p, st);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(st));
    return PNA_OK;
}
// the entries with fSIZ: one decode call per codec into the raw buffer
static int decode_sized(pna_gpu_ctx *c, const std::vector<XEntry> &ents, int slot, hipStream_t st) {
    for (int algo : {PNA_ALGO_ZSTD, PNA_ALGO_DEFLATE}) {
        std::vector<uint64_t> so, sl, dof, rl;
        for (const XEntry &e : ents) if (e.compression == algo && e.has_size) { so.push_back(e.pk_off); sl.push_back(e.pay_len); dof.push_back(e.raw_off); rl.push_back(e.raw_size); }
        if (so.empty()) continue;
        const int rc = pna_gpu_decompress_batch_device(c, algo, so.size(), c->x_pk.p, so.data(), sl.data(), c->x_raw[slot].p, dof.data(), rl.data(), st);
        if (rc) return rc;
    }
    return PNA_OK;
}
// A stream whose decoded size is recorded nowhere -- an entry without fSIZ, a solid stream -- measured on the device (pna_gpu_open_size_device: the exact
// size, or a proven bound), decoded into c->solid_plain of that size and copied to `out` (a stored one is copied from the packed buffer as it is)
static int decode_open(pna_gpu_ctx *c, const XStream &s, const char *what, std::vector<uint8_t> &out, hipStream_t st) {
    uint64_t got = s.pay_len; const void *d = (const uint8_t *)c->x_pk.p + s.pk_off;
    if (s.compression != PNA_ALGO_STORE) {
        OpenSize m;
        int rc = open_size(c, s.compression, c->x_pk.p, s.pk_off, s.pay_len, &m, st); if (rc) return rc;
        const uint64_t cap = m.size; const int exact = m.exact;
        auto nomem = [&]() {
            char msg[192];
            snprintf(msg, sizeof msg, "%s: the stream decodes to %s%llu bytes, more than the device's free memory takes (with the decoder's workspace)", what,
                     exact ? "" : "at most ", (unsigned long long)cap);
            return fail(c, PNA_E_NOMEM, msg);
        };
        if (c->solid_plain.ensure(cap + 8192)) return nomem();
        rc = s.compression == PNA_ALGO_ZSTD ? zstd_open_decode_planned(c, c->x_pk.p, s.pk_off, s.pay_len, c->solid_plain.p, m, &got, st)
                                            : pna_gpu_inflate_open_device(c, c->x_pk.p, s.pk_off, s.pay_len, c->solid_plain.p, 0, cap, &got, st);
        if (rc == PNA_E_NOMEM) return nomem();
        if (rc) return rc;
        d = c->solid_plain.p;
    }
    out.resize((size_t)got);
    if (got) HIPCHK(c, hipMemcpy(out.data(), d, got, hipMemcpyDeviceToHost));
    return PNA_OK;
}
// A solid entry: its stream decoded, then read_next_normal_entry_from_stream over it (lib/src/entry.rs:401-424): small chunks checked here, the
// inner FDAT CRCs on the device over the decoded stream where it stands
static int walk_solid(pna_gpu_ctx *c, const XSolid &so, std::vector<uint8_t> &plain, std::vector<Inner> &inner, uint32_t flag[2], hipStream_t st) {
    int rc = decode_open(c, so, "solid stream buffer", plain, st); if (rc) return rc;
    std::vector<FrameDesc> ichunks; Inner ic; bool in_i = false;
    for (size_t q = 0; q < plain.size();) {
        PnaChunk ch;
        const int r = next_chunk(plain.data(), plain.size(), q, ch);
        if (r) return fail(c, PNA_E_INVAL, r == CHUNK_SHORT_HEADER ? "solid stream: truncated chunk header" : "solid stream: truncated chunk body");
        const bool fd = memcmp(ch.type, "FDAT", 4) == 0;
        if (fd) { if (ch.len > 0xFFFFFFFBu) return fail(c, PNA_E_INVAL, "data chunk too long"); ichunks.push_back(FrameDesc{ch.off, ch.len, 0, 8, 0}); }
        else if (!chunk_crc_ok(ch)) return fail(c, PNA_E_INVAL, "solid stream: chunk CRC mismatch");
        if (memcmp(ch.type, "FHED", 4) == 0) {
            if (in_i || ch.len < 6 || ch.data[0] != 0 || ch.data[1] != 0) return fail(c, PNA_E_INVAL, "solid stream: bad entry header");
            if (ch.data[3] != PNA_ALGO_STORE || ch.data[4] != PNA_ENC_NONE) return fail(c, PNA_E_UNSUPPORTED, "solid stream: inner entry that is not stored");
            ic = Inner(); in_i = true; ic.kind = ch.data[2]; ic.len = 0; ic.name.assign((const char *)ch.data + 6, ch.len - 6);
        } else if (!in_i) { if (!(ch.type[0] & 0x20)) return fail(c, PNA_E_INVAL, "solid stream: unknown critical chunk"); }
        else if (fd) { ic.pieces.push_back(XPiece{ch.off + 8, ch.len}); ic.len += ch.len; }
        else if (memcmp(ch.type, "FEND", 4) == 0) { inner.push_back(std::move(ic)); in_i = false; }
        else if (memcmp(ch.type, "fSIZ", 4) != 0 && !(ch.type[0] & 0x20)) return fail(c, PNA_E_INVAL, "solid stream: unknown critical chunk");
    }
    if (in_i) return fail(c, PNA_E_INVAL, "solid stream: dangling chunks");
    if (ichunks.empty()) return PNA_OK;
    if (c->solid_desc.ensure(ichunks.size() * sizeof(FrameDesc) + 16)) return fail(c, PNA_E_NOMEM, "extract workspace");
    HIPCHK(c, hipMemcpyAsync(c->x_flag.p, flag0, 8, hipMemcpyHostToDevice, st));
    const bool stored = so.compression == PNA_ALGO_STORE;            // a stored stream is checked where it stands in the packed buffer
    if (stored) for (auto &f : ichunks) f.arc_off += so.pk_off;
    HIPCHK(c, hipMemcpyAsync(c->solid_desc.p, ichunks.data(), ichunks.size() * sizeof(FrameDesc), hipMemcpyHostToDevice, st));
    verify_chunks(c, c->solid_desc, ichunks, stored ? c->x_pk : c->solid_plain, "FDAT", st);
    rc = read_back(c, flag, c->x_flag.p, 8, st); if (rc) return rc;
    if (flag[0]) return fail(c, PNA_E_INVAL, "solid stream: inner FDAT CRC mismatch");
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
static int extract_window(XCall &x, const uint8_t *a, size_t archive_len, std::vector<XEntry> &ents, std::vector<FrameDesc> &dchunks, std::vector<FrameDesc> &schunks,
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
    if (!P.enc_list.empty()) { rc = decrypt_ctr_cbc(x, P.enc_list, st); if (rc) return rc; }
    if (!P.gcm_list.empty()) { rc = decrypt_gcm(x, a, P.gcm_list, flag, st); if (rc) return rc; }
    rc = decode_sized(c, ents, slot, st); if (rc) return rc;
    auto D = std::make_shared<XOut>();
    for (size_t i : P.nosize_idx) {                                   // compatibility path, one decode call per entry
        XEntry &e = ents[i];
        D->nosize_data.emplace_back();
        rc = decode_open(c, e, "entry buffer", D->nosize_data.back(), st); if (rc) return rc;
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

extern "C" int pna_gpu_extract_archive_host(pna_gpu_ctx *c, const void *archive, size_t archive_len, const void *password, size_t password_len,
                                            pna_entry_fn cb, void *user) {
    if (!c || !archive || !cb || (!password && password_len)) return fail(c, PNA_E_INVAL, "null argument");
    const uint8_t *a = (const uint8_t *)archive;
    if (archive_len < 8 + 20 + 12 || memcmp(a, PNA_SIGNATURE, 8) != 0) return fail(c, PNA_E_INVAL, "not a PNA archive");
    std::vector<XEntry> ents; std::vector<FrameDesc> dchunks, schunks; std::vector<XSolid> solids;
    int rc = walk_archive(c, a, archive_len, ents, dchunks, schunks, solids);
    if (rc) return rc;
    // ---- 2. windows: a run of entries whose archive bytes, packed payloads and decoded bytes stay within a few GiB each goes through the
    // device at a time (an archive of any size in host memory against a bounded footprint in HBM); a solid entry is a window of its own
    XCall x{c, password, password_len, cb, user, {}, 0};
    size_t si = 0, w0 = 0;
    const size_t n_all = ents.size();
    const uint64_t WIN = (uint64_t)c->tun.extract_win_mib << 20;  // 1 GiB of archive (and at most 3 GiB decoded) per window by default: small enough to pipeline, large enough for the kernels
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
        std::vector<XEntry> we; std::vector<FrameDesc> wd, ws; std::vector<XSolid> wso;
        uint64_t base, span;
        if (si < solids.size() && solids[si].order <= w0) {
            wso.push_back(std::move(solids[si++])); wso[0].order = 0;
            base = wso[0].lo; span = wso[0].hi - base;
            rebase(wso, schunks, wso[0].s0, wso[0].s1, ws, base);
        } else {
            size_t w1 = w0; uint64_t raw = 0, pk = 0;
            const size_t stop = si < solids.size() ? std::min(n_all, solids[si].order) : n_all;
            while (w1 < stop) {
                const XEntry &e = ents[w1];
                const uint64_t r = e.has_size ? e.raw_size : 0;
                if (w1 > w0 && (e.hi - ents[w0].lo > WIN || raw + r > 3 * WIN || pk + e.stream_len > WIN)) break;
                raw += r; pk += e.stream_len; w1++;
            }
            we.assign(std::make_move_iterator(ents.begin() + w0), std::make_move_iterator(ents.begin() + w1));
            base = we.front().lo; span = we.back().hi - base;
            rebase(we, dchunks, we.front().d0, we.back().d1, wd, base);
            w0 = w1;
        }
        XDeferred cur;
        rc = extract_window(x, a + base, (size_t)span, we, wd, ws, wso, slot, &cur, pending ? &pending : nullptr);
        const int rc2 = finish_pending();
        if (rc == PNA_OK) rc = rc2;
        if (rc != PNA_OK) { (void)hipDeviceSynchronize(); return rc; }
        pending = std::move(cur); slot ^= 1;
    }
    return finish_pending();
}
