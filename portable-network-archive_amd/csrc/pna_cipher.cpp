// pna_cipher.cpp -- the host side of the cipher stage: the block cipher as a value (BlockKey), the dispatch from an encryption id to the kernels of
// k_cipher.hip (cipher_ctr, cipher_cbc_enc, cipher_cbc_dec -- the only callers of the six launchers), GCM STREAM's per-segment key list and key
// material, IV resolution, and pna_gpu_cipher_apply_device.  The block functions and key schedules themselves are aes_core.h and camellia_core.h.
// Compiled as part of pna_host.cpp, which includes it.
#include "pna_ctx.h"

// ---- the block cipher as a value
void BlockKey::expand(int encryption, const uint8_t key32[32]) {
    enc = encryption;
    if (enc == PNA_ENC_CAMELLIA) cam_expand_host(key32, cam); else aes256_expand(key32, aes);
}
BlockKey BlockKey::dec() const {
    BlockKey d; d.enc = enc;
    if (enc == PNA_ENC_CAMELLIA) cam_dec_key(cam, d.cam); else aes256_dec_key(aes, d.aes);
    return d;
}
void BlockKey::block(const uint8_t in[16], uint8_t out[16]) const {
    if (enc == PNA_ENC_CAMELLIA) cam_block_host(cam, in, out); else aes256_block_host(aes, in, out);
}
bool camellia_on(const pna_gpu_ctx *c) { return c && c->tun.camellia != 0 && launch_cam_ctr && launch_cam_cbc_enc && launch_cam_cbc_dec; }
int check_cipher(pna_gpu_ctx *c, const pna_gpu_cipher *ci) {
    if (ci->encryption == PNA_ENC_CAMELLIA && !camellia_on(c)) return fail(c, PNA_E_UNSUPPORTED, "Camellia is not offered on the device path");
    if (ci->encryption != PNA_ENC_AES && ci->encryption != PNA_ENC_CAMELLIA) return fail(c, PNA_E_INVAL, "unknown encryption");
    if (ci->cipher_mode != PNA_MODE_CTR && ci->cipher_mode != PNA_MODE_CBC && ci->cipher_mode != PNA_MODE_GCM) return fail(c, PNA_E_UNSUPPORTED, "cipher mode not offered on the device path");
    if (ci->cipher_mode == PNA_MODE_GCM && ci->gcm_segment_size > (64u << 20)) return fail(c, PNA_E_INVAL, "GCM segment size beyond 64 MiB");
    return PNA_OK;
}

// ---- the tables on the device, built on the host once per context and on first use
static int ensure_tabs(pna_gpu_ctx *c, bool &ready, DevBuf &buf, const void *tabs, size_t n, const char *what) {
    if (ready) return PNA_OK;
    if (buf.ensure(n)) return fail(c, PNA_E_NOMEM, what);
    HIPCHK(c, hipMemcpy(buf.p, tabs, n, hipMemcpyHostToDevice));
    ready = true;
    return PNA_OK;
}
static int ensure_aes(pna_gpu_ctx *c) { return ensure_tabs(c, c->aes_ready, c->aes_tabs, &aes_host_tabs(), sizeof(AesTabs), "aes tables"); }
static int ensure_aes_dec(pna_gpu_ctx *c) { return ensure_tabs(c, c->aes_dec_ready, c->aes_dtabs, &aes_host_dec_tabs(), sizeof(AesDecTabs), "aes tables"); }
static int ensure_cam(pna_gpu_ctx *c) { return ensure_tabs(c, c->cam_ready, c->cam_tabs, &cam_host_tabs(), sizeof(CamTabs), "camellia tables"); }
int cipher_mark(pna_gpu_ctx *c, int i, hipStream_t st) {
    if (!c->ev_ci[i]) HIPCHK(c, hipEventCreate(&c->ev_ci[i]));
    HIPCHK(c, hipEventRecord(c->ev_ci[i], st));
    return PNA_OK;
}

// ---- GCM STREAM's per-segment keys
void SegKeys::push(uint32_t segment, const BlockKey &k) {
    is_cam.resize(segment + 1, 0); is_cam[segment] = k.enc == PNA_ENC_CAMELLIA;
    if (is_cam[segment]) { cam.resize(segment + 1, CamKey{}); cam[segment] = k.cam; } else { aes.resize(segment + 1, AesKey{}); aes[segment] = k.aes; }
}
void SegKeys::sort_units(std::vector<CipherUnit> &units) {
    aes_units = (size_t)(std::stable_partition(units.begin(), units.end(), [&](const CipherUnit &u) { return !is_cam[u.iv_idx]; }) - units.begin());
}
int SegKeys::upload(pna_gpu_ctx *c, hipStream_t st) const {
    if (c->ci_keys.ensure(aes.size() * sizeof(AesKey) + 16) || c->ci_ckeys.ensure(cam.size() * sizeof(CamKey) + 16)) return fail(c, PNA_E_NOMEM, "cipher workspace");
    if (!aes.empty()) HIPCHK(c, hipMemcpyAsync(c->ci_keys.p, aes.data(), aes.size() * sizeof(AesKey), hipMemcpyHostToDevice, st));
    if (!cam.empty()) HIPCHK(c, hipMemcpyAsync(c->ci_ckeys.p, cam.data(), cam.size() * sizeof(CamKey), hipMemcpyHostToDevice, st));
    return PNA_OK;
}

// ---- the dispatch: the kernel of the key's cipher over device-resident units.  Each readies its tables first (the first call of a context uploads
// them) and then records event 0 of the stage's pair, so ms_cipher never counts that upload; the caller records event 1 behind what it times.
int cipher_ctr(pna_gpu_ctx *c, const CipherUnit *units, uint32_t n, const uint8_t *ivs, uint8_t *buf, const BlockKey &key, const SegKeys *sk, hipStream_t st) {
    // the AES units are [0, na), Camellia's the rest: without stream keys all of them are the key's; with them, the list's (sorted when it holds both)
    const uint32_t na = !sk ? (key.enc == PNA_ENC_CAMELLIA ? 0u : n) : sk->cam.empty() ? n : sk->aes.empty() ? 0u : (uint32_t)sk->aes_units;
    int rc = na ? ensure_aes(c) : PNA_OK; if (rc) return rc;
    rc = n > na ? ensure_cam(c) : PNA_OK; if (rc) return rc;
    rc = cipher_mark(c, 0, st); if (rc) return rc;
    if (na) {
        launch_aes_ctr(units, na, ivs, (const AesTabs *)c->aes_tabs.p, buf, key.enc == PNA_ENC_AES ? key.aes : AesKey{}, sk ? (const AesKey *)c->ci_keys.p : nullptr, st);
    }
    if (n > na) {
        launch_cam_ctr(units + na, n - na, ivs, (const CamTabs *)c->cam_tabs.p, buf, key.enc == PNA_ENC_CAMELLIA ? key.cam : CamKey{}, sk ? (const CamKey *)c->ci_ckeys.p : nullptr, st);
    }
    return PNA_OK;
}
int cipher_cbc_enc(pna_gpu_ctx *c, const CipherUnit *units, uint32_t n, const uint8_t *ivs, uint8_t *buf, const BlockKey &key, hipStream_t st) {
    const bool cam = key.enc == PNA_ENC_CAMELLIA;
    int rc = cam ? ensure_cam(c) : ensure_aes(c); if (rc) return rc;
    rc = cipher_mark(c, 0, st); if (rc) return rc;
    if (cam) launch_cam_cbc_enc(units, n, ivs, (const CamTabs *)c->cam_tabs.p, buf, key.cam, st);
    else launch_aes_cbc_enc(units, n, ivs, (const AesTabs *)c->aes_tabs.p, buf, key.aes, st);
    return PNA_OK;
}
int cipher_cbc_dec(pna_gpu_ctx *c, const CipherUnit *units, uint32_t n, const uint8_t *ivs, uint8_t *buf, const BlockKey &dkey, uint32_t *plain_len, hipStream_t st) {
    const bool cam = dkey.enc == PNA_ENC_CAMELLIA;
    int rc = cam ? ensure_cam(c) : ensure_aes_dec(c); if (rc) return rc;
    rc = cipher_mark(c, 0, st); if (rc) return rc;
    if (cam) launch_cam_cbc_dec(units, n, ivs, (const CamTabs *)c->cam_tabs.p, buf, dkey.cam, plain_len, st);
    else launch_aes_cbc_dec(units, n, ivs, (const AesDecTabs *)c->aes_dtabs.p, buf, dkey.aes, plain_len, st);
    return PNA_OK;
}

// ---- GCM STREAM key material, the head of a solid archive, IVs
// The stream key of a GCM STREAM (derive_stream_key, lib/src/cipher/aead.rs:184-199), bound to the PHSF string and to the header chunk of the entry
// that carries the stream: FHED or SHED (entry_context, aead.rs:167-190).  `header`: salt || nonce prefix || segment size of the stream header.
void gcm_stream_key(const uint8_t master[32], const uint8_t header[43], const char htype[4], const std::vector<uint8_t> &hbody, const uint8_t phsf_hash[32], int encryption, GcmMaterial &m) {
    uint8_t info[88], ks[32];
    memcpy(info, "PNA-STREAM-v1", 13);
    sha256_bytes(htype, 4, hbody.data(), hbody.size(), info + 13);
    memcpy(info + 45, phsf_hash, 32);
    memcpy(info + 77, header + 32, 11);
    hkdf_sha256_32(master, 32, header, 32, info, 88, ks);
    m.key.expand(encryption, ks);
    uint8_t zero[16] = {0}, hb[16];
    m.key.block(zero, hb);
    for (int i = 0; i < 4; i++) m.h[i] = rd_be32(hb + 4 * i);
}
// Segment `counter` of a stream (segment_nonce, lib/src/cipher/gcm.rs): J0 = nonce prefix || counter || final flag || 0 0 0 1.  Gives the tag
// descriptor's H and E(K, J0) and the counter-mode IV of the segment's first data block (counter 2).
void gcm_segment(const GcmMaterial &m, uint32_t counter, bool fin, GcmEntry &ge, uint8_t iv[16]) {
    uint8_t j0[16], eb[16];
    memcpy(j0, m.header + 32, 7); put_be32(j0 + 7, counter); j0[11] = fin ? 1 : 0;
    put_be32(j0 + 12, 1);
    m.key.block(j0, eb);
    memcpy(ge.h, m.h, 16);
    for (int i = 0; i < 4; i++) ge.ej0[i] = rd_be32(eb + 4 * i);
    memcpy(iv, j0, 16); iv[15] = 2;
}
// GCM STREAM material of one entry (lib/src/entry/write.rs:81-107 to_hashed; lib/src/cipher/aead.rs): stream header, round keys and hash subkey of
// the stream key (name == nullptr: the solid entry's SHED)
void gcm_entry_material(const pna_gpu_cipher *ci, const GcmCallKeys &keys, const uint8_t salt_prefix[39], uint32_t seg_size, const char *name, int compression,
                        GcmMaterial &m) {
    memcpy(m.header, salt_prefix, 39);
    put_be32(m.header + 39, seg_size);
    memcpy(m.header + 43, keys.kc, 32);
    const std::vector<uint8_t> fh = name ? frame_fhed_bytes(name, compression, ci->encryption, PNA_MODE_GCM)
                                         : std::vector<uint8_t>{0, 0, (uint8_t)compression, (uint8_t)ci->encryption, (uint8_t)PNA_MODE_GCM};
    gcm_stream_key(ci->key, m.header, name ? "FHED" : "SHED", fh, keys.phsf_hash, ci->encryption, m);
}
// what the GCM STREAMs under one key and PHSF string share: the key confirmation (key_confirmation, aead.rs:161-163) and the hash of the PHSF string
GcmCallKeys gcm_call_keys(const uint8_t key[32], const char *phsf, size_t phsf_len) {
    GcmCallKeys k;
    hkdf_sha256_32(key, 32, nullptr, 0, "PNA-KC-v1", 9, k.kc);
    sha256_bytes(phsf, phsf_len, nullptr, 0, k.phsf_hash);
    return k;
}
// ... the material of a solid archive's one stream (bound to its SHED chunk)
void gcm_solid_material(const pna_gpu_cipher *ci, const uint8_t salt_prefix[39], int compression, GcmMaterial &m) {
    gcm_entry_material(ci, gcm_call_keys(ci->key, ci->phsf, strlen(ci->phsf)), salt_prefix, gcm_seg_size(ci), nullptr, compression, m);
}
// The head of a solid archive: signature + AHED, then SHED; with a cipher PHSF and the stream's first write, a chunk of its own -- the IV (CTR) or
// the stream header (GCM: salt || nonce prefix || segment size || key confirmation, 75 bytes)
void solid_archive_head(std::vector<uint8_t> &head, int compression, const pna_gpu_cipher *ci, const uint8_t *ivs) {
    frame_archive_head(head, 0);
    if (!ci) { frame_solid_head(head, compression); return; }
    if (ci->cipher_mode != PNA_MODE_GCM) { frame_solid_head_enc(head, compression, ci->encryption, ci->cipher_mode, ci->phsf, ivs, 16); return; }
    GcmMaterial gm;
    gcm_solid_material(ci, ivs, compression, gm);
    frame_solid_head_enc(head, compression, ci->encryption, ci->cipher_mode, ci->phsf, gm.header, 75);
}
// the per-entry IVs of a cipher job: the caller's, or random ones (random::random_vec(block_size) per entry, lib/src/entry/write.rs:108-112)
int resolve_ivs(pna_gpu_ctx *c, const pna_gpu_cipher *cipher, size_t n, std::vector<uint8_t> &own, const uint8_t **ivs) {
    int rc = check_cipher(c, cipher); if (rc) return rc;
    if (!cipher->phsf) return fail(c, PNA_E_INVAL, "cipher without a PHSF string");
    *ivs = cipher->ivs;
    if (*ivs) return PNA_OK;
    const size_t per = cipher->cipher_mode == PNA_MODE_GCM ? 39 : 16;  // GCM: salt(32) || nonce_prefix(7) per stream (to_hashed, write.rs:83-86)
    own.resize(n * per + 16);
    for (size_t o = 0; o < n * per;) {
        const ssize_t got = getrandom(own.data() + o, std::min<size_t>(n * per - o, 1u << 20), 0);
        if (got <= 0) return fail(c, PNA_E_INVAL, "getrandom failed");
        o += (size_t)got;
    }
    *ivs = own.data();
    return PNA_OK;
}

// The cipher stage alone over byte ranges of a device buffer (read side: DecryptReader::CtrAes, lib/src/entry/read.rs:83-88).
extern "C" int pna_gpu_cipher_apply_device(pna_gpu_ctx *c, const pna_gpu_cipher *cipher, int decrypt, size_t n, void *d_buf,
                                           const uint64_t *off, const uint64_t *len, void *hip_stream) {
    if (!c || !cipher || (n && (!d_buf || !off || !len || !cipher->ivs))) return fail(c, PNA_E_INVAL, "null argument");
    int rc = check_cipher(c, cipher); if (rc) return rc;
    const bool cbc = cipher->cipher_mode == PNA_MODE_CBC;
    if (cipher->cipher_mode == PNA_MODE_GCM) return fail(c, PNA_E_UNSUPPORTED, "GCM STREAM is offered by the archive entry points only");
    if (cbc && decrypt) return fail(c, PNA_E_UNSUPPORTED, "CBC decryption is not offered on the device path");
    if (n == 0) return PNA_OK;
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : c->stream;
    std::vector<CipherUnit> units;
    for (size_t i = 0; i < n; i++) {
        if (len[i] >= 0xFFFFFFF0ull) return fail(c, PNA_E_INVAL, "cipher range too long");
        if (cbc) units.push_back(CipherUnit{off[i], 0, (uint32_t)len[i], (uint32_t)i});
        else for (uint64_t o = 0; o < len[i]; o += CTR_UNIT) units.push_back(CipherUnit{off[i] + o, o, (uint32_t)std::min<uint64_t>(CTR_UNIT, len[i] - o), (uint32_t)i});
    }
    if (c->ci_units.ensure(units.size() * sizeof(CipherUnit) + 16) || c->ci_ivs.ensure(n * 16)) return fail(c, PNA_E_NOMEM, "cipher workspace");
    BlockKey key; key.expand(cipher->encryption, cipher->key);
    c->timing = pna_gpu_timing{};
    HIPCHK(c, hipMemcpyAsync(c->ci_units.p, units.data(), units.size() * sizeof(CipherUnit), hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(c->ci_ivs.p, cipher->ivs, n * 16, hipMemcpyHostToDevice, st));
    const CipherUnit *d_units = (const CipherUnit *)c->ci_units.p; const uint32_t nu = (uint32_t)units.size();
    rc = cbc ? cipher_cbc_enc(c, d_units, nu, (const uint8_t *)c->ci_ivs.p, (uint8_t *)d_buf, key, st)
             : cipher_ctr(c, d_units, nu, (const uint8_t *)c->ci_ivs.p, (uint8_t *)d_buf, key, nullptr, st);
    if (rc) return rc;
    rc = cipher_mark(c, 1, st); if (rc) return rc;
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(st));
    float mc = 0; (void)hipEventElapsedTime(&mc, c->ev_ci[0], c->ev_ci[1]);
    c->timing.ms_cipher = mc;
    for (size_t i = 0; i < n; i++) c->timing.in_bytes += len[i];
    return PNA_OK;
}
