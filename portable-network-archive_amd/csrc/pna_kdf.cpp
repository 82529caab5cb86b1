// pna_kdf.cpp -- pna_gpu_kdf_batch: a batch of password hashes (one password, n salts and parameter sets) with Argon2's block fill and PBKDF2's chain on
// the device (k_kdf.hip).  What the kernels do not take -- a lane count, a cost, a password or a salt beyond their limits, a job larger than the block
// memory, parameters the algorithm refuses -- goes to pna_kdf_argon2 / pna_kdf_pbkdf2_sha256 in the same call, so a key is the same bytes whatever path
// its job took.
//
// Host work per device job (kdf_core.h): Argon2 -- H0 and the two seed blocks per lane before the fill (2 KiB up per lane), the XOR of the lanes' last
// blocks and H' after it (1 KiB down per lane); PBKDF2 -- the pad states of the password and U_1 (96 bytes up, 32 down).
//
// The memory plan: ONE allocation holds the blocks of the jobs in flight, at most `cap` bytes (option kdf_mem_mib; by default a quarter of the device's
// free memory when the context's first batch arrives, at most 32 GiB) and never more than the batch needs.  The Argon2 jobs, ordered by lane count, passes
// and size so that the two jobs of a wave run the same loops, are cut into ROUNDS that fit; a round is: seeds up, one launch per lane count, last blocks
// down.  The host functions' jobs run on the calling thread while the first round's kernels do.
#include "pna_ctx.h"
#include "kdf_core.h"

namespace pna {
namespace {
constexpr uint32_t KDF_DEV_LANES = 16, KDF_DEV_T = 64, KDF_DEV_M = 1u << 20;      // what k_argon2_fill takes: p, t, m in KiB
constexpr size_t KDF_DEV_PASSWORD = 1024, KDF_DEV_SALT = 64;
bool is_argon(int kind) { return kind == PNA_KDF_ARGON2D || kind == PNA_KDF_ARGON2I || kind == PNA_KDF_ARGON2ID_JOB; }
int host_job(const void *password, size_t password_len, const pna_kdf_job &j, uint8_t *key) {
    if (is_argon(j.kind)) return pna_kdf_argon2(j.kind, password, password_len, j.salt, j.salt_len, j.t_cost, j.m_cost_kib, j.lanes, key, 32);
    if (j.kind == PNA_KDF_PBKDF2_SHA256_JOB) return pna_kdf_pbkdf2_sha256(password, password_len, j.salt, j.salt_len, j.rounds, key, 32, nullptr, 0);
    return PNA_E_INVAL;
}
}

int kdf_batch(pna_gpu_ctx *c, const void *password, size_t password_len, size_t n, const pna_kdf_job *jobs, uint8_t *keys, int *status, hipStream_t st, bool add) {
    if (!add) { c->kdf_dev_jobs = c->kdf_host_jobs = c->kdf_rounds = 0; c->kdf_ms = 0; }      // (add: a driver's further batch, counted on top)
    if (!launch_argon2_fill || !launch_pbkdf2_sha256) return fail(c, PNA_E_UNSUPPORTED, "this build has no key derivation kernels");
    // the block memory's cap
    if (!c->tun.kdf_mem_mib && !c->kdf_cap) {
        size_t fr = 0, tot = 0;
        HIPCHK(c, hipMemGetInfo(&fr, &tot));
        c->kdf_cap = std::min<size_t>(fr / 4, (size_t)32 << 30);
    }
    const size_t cap = c->tun.kdf_mem_mib ? (size_t)c->tun.kdf_mem_mib << 20 : c->kdf_cap;
    // who derives what
    const bool small = password_len <= KDF_DEV_PASSWORD;
    std::vector<size_t> argon, pbk, host;
    for (size_t i = 0; i < n; i++) {
        const pna_kdf_job &j = jobs[i];
        const bool ok = small && j.salt_len <= KDF_DEV_SALT && (j.salt || !j.salt_len);
        if (ok && is_argon(j.kind) && j.lanes >= 1 && j.lanes <= KDF_DEV_LANES && j.t_cost >= 1 && j.t_cost <= KDF_DEV_T &&
            j.m_cost_kib >= 8 * j.lanes && j.m_cost_kib <= KDF_DEV_M && (size_t)kdf_argon_geom(j.kind, j.t_cost, j.m_cost_kib, j.lanes).blocks * 1024 <= cap) argon.push_back(i);
        else if (ok && j.kind == PNA_KDF_PBKDF2_SHA256_JOB && j.rounds >= 1) pbk.push_back(i);
        else host.push_back(i);
    }
    if (!c->kdf_ev[0]) for (auto &e : c->kdf_ev) HIPCHK(c, hipEventCreate(&e));
    auto timed = [&](float &acc) -> int { float ms = 0; HIPCHK(c, hipEventElapsedTime(&ms, c->kdf_ev[0], c->kdf_ev[1])); acc += ms; return PNA_OK; };
    float ms_all = 0;
    // PBKDF2: one launch
    std::vector<uint32_t> pbk_out(pbk.size() * 8);
    if (!pbk.empty()) {
        std::vector<KdfPbkdf2Job> pj(pbk.size());
        for (size_t k = 0; k < pbk.size(); k++) { const pna_kdf_job &j = jobs[pbk[k]]; kdf_pbkdf2_start(password, password_len, j.salt, j.salt_len, 1, pj[k].s); pj[k].rounds = j.rounds; }
        if (c->kdf_jobs.ensure(pj.size() * sizeof(KdfPbkdf2Job)) || c->kdf_fin.ensure(pbk_out.size() * 4)) return fail(c, PNA_E_NOMEM, "key derivation workspace");
        HIPCHK(c, hipMemcpyAsync(c->kdf_jobs.p, pj.data(), pj.size() * sizeof(KdfPbkdf2Job), hipMemcpyHostToDevice, st));
        HIPCHK(c, hipEventRecord(c->kdf_ev[0], st));
        launch_pbkdf2_sha256((const KdfPbkdf2Job *)c->kdf_jobs.p, (uint32_t)pj.size(), (uint32_t *)c->kdf_fin.p, st);
        HIPCHK(c, hipEventRecord(c->kdf_ev[1], st));
        HIPCHK(c, hipMemcpyAsync(pbk_out.data(), c->kdf_fin.p, pbk_out.size() * 4, hipMemcpyDeviceToHost, st));
        if (!argon.empty()) {                                     // (the workspace is the Argon2 rounds' next: drained here; otherwise after the host's jobs)
            HIPCHK(c, hipStreamSynchronize(st)); HIPCHK(c, hipGetLastError());
            const int rc = timed(ms_all); if (rc) return rc;
        }
    }
    // the host's jobs: after the first device work is in flight
    bool host_done = false; int first_bad = PNA_OK;
    auto run_host = [&]() {
        if (host_done) return;
        host_done = true;
        for (size_t i : host) {
            const int rc = host_job(password, password_len, jobs[i], keys + 32 * i);
            c->kdf_host_jobs++;
            if (status) status[i] = rc; else if (rc && !first_bad) first_bad = rc;
            if (first_bad) return;
        }
    };
    // Argon2: rounds of jobs whose blocks fit
    std::stable_sort(argon.begin(), argon.end(), [&](size_t a, size_t b) {
        const pna_kdf_job &x = jobs[a], &y = jobs[b];
        if (x.lanes != y.lanes) return x.lanes < y.lanes;
        if (x.t_cost != y.t_cost) return x.t_cost < y.t_cost;
        return x.m_cost_kib < y.m_cost_kib;
    });
    for (size_t r0 = 0; r0 < argon.size();) {
        size_t r1 = r0; uint64_t blocks = 0; uint32_t nlanes = 0;
        std::vector<KdfArgonJob> aj;
        while (r1 < argon.size()) {
            const pna_kdf_job &j = jobs[argon[r1]];
            const KdfArgonGeom g = kdf_argon_geom(j.kind, j.t_cost, j.m_cost_kib, j.lanes);
            if ((blocks + g.blocks) * 1024 > cap) break;          // (a job alone fits: the routing above)
            aj.push_back(KdfArgonJob{g, nlanes, 0, blocks});
            blocks += g.blocks; nlanes += g.lanes; r1++;
        }
        if ((size_t)blocks * 1024 > c->kdf_mem.cap) {             // exactly what the largest round so far needs: never beyond the cap
            c->kdf_mem.release();
            if (hipMalloc(&c->kdf_mem.p, (size_t)blocks * 1024) != hipSuccess) { c->kdf_mem.p = nullptr; (void)hipGetLastError(); return fail(c, PNA_E_NOMEM, "Argon2 block memory"); }
            c->kdf_mem.cap = (size_t)blocks * 1024;
        }
        std::vector<uint64_t> seeds((size_t)nlanes * 256), fin((size_t)nlanes * 128);
        for (size_t k = r0; k < r1; k++) {
            const pna_kdf_job &j = jobs[argon[k]]; const KdfArgonJob &a = aj[k - r0];
            uint8_t h0[72];
            kdf_argon_h0(a.g, j.m_cost_kib, 32, password, password_len, j.salt, j.salt_len, h0);
            for (uint32_t l = 0; l < a.g.lanes; l++) for (uint32_t b = 0; b < 2; b++) kdf_argon_seed(h0, l, b, seeds.data() + ((size_t)(a.lane0 + l) * 2 + b) * 128);
        }
        if (c->kdf_jobs.ensure(aj.size() * sizeof(KdfArgonJob)) || c->kdf_seeds.ensure(seeds.size() * 8) || c->kdf_fin.ensure(fin.size() * 8)) return fail(c, PNA_E_NOMEM, "key derivation workspace");
        HIPCHK(c, hipMemcpyAsync(c->kdf_jobs.p, aj.data(), aj.size() * sizeof(KdfArgonJob), hipMemcpyHostToDevice, st));
        HIPCHK(c, hipMemcpyAsync(c->kdf_seeds.p, seeds.data(), seeds.size() * 8, hipMemcpyHostToDevice, st));
        HIPCHK(c, hipEventRecord(c->kdf_ev[0], st));
        for (size_t k = 0; k < aj.size();) {                      // one launch per lane count
            size_t e = k; while (e < aj.size() && aj[e].g.lanes == aj[k].g.lanes) e++;
            launch_argon2_fill((const KdfArgonJob *)c->kdf_jobs.p + k, (uint32_t)(e - k), aj[k].g.lanes, (uint64_t *)c->kdf_mem.p, (const uint64_t *)c->kdf_seeds.p, (uint64_t *)c->kdf_fin.p, st);
            k = e;
        }
        HIPCHK(c, hipEventRecord(c->kdf_ev[1], st));
        HIPCHK(c, hipMemcpyAsync(fin.data(), c->kdf_fin.p, fin.size() * 8, hipMemcpyDeviceToHost, st));
        run_host();
        HIPCHK(c, hipStreamSynchronize(st)); HIPCHK(c, hipGetLastError());
        { const int rc = timed(ms_all); if (rc) return rc; }
        for (size_t k = r0; k < r1; k++) {
            const KdfArgonJob &a = aj[k - r0];
            uint64_t *f = fin.data() + (size_t)a.lane0 * 128;
            for (uint32_t l = 1; l < a.g.lanes; l++) for (int i = 0; i < 128; i++) f[i] ^= f[(size_t)l * 128 + i];
            kdf_argon_tag(f, keys + 32 * argon[k], 32);
            if (status) status[argon[k]] = PNA_OK;
            c->kdf_dev_jobs++;
        }
        c->kdf_rounds++;
        r0 = r1;
    }
    run_host();
    if (!pbk.empty()) {
        if (argon.empty()) { HIPCHK(c, hipStreamSynchronize(st)); HIPCHK(c, hipGetLastError()); const int rc = timed(ms_all); if (rc) return rc; }
        for (size_t k = 0; k < pbk.size(); k++) { kdf_words_be(pbk_out.data() + 8 * k, keys + 32 * pbk[k]); if (status) status[pbk[k]] = PNA_OK; c->kdf_dev_jobs++; }
    }
    c->kdf_ms += ms_all;
    if (first_bad) return fail(c, first_bad, "key derivation: a job's parameters are refused");
    return PNA_OK;
}
}

extern "C" int pna_gpu_kdf_batch(pna_gpu_ctx *c, const void *password, size_t password_len, size_t n, const pna_kdf_job *jobs, uint8_t *keys, int *status, void *hip_stream) {
    if (!c) return PNA_E_NODEVICE;
    if ((!password && password_len) || (n && (!jobs || !keys))) return fail(c, PNA_E_INVAL, "null argument");
    HIPCHK(c, hipSetDevice(c->device));
    return kdf_batch(c, password, password_len, n, jobs, keys, status, hip_stream ? (hipStream_t)hip_stream : c->stream, false);
}

extern "C" int pna_gpu_debug_kdf_stats(pna_gpu_ctx *c, uint64_t *device_jobs, uint64_t *host_jobs, uint64_t *rounds, double *ms_kernels) {
    if (!c) return PNA_E_INVAL;
    if (device_jobs) *device_jobs = c->kdf_dev_jobs;
    if (host_jobs) *host_jobs = c->kdf_host_jobs;
    if (rounds) *rounds = c->kdf_rounds;
    if (ms_kernels) *ms_kernels = c->kdf_ms;
    return PNA_OK;
}
