"""Camellia-256 on the device (k_cipher.hip's k_cam_* kernels; option "camellia" = 1): CTR, CBC and GCM STREAM on the write and the read side, against the CPU core
(csrc/camellia_core.h through tests/camellia_cases.py, which tests/test_camellia_core.py pins to openssl's answers and the reference's archives) and
against the reference's six Camellia fixtures.  Integer work: bit-exact.  A context of its own with the option set, closed afterwards; the session's
default context shows that nothing changes without the option."""
import os
import zlib

import pytest

import camellia_cases as C
from conftest import golden, GOLDEN

pytestmark = pytest.mark.gpu

PW = b"password"
SIZES = [1 << 20, 70000, 0, 3, (1 << 20) + 17, 65536, 15, 16, 17]
MODES = {"cbc": 0, "ctr": 1, "gcm": 2}
KEY = bytes(range(7, 39))
PHSF = "$pbkdf2-sha256$i=1000,l=32$c2FsdHNhbHRzYWx0"


@pytest.fixture(scope="module")
def ctx(pna):
    import torch  # noqa: F401  (shares its HIP runtime with the extension)
    c = pna.Context(0)
    c.set_option("camellia", 1)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ents(codec):
    return [codec.corpus_file(0, 1200 + i, n) if n else b"" for i, n in enumerate(SIZES)]


@pytest.fixture(scope="module")
def keyed(pna):
    return pna.kdf_pbkdf2_sha256(PW, bytes(range(16)), 1000)           # (key, phsf) that the read side derives again from the password


NAMES = ["c/%d.txt" % i for i in range(len(SIZES))]


def iv_kinds():
    return [os.urandom(16), os.urandom(12) + b"\xff" * 4, b"\x00" * 8 + b"\xff" * 8]


def cam(pna, key, phsf, mode, **kw):
    return pna.Cipher(key, phsf, mode, encryption=pna.ENC_CAMELLIA, **kw)


def fix_crc(buf, ty, at, n):
    buf[at + n:at + n + 4] = (zlib.crc32(bytes(buf[at:at + n]), zlib.crc32(ty)) & 0xFFFFFFFF).to_bytes(4, "big")


# ---- the option gate
def test_refused_without_the_option(pna, gpu_ctx):
    import torch
    buf = torch.zeros(64, dtype=torch.uint8, device="cuda")
    with pytest.raises(pna.PnaGpuError) as ei:
        gpu_ctx.cipher_apply_device(cam(pna, KEY, PHSF, pna.MODE_CTR, ivs=bytes(16)), buf.data_ptr(), [0], [16])
    assert ei.value.code == -7 and "Camellia is not offered" in str(ei.value)
    with pytest.raises(pna.PnaGpuError) as ei:
        pna.create_archive_encrypted(gpu_ctx, ["a"], [b"abc"], PW, rounds=1000, encryption=pna.ENC_CAMELLIA)
    assert ei.value.code == -7
    with pytest.raises(pna.PnaGpuError) as ei:
        pna.extract_archive(gpu_ctx, golden("camellia/zstd_camellia_ctr.pna"), PW)
    assert ei.value.code == -7 and "only AES entries" in str(ei.value)
    recs, s = pna.verify_archive(gpu_ctx, golden("camellia/zstd_camellia_gcm.pna"), PW)
    assert len(recs) == 9 and all(r[2] == pna.VERIFY_UNSUPPORTED for r in recs) and s["unsupported"] == 9


def test_option_values(pna, ctx):
    with pytest.raises(pna.PnaGpuError) as ei:
        ctx.set_option("camellia", 2)
    assert ei.value.code == pna.E_INVAL
    with pytest.raises(pna.PnaGpuError) as ei:
        ctx.set_option("camellia", -1)
    assert ei.value.code == pna.E_INVAL
    ctx.set_option("camellia", 0)
    import torch
    buf = torch.zeros(64, dtype=torch.uint8, device="cuda")
    with pytest.raises(pna.PnaGpuError) as ei:
        ctx.cipher_apply_device(cam(pna, KEY, PHSF, pna.MODE_CTR, ivs=bytes(16)), buf.data_ptr(), [0], [16])
    assert ei.value.code == -7
    ctx.set_option("camellia", 1)


# ---- pna_gpu_cipher_apply_device
def test_rfc3713_block_on_device(pna, ctx):
    """CTR over 16 zero bytes with IV = the RFC 3713 Appendix A plaintext yields Camellia-256(key, IV): the appendix ciphertext"""
    import torch
    buf = torch.zeros(64, dtype=torch.uint8, device="cuda")
    key = bytes.fromhex("0123456789abcdeffedcba987654321000112233445566778899aabbccddeeff")
    ctx.cipher_apply_device(cam(pna, key, PHSF, pna.MODE_CTR, ivs=bytes.fromhex("0123456789abcdeffedcba9876543210")), buf.data_ptr(), [0], [16])
    out = bytes(buf.cpu().numpy())
    assert out[:16].hex() == "9acc237dff16d76c20ef7c919e3a7509" and out[16:] == bytes(48)


def test_ctr_known_answers_on_device(pna, ctx):
    """openssl's CTR answers (tests/golden/camellia_kat.json), one call per key"""
    import torch
    by_key = {}
    for c in C.kat():
        if c["kind"] == "ctr":
            by_key.setdefault(c["key"], []).append(c)
    assert len(by_key) == 3
    for key, cases in by_key.items():
        flat, offs = bytearray(), []
        for c in cases:
            flat += b"\xA5" * 5; offs.append(len(flat)); flat += bytes.fromhex(c["in"])
        flat += b"\xA5" * 32
        lens = [len(c["in"]) // 2 for c in cases]
        buf = torch.frombuffer(bytearray(flat), dtype=torch.uint8).cuda()
        ctx.cipher_apply_device(cam(pna, bytes.fromhex(key), PHSF, pna.MODE_CTR, ivs=b"".join(bytes.fromhex(c["iv"]) for c in cases)), buf.data_ptr(), offs, lens)
        got = bytes(buf.cpu().numpy())
        for c, o, n in zip(cases, offs, lens):
            assert got[o:o + n].hex() == c["out"], c["note"]
            assert got[o - 5:o] == b"\xA5" * 5


@pytest.mark.parametrize("align", [0, 1, 7, 13])
def test_ctr_ranges_equal_cpu_core(pna, ctx, align):
    """Ranges that start at byte offset `align` mod 16, lengths around the block and 256 KiB + 1 (two units, the seam inside a keystream block), the
    three kinds of IV; guard bytes between and around the ranges stay untouched; applying it twice restores the input."""
    import torch
    lens = [0, 1, 15, 16, 17, 255, (256 << 10) + 1]
    flat, offs, ivs, want_lens = bytearray(os.urandom(16 + align)), [], [], []
    for iv in iv_kinds():
        for n in lens:
            offs.append(len(flat)); ivs.append(iv); want_lens.append(n)
            flat += os.urandom(n)
            flat += os.urandom(16 + (-n) % 16)                        # guard; the next range starts at `align` mod 16 again
    assert all(o % 16 == align for o in offs)
    buf = torch.frombuffer(bytearray(flat), dtype=torch.uint8).cuda()
    ci = cam(pna, KEY, PHSF, pna.MODE_CTR, ivs=b"".join(ivs))
    ctx.cipher_apply_device(ci, buf.data_ptr(), offs, want_lens)
    got = bytes(buf.cpu().numpy())
    want = bytearray(flat)
    for o, n, iv in zip(offs, want_lens, ivs):
        want[o:o + n] = C.ctr(KEY, iv, bytes(flat[o:o + n]))
    assert got == bytes(want)
    assert ctx.timing().ms_cipher > 0
    ctx.cipher_apply_device(ci, buf.data_ptr(), offs, want_lens, decrypt=True)
    assert bytes(buf.cpu().numpy()) == bytes(flat)


def test_cbc_encrypt_equals_cpu_core(pna, ctx):
    import torch
    lens = [0, 1, 15, 16, 17, 4095, 4096]
    blobs = [os.urandom(n) for n in lens]
    flat, offs = bytearray(), []
    for i, b in enumerate(blobs):
        flat += os.urandom(1 + i % 5); offs.append(len(flat)); flat += b + bytes(16 - len(b) % 16)     # room for the padding block
    flat += os.urandom(64)
    ivs = os.urandom(16 * len(lens))
    buf = torch.frombuffer(bytearray(flat), dtype=torch.uint8).cuda()
    ctx.cipher_apply_device(cam(pna, KEY, PHSF, pna.MODE_CBC, ivs=ivs), buf.data_ptr(), offs, lens)
    got = bytes(buf.cpu().numpy())
    want = bytearray(flat)
    for i, (o, b) in enumerate(zip(offs, blobs)):
        c = C.cbc_encrypt(KEY, ivs[16 * i:16 * i + 16], b)
        want[o:o + len(c)] = c
    assert got == bytes(want)
    # openssl's CBC answers as well
    for c in (c for c in C.kat() if c["kind"] == "cbc"):
        pt = bytes.fromhex(c["in"])
        b2 = torch.frombuffer(bytearray(pt + bytes(16 - len(pt) % 16) + b"\xA5" * 16), dtype=torch.uint8).cuda()
        ctx.cipher_apply_device(cam(pna, bytes.fromhex(c["key"]), PHSF, pna.MODE_CBC, ivs=bytes.fromhex(c["iv"])), b2.data_ptr(), [0], [len(pt)])
        assert bytes(b2.cpu().numpy()).hex() == c["out"] + "a5" * 16, c["note"]
    with pytest.raises(pna.PnaGpuError) as ei:
        ctx.cipher_apply_device(cam(pna, KEY, PHSF, pna.MODE_CBC, ivs=ivs), buf.data_ptr(), offs, lens, decrypt=True)
    assert ei.value.code == -7
    with pytest.raises(pna.PnaGpuError) as ei:
        ctx.cipher_apply_device(cam(pna, KEY, PHSF, pna.MODE_GCM, ivs=bytes(39)), buf.data_ptr(), [0], [16])
    assert ei.value.code == -7


# ---- archives
def _to_device(ents):
    import torch
    offs, pos = [], 0
    for e in ents:
        offs.append(pos); pos = (pos + len(e) + 15) & ~15
    src = torch.zeros(pos + 8192, dtype=torch.uint8, device="cuda")
    for o, e in zip(offs, ents):
        if e:
            src[o:o + len(e)] = torch.frombuffer(bytearray(e), dtype=torch.uint8).cuda()
    return src, offs


def _create(pna, ctx, form, names, ents, ci, algo):
    if form == "host":
        return pna.create_archive_encrypted(ctx, names, ents, b"", algo=algo, cipher=ci)
    import torch
    src, offs = _to_device(ents)
    lens = [len(e) for e in ents]
    cap = pna.archive_enc_bound(algo, names, lens, ci)
    dst = torch.full((cap,), 0xA5, dtype=torch.uint8, device="cuda")
    total, _ = ctx.create_archive_device(names, src.data_ptr(), offs, lens, dst.data_ptr(), cap, algo=algo, cipher=ci)
    assert bytes(dst[total:total + 16].cpu().numpy()) == b"\xA5" * 16
    return dst[:total].cpu().numpy().tobytes()


@pytest.mark.parametrize("form", ["device", "host"])
@pytest.mark.parametrize("algo_name", ["zstd", "deflate"])
@pytest.mark.parametrize("mode_name", ["ctr", "cbc", "gcm"])
def test_archives(pna, ctx, pf, codec, ents, keyed, mode_name, algo_name, form):
    """create with Camellia on the device -> the oracle's container reader (every chunk CRC) -> the CPU core decrypts, the oracle decodes: the input;
    the FHED encryption byte is 2; the extract driver gives the entries back; a wrong password is -2 (GCM: the key confirmation says so); GCM
    ciphertext altered with its chunk CRC repaired is -2 with "authentication"."""
    key, phsf = keyed
    algo = pna.ALGO_ZSTD if algo_name == "zstd" else pna.ALGO_DEFLATE
    mode = MODES[mode_name]
    arc = _create(pna, ctx, form, NAMES, ents, cam(pna, key, phsf, mode), algo)
    items = pf.read_archive(arc)[1]
    assert [it.name for it in items] == NAMES
    for it, e in zip(items, ents):
        assert (it.encryption, it.cipher_mode, it.compression, it.raw_file_size) == (2, mode, algo, len(e)) and it.chunks[0][1][4] == 2
        assert codec.decode_payload(algo, C.decrypt_stream(codec, it, PW), len(e) + 64) == e
    assert len({it.data[:16] for it in items}) == len(items)          # a fresh IV / salt per entry
    assert pna.extract_archive(ctx, arc, PW) == [(n, 0, e) for n, e in zip(NAMES, ents)]
    with pytest.raises(pna.PnaGpuError) as ei:
        pna.extract_archive(ctx, arc, b"passw0rd")
    assert ei.value.code == -2
    if mode_name == "gcm":
        assert "key confirmation" in str(ei.value)
        body = items[0].chunks[4][1]                                  # FDAT(ciphertext || tag) of the first entry
        at = arc.index(body[:64])
        bad = bytearray(arc); bad[at + 100] ^= 1
        fix_crc(bad, b"FDAT", at, len(body))
        with pytest.raises(pna.PnaGpuError) as ei:
            pna.extract_archive(ctx, bytes(bad), PW)
        assert ei.value.code == -2 and "authentication" in str(ei.value)


@pytest.mark.parametrize("form", ["device", "host"])
def test_gcm_small_segments(pna, ctx, pf, codec, keyed, form):
    """gcm_segment_size 4096: payloads of 70 000 bytes (many segments, a partial last one) and a payload of exactly 8 192 compressed bytes (a full final
    segment) -- a deflate level-0 entry, whose stored stream is its bytes plus a fixed frame"""
    key, phsf = keyed
    noise = [codec.corpus_file(2, 77 + i, 70000) for i in range(3)]   # incompressible: ~70 000 bytes of payload each
    over = len(ctx.compress_batch([noise[0][:8000]], algo=pna.ALGO_DEFLATE, level=0)[0]) - 8000
    exact = noise[1][:8192 - over]
    assert len(ctx.compress_batch([exact], algo=pna.ALGO_DEFLATE, level=0)[0]) == 8192
    ci = cam(pna, key, phsf, pna.MODE_GCM, gcm_segment_size=4096)
    for algo, level, group in ((pna.ALGO_ZSTD, pna.LEVEL_DEFAULT, noise), (pna.ALGO_DEFLATE, 0, [exact])):
        names = ["g/%d" % i for i in range(len(group))]
        if form == "host":
            arc = pna.create_archive_encrypted(ctx, names, group, b"", algo=algo, level=level, cipher=ci)
        else:
            import torch
            src, offs = _to_device(group)
            lens = [len(e) for e in group]
            cap = pna.archive_enc_bound(algo, names, lens, ci)
            dst = torch.full((cap,), 0xA5, dtype=torch.uint8, device="cuda")
            total, _ = ctx.create_archive_device(names, src.data_ptr(), offs, lens, dst.data_ptr(), cap, algo=algo, level=level, cipher=ci)
            arc = dst[:total].cpu().numpy().tobytes()
        items = pf.read_archive(arc)[1]
        for it, e in zip(items, group):
            assert int.from_bytes(it.data[39:43], "big") == 4096
            comp = C.decrypt_stream(codec, it, PW)
            nseg = max(1, -(-len(comp) // 4096))
            assert len(it.data) == 75 + len(comp) + 16 * nseg
            if algo == pna.ALGO_DEFLATE:
                assert len(comp) == 8192 and nseg == 2
            else:
                assert nseg >= 17 and len(comp) % 4096
            assert codec.decode_payload(algo, comp, len(e) + 64) == e
        assert pna.extract_archive(ctx, arc, PW) == [(n, 0, e) for n, e in zip(names, group)]


# ---- solid
@pytest.mark.parametrize("mode_name", ["ctr", "gcm"])
def test_solid_round_trips(pna, ctx, pf, codec, ents, keyed, mode_name):
    import torch
    key, phsf = keyed
    mode = MODES[mode_name]
    ci = cam(pna, key, phsf, mode)
    lens = [len(e) for e in ents]
    src, offs = _to_device(ents)
    cap = pna.solid_archive_enc_bound(pna.ALGO_ZSTD, NAMES, lens, ci)
    dst = torch.full((cap,), 0xA5, dtype=torch.uint8, device="cuda")
    total = ctx.create_solid_archive_device(NAMES, src.data_ptr(), offs, lens, dst.data_ptr(), cap, cipher=ci)
    dev = dst[:total].cpu().numpy().tobytes()
    assert bytes(dst[total:total + 16].cpu().numpy()) == b"\xA5" * 16
    host = ctx.create_solid_archive_enc_host(NAMES, ents, cipher=ci)
    big = ents + [codec.corpus_file(2, 5, (3 << 20) + 5)]             # incompressible: the stream spans several windows of 1 MiB
    bnames = NAMES + ["c/noise.bin"]
    ctx.set_option("solid_win_mib", 1)
    try:
        windows = ctx.create_solid_archive_enc_host(bnames, big, cipher=ci)
    finally:
        ctx.set_option("solid_win_mib", 256)
    for arc, nm, en in ((dev, NAMES, ents), (host, NAMES, ents), (windows, bnames, big)):
        (so,) = pf.read_archive(arc)[1]
        assert (so.encryption, so.cipher_mode) == (2, mode) and so.chunks[0][1][3] == 2
        inner = pf.read_solid_inner(codec.decode_payload(so.compression, C.decrypt_stream(codec, so, PW), sum(len(e) for e in en) + 65536))
        assert [(e.name, e.data) for e in inner] == list(zip(nm, en))
        assert [(n, d) for n, _, d in pna.extract_archive(ctx, arc, PW)] == list(zip(nm, en))
    with pytest.raises(pna.PnaGpuError) as ei:
        pna.extract_archive(ctx, dev, b"passw0rd")
    assert ei.value.code == -2
    arc = pna.create_archive_encrypted(ctx, NAMES, ents, PW, mode=mode, rounds=1000, solid=True, encryption=pna.ENC_CAMELLIA)
    assert [(n, d) for n, _, d in pna.extract_archive(ctx, arc, PW)] == list(zip(NAMES, ents))


def test_solid_cbc_is_still_refused(pna, ctx, ents, keyed):
    key, phsf = keyed
    with pytest.raises(pna.PnaGpuError) as ei:
        ctx.create_solid_archive_enc_host(NAMES, ents, cipher=cam(pna, key, phsf, pna.MODE_CBC, ivs=bytes(16)))
    assert ei.value.code == -7
    with pytest.raises(pna.PnaGpuError) as ei:
        pna.create_archive_encrypted(ctx, NAMES, ents, PW, mode=pna.MODE_CBC, rounds=1000, solid=True, encryption=pna.ENC_CAMELLIA)
    assert ei.value.code == -7


def test_password_entry_point(pna, ctx, pf, codec, ents):
    """pna_create_archive_encrypted_with: the password hash on the host (Argon2id, PBKDF2), Camellia on the device"""
    for mode, kdf in ((pna.MODE_CTR, "pbkdf2"), (pna.MODE_GCM, "argon2id")):
        arc = pna.create_archive_encrypted(ctx, NAMES[:4], ents[:4], b"secret", mode=mode, rounds=1000, kdf=kdf, encryption=pna.ENC_CAMELLIA)
        items = pf.read_archive(arc)[1]
        assert all((it.encryption, it.cipher_mode) == (2, mode) for it in items)
        for it, e in zip(items, ents):
            assert codec.decode_payload(it.compression, C.decrypt_stream(codec, it, b"secret"), len(e) + 64) == e
        assert pna.extract_archive(ctx, arc, b"secret") == [(n, 0, e) for n, e in zip(NAMES[:4], ents[:4])]


# ---- the reference's archives
def golden_files():
    out = {}
    for d, _, fs in os.walk(os.path.join(GOLDEN, "raw")):
        for f in fs:
            p = os.path.join(d, f)
            out[os.path.relpath(p, GOLDEN).replace(os.sep, "/")] = open(p, "rb").read()
    return out


FIXTURES = [s + "zstd_camellia_" + m + ".pna" for s in ("", "solid_") for m in ("ctr", "cbc", "gcm")]


@pytest.mark.parametrize("fname", FIXTURES)
def test_reference_archives(pna, ctx, gpu_ctx, fname):
    """extract: the 9 entries of the AES fixture of the same mode (read by the same driver); verify: all OK; under a wrong password BAD_AUTH on GCM and UNAUTHENTICATED failures on CTR / CBC only; SKIPPED
    without a password, UNSUPPORTED without the option; diff against tests/golden/raw: SAME; extract-select: one entry to device memory, one to host"""
    import torch
    arc, aes = golden("camellia/" + fname), golden(fname.replace("camellia", "aes"))
    got = pna.extract_archive(ctx, arc, PW)
    want = pna.extract_archive(ctx, aes, PW)
    assert len(got) == 9 and sorted(got) == sorted(want)
    files = golden_files()
    assert sum(1 for n, _, d in got if files.get(n) == d) >= 5
    with pytest.raises(pna.PnaGpuError) as ei:
        pna.extract_archive(ctx, arc, b"passw0rd")
    assert ei.value.code == -2
    gcm = fname.endswith("gcm.pna")
    recs, s = pna.verify_archive(ctx, arc, PW)
    assert s["rc"] == 0 and s["failed"] == 0 and s["unsupported"] == 0 and s["skipped"] == 0 and s["ok"] == s["total"] == len(recs)
    assert all(r[2] == pna.VERIFY_OK for r in recs)
    assert not any(r[3] & pna.VERIFY_UNAUTHENTICATED for r in recs)   # (the flag qualifies a failure)
    arecs, _ = pna.verify_archive(ctx, aes, PW)
    assert sorted((r[0] or "", r[1], r[2], r[3]) for r in recs) == sorted((r[0] or "", r[1], r[2], r[3]) for r in arecs)     # the AES fixture's verdicts
    # a wrong password: GCM's key confirmation tells it apart (BAD_AUTH); on CTR / CBC it cannot be told from damage -- UNAUTHENTICATED on what fails
    recs, s = pna.verify_archive(ctx, arc, b"passw0rd")
    failed = [r for r in recs if r[2] != pna.VERIFY_OK]
    assert s["failed"] == len(failed) >= 1 and s["unauthenticated_failure"] == (0 if gcm else 1)
    for r in failed:
        if gcm:
            assert r[2] == pna.VERIFY_BAD_AUTH and not (r[3] & pna.VERIFY_UNAUTHENTICATED), r
        else:
            assert r[2] in (pna.VERIFY_BAD_DECRYPT, pna.VERIFY_BAD_STREAM) and r[3] & pna.VERIFY_UNAUTHENTICATED, r
    arecs, _ = pna.verify_archive(ctx, aes, b"passw0rd")
    assert sorted((r[0] or "", r[1], r[3]) for r in recs) == sorted((r[0] or "", r[1], r[3]) for r in arecs)
    recs, s = pna.verify_archive(ctx, arc)
    assert s["skipped"] >= 1 and s["failed"] == 0 and all(r[2] == pna.VERIFY_SKIPPED for r in recs if r[1] == pna.VERIFY_KIND_SOLID or not fname.startswith("solid_"))
    recs, s = pna.verify_archive(gpu_ctx, arc, PW)
    assert s["unsupported"] >= 1 and s["ok"] == 0 and all(r[2] == pna.VERIFY_UNSUPPORTED for r in recs if r[1] == pna.VERIFY_KIND_SOLID or not fname.startswith("solid_"))
    recs, s = pna.diff_archive(ctx, arc, files, PW)
    assert s["rc"] == 0 and s["damaged"] == 0 and s["skipped"] == 0 and len(recs) == 9
    assert all(r.status == pna.DIFF_SAME and r.first_diff is None and r.size == len(files[r.name]) for r in recs if r.name in files)
    assert all(r.status == pna.DIFF_MISSING for r in recs if r.name not in files) and s["same"] >= 5
    dev_name, host_name = "raw/images/icon.png", "raw/text.txt"
    t = torch.full((len(files[dev_name]) + 32,), 0xA5, dtype=torch.uint8, device="cuda")
    recs, s = pna.extract_select(ctx, arc, lambda i, nm, k, st: t[16:16 + len(files[dev_name])] if nm == dev_name else ("host" if nm == host_name else None), PW)
    assert s["selected"] == 2 and s["to_host"] == 1 and s["to_device"] == 1
    by = {r[1]: r for r in recs}
    assert by[host_name][3] == pna.EXTRACT_OK and by[host_name][4] == files[host_name]
    assert by[dev_name][3] == pna.EXTRACT_OK and by[dev_name][5] == len(files[dev_name])
    back = bytes(t.cpu().numpy())
    assert back[16:-16] == files[dev_name] and back[:16] == b"\xA5" * 16 and back[-16:] == b"\xA5" * 16


# ---- AES and Camellia streams in one window
@pytest.mark.parametrize("mode_name", ["ctr", "gcm", "cbc"])
def test_mixed_archive(pna, ctx, pf, ents, keyed, mode_name):
    """HEAD part with AES entries + TAIL part with Camellia entries, concatenated: one archive, extracted in one window; verify and diff read it too"""
    key, phsf = keyed
    mode = MODES[mode_name]
    head = pna.create_archive_chunked(ctx, ["a/%d" % i for i in range(len(ents))], ents, 0, cipher=pna.Cipher(key, phsf, mode), part=pna.PART_HEAD)
    tail = pna.create_archive_chunked(ctx, ["k/%d" % i for i in range(len(ents))], ents, 0, cipher=cam(pna, key, phsf, mode), part=pna.PART_TAIL)
    arc = head + tail
    items = pf.read_archive(arc)[1]
    assert [it.encryption for it in items] == [1] * len(ents) + [2] * len(ents)
    got = pna.extract_archive(ctx, arc, PW)
    assert got == [("a/%d" % i, 0, e) for i, e in enumerate(ents)] + [("k/%d" % i, 0, e) for i, e in enumerate(ents)]
    recs, s = pna.verify_archive(ctx, arc, PW)
    assert s["ok"] == s["total"] == 2 * len(ents) and s["failed"] == 0
    # interleaved as well: every other entry of each family
    def entries(buf):
        out, cur, pos = [], None, 0
        for ty, d, end in pf.read_chunks(buf, 0):
            if ty == b"FHED":
                cur = pos
            if ty == b"FEND":
                out.append(buf[cur:end])
            pos = end
        return out
    ea, ek = entries(head[8 + 20:]), entries(tail[:-12])
    assert len(ea) == len(ek) == len(ents)
    woven = head[:28] + b"".join(a + k for a, k in zip(ea, ek)) + tail[-12:]
    got = pna.extract_archive(ctx, woven, PW)
    assert [d for _, _, d in got] == [e for e in ents for _ in (0, 1)]
