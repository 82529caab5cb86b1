"""`pna create --solid --aes ctr|gcm` from host memory (pna_gpu_create_solid_archive_enc_host): the serialised inner entries stream through windows of
solid_win_mib MiB and the cipher runs window by window -- CTR with the keystream continued at the window's stream offset, GCM STREAM with segments cut
from the whole compressed stream (GcmEncryptWriter, lib/src/cipher/gcm.rs:45-90) and the tail that is not yet a segment carried on the device.  Every
archive must equal the one-shot device archive (pna_gpu_create_solid_archive_enc_device) with the same IV / salt, and read back with the oracle."""
import os

import pytest

pytestmark = pytest.mark.gpu

MODES = ("ctr", "gcm")
GCM_SEGS = (4096, 333333, 1 << 20, 64 << 20)        # segment edges at many places inside windows, on them, and one segment longer than an archive


def _key(pna):
    return pna.kdf_pbkdf2_sha256(b"password", bytes(range(16)), 1000)


def _cipher(pna, mode, seg=0, ivs=None):
    key, phsf = _key(pna)
    if mode == "ctr":
        return pna.Cipher(key, phsf, pna.MODE_CTR, ivs=ivs if ivs is not None else os.urandom(16))
    return pna.Cipher(key, phsf, pna.MODE_GCM, ivs=ivs if ivs is not None else os.urandom(39), gcm_segment_size=seg)


def _device_one_shot(ctx, pna, names, ents, algo, cipher):
    import torch
    offs, pos = [], 0
    for e in ents:
        offs.append(pos); pos = (pos + len(e) + 15) & ~15
    src = torch.zeros(pos + 8192, dtype=torch.uint8, device="cuda")
    for o, e in zip(offs, ents):
        if e:
            src[o:o + len(e)] = torch.frombuffer(bytearray(e), dtype=torch.uint8).cuda()
    lens = [len(e) for e in ents]
    cap = pna.solid_archive_enc_bound(algo, names, lens, cipher)
    dst = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    total = ctx.create_solid_archive_device(names, src.data_ptr(), offs, lens, dst.data_ptr(), cap, algo=algo, cipher=cipher)
    return dst[:total].cpu().numpy().tobytes()


def _plain(pf, names, ents):
    """the serialised inner stream, from the oracle's writer (STORE records, lib/src/entry.rs:888-913)"""
    return b"".join(pf.write_normal_entry(pf.file_entry_header(0, pf.sanitize_name(nm)), [e] if e else [], len(e)) for nm, e in zip(names, ents))


def _oracle_reads(pna, pf, codec, arc, algo, mode, want_plain):
    """the reference's read path with the oracle: decrypt the SDAT bodies (CTR: IV first; GCM: stream header, every tag and the final flag), decode"""
    key, phsf = _key(pna)
    (so,) = pf.read_archive(arc)[1]
    assert so.encryption == 1 and so.cipher_mode == (1 if mode == "ctr" else 2)
    if mode == "ctr":
        comp = codec.decrypt_payload(1, 1, key, so.data)
    else:
        comp = codec.decrypt_payload_gcm(key, so.data, b"SHED", pf.solid_header_bytes(algo, 1, 2), phsf.encode())
    assert codec.decode_payload(algo, comp, len(want_plain) + 4096) == want_plain


def _sized_last(pf, names, ents, target):
    """the last entry's length that makes the serialised stream exactly `target` bytes long"""
    head = len(_plain(pf, names[:-1], ents[:-1]))
    ln = target - head - 100
    for _ in range(8):
        rec = len(pf.write_normal_entry(pf.file_entry_header(0, pf.sanitize_name(names[-1])), [b"x"], ln)) - 1 + ln
        if head + rec == target:
            return ln
        ln += target - head - rec
    raise AssertionError("no length fits")


def _cases(pf, codec, win):
    """(names, entries) of the test streams for a window of `win` MiB"""
    out = []
    big = codec.corpus_file(0, 9001, 2600000)
    for delta in (0, 7, 13):
        # the first record ends around the 1 MiB edge: its CRC field, FEND and the next FHED straddle the edge in turn
        first = codec.corpus_file(1, 9100 + delta, (1 << 20) - 70 - delta)
        ents = [first, b"", big, b"", codec.corpus_file(2, 9002, 300000), codec.corpus_file(1, 9003, (1 << 20) + 5)]
        out.append(([f"d/{i}.bin" for i in range(len(ents))], ents))
    W = win << 20
    for target in (3 * W, 3 * W + 1, 700000):                  # the stream ends on a window edge, one byte past one; a one-window stream
        ents = [codec.corpus_file(0, 9200, 300000), b"", codec.corpus_file(1, 9201, 1 << 16)]
        names = [f"e/{i}" for i in range(len(ents))] + ["e/last"]
        ents.append(codec.corpus_file(0, 9202 + target % 7, _sized_last(pf, names, ents + [b""], target)))
        assert len(_plain(pf, names, ents)) == target
        out.append((names, ents))
    return out


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("algo_name", ["zstd", "deflate"])
def test_encrypted_solid_stream_equals_device_archive(gpu_ctx, pna, pf, codec, algo_name, mode):
    algo = pna.ALGO_ZSTD if algo_name == "zstd" else pna.ALGO_DEFLATE
    segs = GCM_SEGS if mode == "gcm" else (0,)
    read = 0
    try:
        for win in (1, 2):
            gpu_ctx.set_option("solid_win_mib", win)
            for ci, (names, ents) in enumerate(_cases(pf, codec, win)):
                for seg in segs:
                    cipher = _cipher(pna, mode, seg)
                    got = gpu_ctx.create_solid_archive_enc_host(names, ents, algo=algo, cipher=cipher)
                    assert got == _device_one_shot(gpu_ctx, pna, names, ents, algo, cipher), (win, ci, seg)
                    if (ci + segs.index(seg)) % 3 == 0:
                        _oracle_reads(pna, pf, codec, got, algo, mode, _plain(pf, names, ents))
                        read += 1
                    if ci == 1 and seg in (0, 333333):
                        assert [(n, d) for n, _, d in pna.extract_archive(gpu_ctx, got, b"password")] == list(zip(names, ents))
        gpu_ctx.set_option("solid_win_mib", 1)
        many = [codec.corpus_file(1, 9300 + i, 3000 + 37 * (i % 50)) for i in range(900)]       # many small inner entries
        nm = [f"m/{i}" for i in range(len(many))]
        for seg in segs[:2]:
            cipher = _cipher(pna, mode, seg)
            got = gpu_ctx.create_solid_archive_enc_host(nm, many, algo=algo, cipher=cipher)
            assert got == _device_one_shot(gpu_ctx, pna, nm, many, algo, cipher), seg
            _oracle_reads(pna, pf, codec, got, algo, mode, _plain(pf, nm, many))
        assert [(n, d) for n, _, d in pna.extract_archive(gpu_ctx, got, b"password")] == list(zip(nm, many))
        for seg in segs:                                                               # the empty archive (the one-shot form)
            cipher = _cipher(pna, mode, seg)
            got = gpu_ctx.create_solid_archive_enc_host([], [], algo=algo, cipher=cipher)
            assert got == _device_one_shot(gpu_ctx, pna, [], [], algo, cipher)
            _oracle_reads(pna, pf, codec, got, algo, mode, b"")
    finally:
        gpu_ctx.set_option("solid_win_mib", 256)
    assert read >= 4


def test_encrypted_solid_stream_in_latency_mode(pna, codec):
    """The library's defaults (latency mode: small streams take small blocks and LZ units): the windowed GCM / CTR archives equal the one-shot ones"""
    import torch  # noqa: F401  (shares its HIP runtime with the extension)
    ctx = pna.Context(0)
    try:
        ents = [codec.corpus_file(i % 3, 9400 + i, (1 << 20) - 1000 * i) for i in range(5)] + [codec.corpus_file(0, 9499, 50000)]
        names = [f"l/{i}" for i in range(len(ents))]
        for mode, seg in (("ctr", 0), ("gcm", 65536)):
            cipher = _cipher(pna, mode, seg)
            want = _device_one_shot(ctx, pna, names, ents, pna.ALGO_ZSTD, cipher)
            ctx.set_option("solid_win_mib", 1)
            assert ctx.create_solid_archive_enc_host(names, ents, cipher=cipher) == want, mode
            ctx.set_option("solid_win_mib", 256)
    finally:
        ctx.close()


def test_encrypted_solid_top_level_and_refusals(gpu_ctx, pna, pf, codec):
    ents = [codec.corpus_file(0, 9500, 400000), b"", codec.corpus_file(1, 9501, 1 << 20), b"tail"]
    names = [f"t/{i}" for i in range(len(ents))]
    try:
        gpu_ctx.set_option("solid_win_mib", 1)
        # Argon2id by default in the reference: the PHSF in the argon2 crate's PHC form, and the archive opens with the password
        for mode in (pna.MODE_CTR, pna.MODE_GCM):
            arc = pna.create_archive_encrypted(gpu_ctx, names, ents, b"secret", mode=mode, solid=True, kdf="argon2id")
            (so,) = pf.read_archive(arc)[1]
            phsf = dict(so.chunks)[b"PHSF"].decode()
            assert phsf.startswith("$argon2id$v=19$m=19456,t=2,p=1$") and len(phsf.rsplit("$", 1)[1]) == 22, phsf
            assert (so.encryption, so.cipher_mode) == (1, mode)
            assert [(n, d) for n, _, d in pna.extract_archive(gpu_ctx, arc, b"secret")] == list(zip(names, ents))
            with pytest.raises(pna.PnaGpuError):
                pna.extract_archive(gpu_ctx, arc, b"wrong")
            key = codec.derive_key_from_phsf(phsf, b"secret")
            comp = codec.decrypt_payload(1, 1, key, so.data) if mode == pna.MODE_CTR else \
                codec.decrypt_payload_gcm(key, so.data, b"SHED", pf.solid_header_bytes(pna.ALGO_ZSTD, 1, 2), phsf.encode())
            assert codec.decode_payload(pna.ALGO_ZSTD, comp, 1 << 22) == _plain(pf, names, ents)
        # PBKDF2 with a round count, solid, deflate
        arc = pna.create_archive_encrypted(gpu_ctx, names, ents, b"secret", algo=pna.ALGO_DEFLATE, mode=pna.MODE_GCM, rounds=1000, solid=True)
        (so,) = pf.read_archive(arc)[1]
        assert dict(so.chunks)[b"PHSF"].startswith(b"$pbkdf2-sha256$i=1000,l=32$")
        assert [(n, d) for n, _, d in pna.extract_archive(gpu_ctx, arc, b"secret")] == list(zip(names, ents))
        # non-solid with Argon2id: pna_gpu_create_archive_enc_host under the new entry point
        arc = pna.create_archive_encrypted(gpu_ctx, names, ents, b"secret", mode=pna.MODE_GCM, kdf="argon2id")
        assert all(it.encryption == 1 for it in pf.read_archive(arc)[1])
        assert [(n, d) for n, _, d in pna.extract_archive(gpu_ctx, arc, b"secret")] == list(zip(names, ents))
        # refusals: CBC over a solid stream, Camellia
        for kw in (dict(mode=pna.MODE_CBC, solid=True), dict(mode=pna.MODE_CBC, solid=True, kdf="argon2id")):
            with pytest.raises(pna.PnaGpuError) as ei:
                pna.create_archive_encrypted(gpu_ctx, names, ents, b"secret", rounds=1000, **kw)
            assert ei.value.code == pna.E_UNSUPPORTED
        key, phsf = _key(pna)
        for ci in (pna.Cipher(key, phsf, pna.MODE_CBC, ivs=bytes(16)), pna.Cipher(key, phsf, pna.MODE_CTR, encryption=pna.ENC_CAMELLIA, ivs=bytes(16))):
            with pytest.raises(pna.PnaGpuError) as ei:
                gpu_ctx.create_solid_archive_enc_host(names, ents, cipher=ci)
            assert ei.value.code == pna.E_UNSUPPORTED
        with pytest.raises(ValueError):
            pna.create_archive_encrypted(gpu_ctx, names, ents, b"secret", kdf="scrypt")
        # no cipher: the plain windowed archive
        for algo in (pna.ALGO_ZSTD, pna.ALGO_DEFLATE):
            assert gpu_ctx.create_solid_archive_enc_host(names, ents, algo=algo, cipher=None) == pna.create_archive(gpu_ctx, names, ents, algo=algo, solid=True)
            assert gpu_ctx.create_solid_archive_enc_host(names, ents, algo=algo, cipher=pna.Cipher(key, phsf, encryption=pna.ENC_NONE)) == \
                pna.create_archive(gpu_ctx, names, ents, algo=algo, solid=True)
    finally:
        gpu_ctx.set_option("solid_win_mib", 256)
