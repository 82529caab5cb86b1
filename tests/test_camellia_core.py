"""Camellia-256 on the CPU (csrc/camellia_core.h: key schedule, decrypt-order schedule, the byte-wise block form of RFC 3713 and the table form the
Camellia kernels of k_cipher.hip run, the CTR / CBC helpers) -- the model tests/test_gpu_camellia.py leans on.  Built with g++ alone by
tests/camellia_core/Makefile, once as a shared object (tests/camellia_cases.py loads it), once as a stand-alone program under
-fsanitize=address,undefined that runs the known answers with buffers of exactly the needed sizes (never loaded into this process).

The known answers, tests/golden/camellia_kat.json, are the `openssl` command-line tool's (3.0.2); the file was written by

    python tests/tools/gen_camellia_kat.py tests/golden/camellia_kat.json

(`openssl enc -camellia-256-{ecb,ctr,cbc} -K <key> [-iv <iv>]`; ECB with -nopad): the RFC 3713 Appendix A vector, 64 random ECB triples, CTR at lengths
0, 1, 15, 16, 17, 31, 33, 4097 under a random IV, one whose last four bytes are ff, and 00..00 ff x 8 (the carry crosses into the high half), CBC at
lengths 0, 1, 15, 16, 17, 47, 48, and the reference's own CBC answer for `PNA test vector!`."""
import os
import random
import shutil
import subprocess

import pytest

import camellia_cases as C
from conftest import golden

KAT = C.kat()
b = bytes.fromhex


def _of(kind):
    return [c for c in KAT if c["kind"] == kind]


def test_kat_file_holds_what_it_should():
    assert len(_of("ecb")) == 65 and len(_of("ctr")) == 24 and len(_of("cbc")) == 8
    rfc = _of("ecb")[0]
    assert rfc["key"] == "0123456789abcdeffedcba987654321000112233445566778899aabbccddeeff" and rfc["out"] == "9acc237dff16d76c20ef7c919e3a7509"
    assert sorted({len(c["in"]) // 2 for c in _of("ctr")}) == [0, 1, 15, 16, 17, 31, 33, 4097]
    assert {c["iv"][-8:] for c in _of("ctr")} >= {"ffffffff"} and any(c["iv"] == "00" * 8 + "ff" * 8 for c in _of("ctr"))
    assert sorted(len(c["in"]) // 2 for c in _of("cbc")) == [0, 1, 15, 16, 16, 17, 47, 48]
    pna = _of("cbc")[-1]
    assert b(pna["in"]) == b"PNA test vector!" and pna["key"] == "11" * 32 and pna["iv"] == "22" * 16
    assert pna["out"] == "47d8900ace4556eff9ff32a5b9605329feabcb5593910cb9acfc2fcb86c8a78b"


@pytest.mark.parametrize("i", range(65))
def test_ecb_known_answers_both_forms_and_back(i):
    c = _of("ecb")[i]
    key, pt, ct = b(c["key"]), b(c["in"]), b(c["out"])
    e = C.schedule(key)
    d = C.dec_schedule(e)
    assert C.block(e, pt) == ct and C.ref_block(key, pt) == ct
    assert C.block(d, ct) == pt and C.ref_block(key, ct, decrypt=True) == pt
    assert list(C.dec_schedule(d)) == list(e)
    assert C.ecb(key, pt) == ct and C.ecb(key, ct, decrypt=True) == pt


def test_ctr_known_answers():
    for c in _of("ctr"):
        key, iv, pt, ct = b(c["key"]), b(c["iv"]), b(c["in"]), b(c["out"])
        assert C.ctr(key, iv, pt) == ct, c["note"]
        assert C.ctr(key, iv, ct) == pt
        for at in (1, 7, 13, 16, 17):                           # a piece of the stream from any byte position
            if at < len(pt):
                assert C.ctr(key, iv, pt[at:], pos=at) == ct[at:], (c["note"], at)


def test_cbc_known_answers():
    for c in _of("cbc"):
        key, iv, pt, ct = b(c["key"]), b(c["iv"]), b(c["in"]), b(c["out"])
        assert C.cbc_encrypt(key, iv, pt) == ct, c["note"]
        assert C.cbc_decrypt(key, iv, ct) == pt
        bad = bytearray(ct); bad[-1] ^= 0x55
        try:
            assert C.cbc_decrypt(key, iv, bytes(bad)) != pt
        except ValueError:
            pass
    with pytest.raises(ValueError):
        C.cbc_decrypt(bytes(32), bytes(16), b"")
    with pytest.raises(ValueError):
        C.cbc_decrypt(bytes(32), bytes(16), bytes(17))


def test_table_form_equals_byte_wise_form():
    """Every byte position of F's input driven through all 256 values: the first round's F sees the plaintext XOR kw1 directly (bytes 0..7), and the
    second round's sees bytes 8..15 XOR kw2 XOR F's output -- so sweeping each of the 16 plaintext bytes sweeps each S-box input of both halves; the
    later rounds see them diffused.  Encrypt and decrypt, three keys."""
    rnd = random.Random(1)
    for key in (bytes(32), bytes(range(32)), bytes(rnd.getrandbits(8) for _ in range(32))):
        e = C.schedule(key)
        d = C.dec_schedule(e)
        base = bytearray(rnd.getrandbits(8) for _ in range(16))
        for pos in range(16):
            for v in range(256):
                blk = bytearray(base); blk[pos] = v
                ct = C.block(e, bytes(blk))
                assert ct == C.ref_block(key, bytes(blk)), (pos, v)
                assert C.block(d, bytes(blk)) == C.ref_block(key, bytes(blk), decrypt=True), (pos, v)
    # ... and the key bytes, through the schedule
    for pos in range(32):
        for v in range(0, 256, 5):
            key = bytearray(range(32)); key[pos] = v
            assert C.block(C.schedule(bytes(key)), bytes(16)) == C.ref_block(bytes(key), bytes(16)), (pos, v)


def test_decrypt_inverts_encrypt():
    rnd = random.Random(2)
    for _ in range(200):
        key, blk = bytes(rnd.getrandbits(8) for _ in range(32)), bytes(rnd.getrandbits(8) for _ in range(16))
        e = C.schedule(key)
        assert C.block(C.dec_schedule(e), C.block(e, blk)) == blk
    for n in (0, 1, 15, 16, 17, 100, 4096):
        key, iv, pt = os.urandom(32), os.urandom(16), os.urandom(n)
        assert C.cbc_decrypt(key, iv, C.cbc_encrypt(key, iv, pt)) == pt
        assert C.ctr(key, iv, C.ctr(key, iv, pt)) == pt


@pytest.mark.skipif(shutil.which("openssl") is None, reason="no openssl command-line tool")
def test_live_against_openssl(tmp_path):
    def ossl(mode, key, data, iv=None):
        a, o = tmp_path / "in", tmp_path / "out"
        a.write_bytes(data)
        cmd = ["openssl", "enc", "-camellia-256-" + mode, "-K", key.hex(), "-in", str(a), "-out", str(o)]
        if iv is not None:
            cmd += ["-iv", iv.hex()]
        if mode == "ecb":
            cmd.append("-nopad")
        r = subprocess.run(cmd, capture_output=True)
        if r.returncode:
            pytest.skip("this openssl has no camellia-256-" + mode)
        return o.read_bytes()
    key, iv = os.urandom(32), os.urandom(12) + b"\xff\xff\xff\xfe"
    data = os.urandom(1000)
    assert C.ecb(key, data[:992]) == ossl("ecb", key, data[:992])
    assert C.ctr(key, iv, data) == ossl("ctr", key, data, iv)
    assert C.cbc_encrypt(key, iv, data) == ossl("cbc", key, data, iv)


def test_sanitizer_program():
    out = C.built()
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([os.path.join(out, "cam_host_san"), os.path.join(C.GOLDEN, "camellia_kat.json")], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "%d cases, 0 bad" % len(KAT) in r.stdout


def _aes_plain(codec, item):
    phsf = [x for ty, x in item.chunks if ty == b"PHSF"][0]
    km = codec.derive_key_from_phsf(phsf.decode(), b"password")
    if item.cipher_mode == 2:
        return codec.decrypt_payload_gcm(km, item.data, item.chunks[0][0], item.chunks[0][1], phsf)
    return codec.decrypt_payload(item.encryption, item.cipher_mode, km, item.data)


@pytest.mark.parametrize("mode", ["ctr", "cbc", "gcm"])
def test_reference_archives(codec, pf, mode):
    """The reference's zstd_camellia_<mode>.pna read with the oracle's container reader, key derivation, stream-key derivation and zstd decoder and this
    core's Camellia: 9 entries, each equal to its namesake of zstd_aes_<mode>.pna; GCM: every segment's tag verifies (camellia_cases.gcm_open raises
    otherwise)."""
    items = pf.read_archive(golden("camellia/zstd_camellia_%s.pna" % mode))[1]
    ref = pf.read_archive(golden("zstd_aes_%s.pna" % mode))[1]
    assert len(items) == 9 and [it.name for it in items] == [it.name for it in ref]
    for it, rt in zip(items, ref):
        assert (it.encryption, it.cipher_mode) == (2, {"cbc": 0, "ctr": 1, "gcm": 2}[mode])
        got = codec.decode_payload(it.compression, C.decrypt_stream(codec, it), 8 << 20)
        assert got == codec.decode_payload(rt.compression, _aes_plain(codec, rt), 8 << 20), it.name
    if mode == "gcm":                                            # a flipped ciphertext bit does not pass
        it = items[0]
        bad = bytearray(it.data); bad[80] ^= 1
        phsf = [x for ty, x in it.chunks if ty == b"PHSF"][0]
        km = codec.derive_key_from_phsf(phsf.decode(), b"password")
        with pytest.raises(ValueError, match="authentication"):
            C.gcm_stream_open(codec, km, bytes(bad), it.chunks[0][0], it.chunks[0][1], phsf)
        with pytest.raises(ValueError, match="key confirmation"):
            C.gcm_stream_open(codec, bytes(32), it.data, it.chunks[0][0], it.chunks[0][1], phsf)


@pytest.mark.parametrize("mode", ["ctr", "cbc", "gcm"])
def test_reference_solid_archives(codec, pf, mode):
    (so,) = pf.read_archive(golden("camellia/solid_zstd_camellia_%s.pna" % mode))[1]
    (ro,) = pf.read_archive(golden("solid_zstd_aes_%s.pna" % mode))[1]
    assert (so.encryption, so.cipher_mode) == (2, {"cbc": 0, "ctr": 1, "gcm": 2}[mode])
    inner = pf.read_solid_inner(codec.decode_payload(so.compression, C.decrypt_stream(codec, so), 16 << 20))
    rinner = pf.read_solid_inner(codec.decode_payload(ro.compression, _aes_plain(codec, ro), 16 << 20))
    # (the two fixtures were written from one directory walk each: the same nine entries, not in the same order)
    assert len(inner) == 9 and sorted((e.name, e.data) for e in inner) == sorted((e.name, e.data) for e in rinner)
