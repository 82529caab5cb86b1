"""Argon2 and PBKDF2-SHA256 on the CPU (csrc/kdf_core.h: BLAKE2b and H', the compression G, the reference-index arithmetic, the segment fill, SHA-256,
HMAC and the PBKDF2 chain) -- the code the host functions pna_kdf_argon2 / pna_kdf_pbkdf2_sha256 call and the kernels of k_kdf.hip share.  Built with
g++ alone by tests/kdf_core/Makefile, once as a shared object (tests/kdf_cases.py loads it), once as a stand-alone program under
-fsanitize=address,undefined that derives every case with buffers of exactly the needed sizes (never loaded into this process).  The cases and where
their answers come from: tests/kdf_cases.py.  pna_phsf_parse, the parsing half of the read side's key look-up, is held against the fixtures' PHSF
strings and the forms it refuses."""
import ctypes
import hashlib
import hmac
import os
import subprocess

import pytest

import kdf_cases as K
from conftest import GOLDEN, golden


def test_case_list_holds_what_it_should():
    a, p = K.argon_cases(), K.pbkdf2_cases()
    for kind in (0, 1, 2):
        mine = [c for c in a if c[0] == kind]
        assert {c[2] for c in mine} >= {8, 9, 11, 16, 50, 64, 1024, 4096} and {c[1] for c in mine} == {1, 2, 3} and {c[3] for c in mine} == {1, 2, 4}
        assert {(c[3], c[2]) for c in mine} >= {(2, 16), (2, 17), (4, 32), (4, 33)}
        assert {len(c[4]) for c in mine} == set(K.PW_LENS) and {len(c[5]) for c in mine} == set(K.SALT_LENS)
        assert kind == 0 or any(c[2] == 1024 and c[3] == 1 and c[1] >= 2 for c in mine)      # address blocks inside a segment, with the XOR pass
    assert {c[0] for c in p} == {1, 2, 1000, 4096} and {len(c[1]) for c in p} == {0, 63, 64, 65, 200} and {len(c[2]) for c in p} == {1, 51, 52, 55, 56, 64}
    assert len(p) == 4 * 5 * 6


def test_hash_primitives():
    for n in (0, 1, 55, 56, 63, 64, 65, 111, 112, 127, 128, 129, 255, 256, 257, 1000):
        data = K._bytes(n, n)
        o = ctypes.create_string_buffer(32)
        K.lib().kdf_sha256_c(data, ctypes.c_size_t(n), o)
        assert o.raw == hashlib.sha256(data).digest(), n
        for outlen in (1, 32, 64):
            o = ctypes.create_string_buffer(outlen)
            K.lib().kdf_blake2b_c(data, ctypes.c_size_t(n), o, ctypes.c_size_t(outlen))
            assert o.raw == hashlib.blake2b(data, digest_size=outlen).digest(), (n, outlen)
        for kl in (0, 1, 63, 64, 65, 200):
            key = K._bytes(77 + kl, kl)
            o = ctypes.create_string_buffer(32)
            K.lib().kdf_hmac_sha256_c(key, ctypes.c_size_t(kl), data, ctypes.c_size_t(n), o)
            assert o.raw == hmac.new(key, data, "sha256").digest(), (n, kl)


def test_argon2_against_the_oracle():
    want = K.argon_expected()
    for c, w in zip(K.argon_cases(), want):
        kind, t, m, p, pw, salt = c
        assert K.argon2(kind, pw, salt, t, m, p) == w, c[:4] + (len(pw), len(salt))
    assert len(set(want)) == len(want)


def test_argon2_other_tag_lengths(codec):
    for n in (4, 31, 33, 64, 65, 100):
        assert K.argon2(2, b"password", b"saltsalt", 2, 32, 2, n) == codec.argon2(2, b"password", b"saltsalt", 2, 32, 2, n), n


def test_pbkdf2_against_hashlib():
    for c, w in zip(K.pbkdf2_cases(), K.pbkdf2_expected()):
        r, pw, salt = c
        assert K.pbkdf2(pw, salt, r) == w, (r, len(pw), len(salt))


def test_host_functions_are_callers_of_the_core(pna):
    """pna_kdf_argon2 / pna_kdf_pbkdf2_sha256 (libpna_gpu.so) over the same cases: same answers, other output lengths included"""
    for c, w in zip(K.argon_cases(), K.argon_expected()):
        kind, t, m, p, pw, salt = c
        assert pna.kdf_argon2(kind, pw, salt, t, m, p) == w, c[:4]
    for c, w in zip(K.pbkdf2_cases(), K.pbkdf2_expected()):
        r, pw, salt = c
        assert pna.kdf_pbkdf2_sha256(pw, salt, r)[0] == w, (r, len(pw), len(salt))
    assert pna.kdf_pbkdf2_sha256(b"pw", b"salt", 3, key_len=80)[0] == hashlib.pbkdf2_hmac("sha256", b"pw", b"salt", 3, 80)


def test_sanitizer_program(tmp_path):
    out = K.built()
    cases = tmp_path / "cases.txt"
    cases.write_text(K.case_file_text())
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([os.path.join(out, "kdf_host_san"), str(cases)], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "%d cases, 0 bad" % (len(K.argon_cases()) + len(K.pbkdf2_cases())) in r.stdout


# ---- pna_phsf_parse
def fixture_phsf_strings(pf):
    out = []
    for root, _, files in os.walk(GOLDEN):
        for f in sorted(files):
            if not f.endswith(".pna"):
                continue
            try:
                items = pf.read_archive(open(os.path.join(root, f), "rb").read())[1]
            except Exception:
                continue
            for it in items:
                out += [x.decode() for ty, x in it.chunks if ty == b"PHSF"]
    return out


def test_phsf_parse_fixture_strings(pna, pf, codec):
    strings = fixture_phsf_strings(pf)
    assert len(set(strings)) >= 36                               # 9 distinct strings in each of the four reference archives of earlier releases alone
    for name in ("zstd_aes_ctr.pna", "zstd_aes_cbc.pna", "camellia/zstd_camellia_ctr.pna", "camellia/zstd_camellia_cbc.pna"):
        mine = {x.decode() for it in pf.read_archive(golden(name))[1] for ty, x in it.chunks if ty == b"PHSF"}
        assert len(mine) == 9, name
    for s in sorted(set(strings)):
        f = s.split("$")
        j = pna.phsf_parse(s)
        if f[1].startswith("argon2"):
            prm = dict(kv.split("=") for kv in f[3].split(","))
            assert (j["kind"], j["m_cost_kib"], j["t_cost"], j["lanes"]) == ({"argon2d": 0, "argon2i": 1, "argon2id": 2}[f[1]], int(prm["m"]), int(prm["t"]), int(prm["p"])), s
            assert j["salt"] == codec._b64_nopad(f[4]), s
        else:
            assert f[1] == "pbkdf2-sha256" and j["kind"] == 3 and j["rounds"] == int(dict(kv.split("=") for kv in f[2].split(","))["i"]), s
            assert j["salt"] == codec._b64_nopad(f[3]), s


def test_phsf_parse_grammar_and_caps(pna):
    ok = pna.phsf_parse
    salt = "c2FsdHNhbHQ"                                         # "saltsalt"
    assert ok("$argon2id$v=19$m=64,t=3,p=2$" + salt) == {"kind": 2, "t_cost": 3, "m_cost_kib": 64, "lanes": 2, "rounds": 600000, "salt": b"saltsalt"}
    assert ok("$argon2id$m=64,t=3,p=2$" + salt) == ok("$argon2id$v=19$m=64,t=3,p=2$" + salt)        # the version is optional
    assert ok("$argon2i$v=19$m=8,t=1,p=1$" + salt)["kind"] == 1 and ok("$argon2d$m=8,t=1,p=1$" + salt)["kind"] == 0
    d = ok("$argon2id$v=19$$" + salt)                            # absent parameters: the argon2 crate's defaults
    assert (d["m_cost_kib"], d["t_cost"], d["lanes"]) == (19456, 2, 1)
    assert ok("$argon2id$v=19$t=5$" + salt)["t_cost"] == 5 and ok("$argon2id$v=19$t=5$" + salt)["m_cost_kib"] == 19456
    assert ok("$argon2id$v=19$m=64,t=3,p=2$" + salt + "$aGFzaA")["salt"] == b"saltsalt"      # a hash behind the salt is ignored
    assert ok(b"$argon2id$v=19$m=64,t=3,p=2$" + salt.encode())["salt"] == b"saltsalt"
    p = ok("$pbkdf2-sha256$i=1000,l=32$" + salt)
    assert p["kind"] == 3 and p["rounds"] == 1000 and p["salt"] == b"saltsalt"
    assert ok("$pbkdf2-sha256$l=32$" + salt)["rounds"] == 600000 and ok("$pbkdf2-sha256$i=7$" + salt)["rounds"] == 7
    # each cap's edge
    assert ok("$argon2id$v=19$m=4194304,t=64,p=256$" + salt)["m_cost_kib"] == 4194304
    assert ok("$pbkdf2-sha256$i=10000000,l=32$" + salt)["rounds"] == 10000000
    unsupported = ["$argon2id$v=19$m=4194305,t=1,p=1$" + salt, "$argon2id$v=19$m=64,t=65,p=1$" + salt, "$argon2id$v=19$m=64,t=1,p=257$" + salt,
                   "$argon2id$v=19$m=64,t=1,p=300$" + salt, "$pbkdf2-sha256$i=10000001,l=32$" + salt, "$argon2id$v=16$m=64,t=1,p=1$" + salt,
                   "$argon2id$v=19", "$scrypt$ln=15,r=8,p=1$" + salt, "$pbkdf2-sha512$i=1000$" + salt, "", "argon2id"]
    invalid = ["$argon2x$v=19$m=64,t=1,p=1$" + salt, "$argon2$v=19$m=64,t=1,p=1$" + salt, "$argon2id$v=19$m=64,t=1,p=1", "$argon2id$v=19$m=abc,t=1,p=1$" + salt,
               "$argon2id$v=19$m=64x,t=1,p=1$" + salt, "$argon2id$v=19$m=6 4,t=1,p=1$" + salt,
               "$argon2id$v=19$m=64,t=1,p=1$sa!t", "$pbkdf2-sha256$i=0,l=32$" + salt, "$pbkdf2-sha256$i=abc,l=32$" + salt, "$pbkdf2-sha256$i=5x$" + salt,
               "$pbkdf2-sha256$i=1000,l=32", "$pbkdf2-sha256$i=1000$sa lt"]
    for s, code in [(s, pna.E_UNSUPPORTED) for s in unsupported] + [(s, pna.E_INVAL) for s in invalid]:
        with pytest.raises(pna.PnaGpuError) as e:
            ok(s)
        assert e.value.code == code, s
    # the C entry point: room for the salt, null arguments
    L = pna.load_library()
    j, n, buf = pna.KdfJob(), ctypes.c_size_t(), ctypes.create_string_buffer(8)
    s = ("$argon2id$v=19$m=64,t=3,p=2$" + salt).encode()
    assert L.pna_phsf_parse(s, len(s), ctypes.byref(j), buf, 7, ctypes.byref(n)) == pna.E_DSTSIZE and n.value == 8
    assert L.pna_phsf_parse(s, len(s), ctypes.byref(j), buf, 8, ctypes.byref(n)) == 0 and buf.raw == b"saltsalt" and j.salt_len == 8
    assert L.pna_phsf_parse(s, len(s), None, buf, 8, ctypes.byref(n)) == pna.E_INVAL
