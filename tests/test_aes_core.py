"""AES-256 on the CPU (csrc/aes_core.h: the S-box and table builders, aes256_expand, aes256_dec_key, and the block function the kernels of k_cipher.hip
run -- aes_block and aes_block_inv over a table accessor).  Built with g++ alone by tests/aes_core/Makefile, once as a shared object that this module
loads, once as a stand-alone program under -fsanitize=address,undefined that runs the known answers and seeded round trips with buffers of exactly the
needed sizes (never loaded into this process).

Known answers: FIPS-197 Appendix C.3 (AES-256 block) and NIST SP 800-38A F.2.5 / F.2.6 (CBC-AES256) and F.5.5 / F.5.6 (CTR-AES256); the independent
model is oracle/cipher_model.c (byte-wise FIPS-197, no tables shared with the library)."""
import ctypes
import functools
import os
import random
import subprocess
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(tempfile.gettempdir(), "pna_aes_core_%d" % os.getuid())
b = bytes.fromhex

C3_KEY, C3_PT, C3_CT = b("000102030405060708090a0b0c0d0e0f101112131415161718191a1b1c1d1e1f"), b("00112233445566778899aabbccddeeff"), b("8ea2b7ca516745bfeafc49904b496089")
SP_KEY = b("603deb1015ca71be2b73aef0857d77811f352c073b6108d72d9810a30914dff4")
SP_PT = b("6bc1bee22e409f96e93d7e117393172aae2d8a571e03ac9c9eb76fac45af8e5130c81c46a35ce411e5fbc1191a0a52eff69f2445df4f9b17ad2b417be66c3710")
CBC_IV, CBC_CT = b("000102030405060708090a0b0c0d0e0f"), b(
    "f58c4c04d6e5f1ba779eabfb5f7bfbd69cfc4e967edb808d679f777bc6702c7d39f23369a9d9bacfa530e26304231461b2eb05e2c39be9fcda6c19078c6a9d1b")
CTR_IV, CTR_CT = b("f0f1f2f3f4f5f6f7f8f9fafbfcfdfeff"), b(
    "601ec313775789a5b7a7f504bbf3d228f443e3ca4d62b59aca84e990cacaf5c52b0930daa23de94ce87017ba2d84988ddfc9c58db67aada613c2dd08457941a6")


@functools.lru_cache(maxsize=None)
def built() -> str:
    subprocess.run(["make", "-s", "-C", os.path.join(HERE, "aes_core"), "OUT=" + OUT, "lib", "san"], check=True)
    return OUT


@functools.lru_cache(maxsize=None)
def lib():
    return ctypes.CDLL(os.path.join(built(), "libaes_host.so"))


def schedule(key: bytes):
    out = (ctypes.c_uint32 * 60)()
    lib().aes_expand_c(bytes(key), out)
    return out


def dec_schedule(sched):
    out = (ctypes.c_uint32 * 60)()
    lib().aes_dec_key_c(sched, out)
    return out


def block(sched, data: bytes, inv: bool = False) -> bytes:
    out = ctypes.create_string_buffer(16)
    lib().aes_block_c(sched, int(inv), bytes(data), out)
    return out.raw


def ctr(key: bytes, iv: bytes, data: bytes, pos: int = 0) -> bytes:
    buf = ctypes.create_string_buffer(bytes(data), max(len(data), 1))
    lib().aes_ctr_c(bytes(key), bytes(iv), ctypes.c_uint64(pos), buf, ctypes.c_size_t(len(data)))
    return buf.raw[:len(data)]


def cbc(key: bytes, iv: bytes, data: bytes, decrypt: bool = False) -> bytes:
    out = ctypes.create_string_buffer(max(len(data), 1))
    lib().aes_cbc_c(bytes(key), bytes(iv), int(decrypt), bytes(data), ctypes.c_size_t(len(data) // 16), out)
    return out.raw[:len(data)]


def test_fips197_c3_both_directions():
    e = schedule(C3_KEY)
    assert block(e, C3_PT) == C3_CT
    assert block(dec_schedule(e), C3_CT, inv=True) == C3_PT
    # the schedule's ends for the key of FIPS-197 A.3: w0 = the key's first word, w59 = 706c631e -- words little-endian here
    a3 = schedule(SP_KEY)
    assert a3[0] == int.from_bytes(SP_KEY[:4], "little") and a3[59] == int.from_bytes(b("706c631e"), "little")


def test_sp800_38a_cbc_aes256():
    assert cbc(SP_KEY, CBC_IV, SP_PT) == CBC_CT
    assert cbc(SP_KEY, CBC_IV, CBC_CT, decrypt=True) == SP_PT


def test_sp800_38a_ctr_aes256():
    assert ctr(SP_KEY, CTR_IV, SP_PT) == CTR_CT
    assert ctr(SP_KEY, CTR_IV, CTR_CT) == SP_PT
    for at in (1, 7, 15, 16, 17, 33, 63):                       # a piece of the stream from any byte position
        assert ctr(SP_KEY, CTR_IV, SP_PT[at:], pos=at) == CTR_CT[at:], at


def test_inverse_cipher_inverts_the_forward_one():
    rnd = random.Random(11)
    for _ in range(300):
        key, blk = bytes(rnd.getrandbits(8) for _ in range(32)), bytes(rnd.getrandbits(8) for _ in range(16))
        e = schedule(key)
        d = dec_schedule(e)
        ct = block(e, blk)
        assert ct != blk and block(d, ct, inv=True) == blk
        assert block(e, block(d, blk, inv=True)) == blk


def test_agrees_with_the_oracle(codec):
    rnd = random.Random(12)
    for _ in range(200):
        key, blk = bytes(rnd.getrandbits(8) for _ in range(32)), bytes(rnd.getrandbits(8) for _ in range(16))
        e = schedule(key)
        assert block(e, blk) == codec.aes_block(key, blk)
        assert block(dec_schedule(e), blk, inv=True) == codec.aes_block(key, blk, decrypt=True)
    # every byte position of the state through all 256 values: every table entry of both directions is read
    key, base = bytes(range(32)), bytes(rnd.getrandbits(8) for _ in range(16))
    e = schedule(key)
    d = dec_schedule(e)
    for pos in range(16):
        for v in range(256):
            blk = base[:pos] + bytes([v]) + base[pos + 1:]
            assert block(e, blk) == codec.aes_block(key, blk), (pos, v)
            assert block(d, blk, inv=True) == codec.aes_block(key, blk, decrypt=True), (pos, v)
    # the modes: an IV whose low half is all ones (the carry into the high half), any start position; CBC without its padding block
    key, iv, data = bytes(rnd.getrandbits(8) for _ in range(32)), bytes(8) + b"\xff" * 8, bytes(rnd.getrandbits(8) for _ in range(100))
    for pos in (0, 1, 16, 17, 4095):
        assert ctr(key, iv, data, pos) == codec.aes_ctr(key, iv, data, pos=pos), pos
    assert cbc(key, iv, data[:96]) == codec.aes_cbc_encrypt(key, iv, data[:96])[:96]
    assert codec.aes_ctr(SP_KEY, CTR_IV, SP_PT) == CTR_CT and codec.aes_cbc_encrypt(SP_KEY, CBC_IV, SP_PT)[:64] == CBC_CT


def test_sanitizer_program():
    out = built()
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([os.path.join(out, "aes_host_san")], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "403 checks, 0 bad" in r.stdout
