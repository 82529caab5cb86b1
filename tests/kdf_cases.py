"""The key derivation cases that tests/test_kdf_core.py (CPU: csrc/kdf_core.h built with g++ alone) and tests/test_gpu_kdf.py (pna_gpu_kdf_batch) share,
the CPU build of kdf_core.h, and the case list as pna_gpu_kdf_batch jobs.

Argon2 -- expected keys from oracle.codec.argon2, an independent C implementation that the reference's encrypted fixtures pin:
  the three kinds; m in {8, 9, 11, 16, 50, 64, 1024, 4096} KiB (8: segments of two blocks, pass 0 slice 0 has no step; 9 and 11 round down to 8; 1024:
  segments of 256 blocks, the data-independent address block is made again inside a segment); t in {1, 2, 3} (with and without the XOR of the old
  block); p in {1, 2, 4} with m at and just above 8 p; passwords of 0, 1, 55, 87, 88, 89 and 300 bytes (H0's input crosses a BLAKE2b block edge:
  the 40 bytes of parameters and lengths, the password, an 8 / 16 / 48-byte salt); salts of 8, 16 and 48 bytes.
PBKDF2 -- expected keys from hashlib.pbkdf2_hmac: rounds 1, 2, 1000, 4096; passwords of 0, 63, 64, 65, 200 bytes (beyond 64 the key is hashed first);
  salts of 1, 51, 52, 55, 56, 64 bytes (salt || INT(1) crosses SHA-256's padding edge at 55 / 56 message bytes)."""
import ctypes
import functools
import hashlib
import os
import random
import subprocess
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(tempfile.gettempdir(), "pna_kdf_core_%d" % os.getuid())
ARGON2D, ARGON2I, ARGON2ID, PBKDF2 = 0, 1, 2, 3                  # pna_kdf_job.kind

PW_LENS = (0, 1, 55, 87, 88, 89, 300)
SALT_LENS = (8, 16, 48)


def _bytes(seed, n):
    rnd = random.Random(seed)
    return bytes(rnd.getrandbits(8) for _ in range(n))


@functools.lru_cache(maxsize=None)
def argon_cases():
    """(kind, t, m, p, password, salt) -- every kind meets every m, every t and every p; password and salt lengths go round"""
    out, k = [], 0
    def add(kind, t, m, p):
        nonlocal k
        out.append((kind, t, m, p, _bytes(1000 + k, PW_LENS[k % 7]), _bytes(2000 + k, SALT_LENS[k % 3])))
        k += 1
    for kind in (ARGON2D, ARGON2I, ARGON2ID):
        for mi, m in enumerate((8, 9, 11, 16, 50, 64, 1024, 4096)):
            add(kind, 1 + (mi + kind) % 3, m, 1)
        for p in (2, 4):
            for mi, m in enumerate((8 * p, 8 * p + 1, 64, 1024)):
                add(kind, 1 + (mi + kind + p) % 3, m, p)
    add(ARGON2ID, 3, 4096, 4)
    add(ARGON2I, 2, 1024, 1)                                      # Argon2i with the XOR pass and a second address block per segment
    for i, n in enumerate(PW_LENS):                               # every password length with every kind at one small shape
        for kind in (ARGON2D, ARGON2I, ARGON2ID):
            out.append((kind, 2, 16, 1, _bytes(3000 + i, n), _bytes(4000 + i, SALT_LENS[i % 3])))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def pbkdf2_cases():
    """(rounds, password, salt): the full product"""
    return tuple((r, _bytes(5000 + pl, pl), _bytes(6000 + sl, sl)) for r in (1, 2, 1000, 4096) for pl in (0, 63, 64, 65, 200) for sl in (1, 51, 52, 55, 56, 64))


@functools.lru_cache(maxsize=None)
def argon_expected():
    from oracle import codec
    return tuple(codec.argon2(kind, pw, salt, t, m, p) for kind, t, m, p, pw, salt in argon_cases())


@functools.lru_cache(maxsize=None)
def pbkdf2_expected():
    return tuple(hashlib.pbkdf2_hmac("sha256", pw, salt, r, 32) for r, pw, salt in pbkdf2_cases())


@functools.lru_cache(maxsize=None)
def built() -> str:
    subprocess.run(["make", "-s", "-C", os.path.join(HERE, "kdf_core"), "OUT=" + OUT, "lib", "san"], check=True)
    return OUT


@functools.lru_cache(maxsize=None)
def lib():
    return ctypes.CDLL(os.path.join(built(), "libkdf_host.so"))


def argon2(kind, pw, salt, t, m, p, n=32):
    out = ctypes.create_string_buffer(n)
    rc = lib().kdf_argon2_c(kind, pw, ctypes.c_size_t(len(pw)), salt, ctypes.c_size_t(len(salt)), t, m, p, out, n)
    if rc:
        raise ValueError("kdf_argon2_c: %d" % rc)
    return out.raw


def pbkdf2(pw, salt, rounds):
    out = ctypes.create_string_buffer(32)
    lib().kdf_pbkdf2_c(pw, ctypes.c_size_t(len(pw)), salt, ctypes.c_size_t(len(salt)), rounds, out)
    return out.raw


def case_file_text():
    h = lambda x: x.hex() or "-"
    lines = ["argon2 %d %d %d %d %s %s %s" % (kind, t, m, p, h(pw), h(salt), key.hex()) for (kind, t, m, p, pw, salt), key in zip(argon_cases(), argon_expected())]
    lines += ["pbkdf2 %d %s %s %s" % (r, h(pw), h(salt), key.hex()) for (r, pw, salt), key in zip(pbkdf2_cases(), pbkdf2_expected())]
    return "\n".join(lines) + "\n"


def jobs_one_password(password):
    """The case list's shapes as pna_gpu_kdf_batch jobs under ONE password (a batch has one), with the keys the host functions' models give:
    (jobs, expected).  The password lengths of the list are covered by calling this once per length."""
    from oracle import codec
    jobs, want = [], []
    for kind, t, m, p, _, salt in argon_cases():
        jobs.append({"kind": kind, "t_cost": t, "m_cost_kib": m, "lanes": p, "salt": salt})
        want.append(codec.argon2(kind, password, salt, t, m, p))
    for r, _, salt in pbkdf2_cases():
        jobs.append({"kind": PBKDF2, "rounds": r, "salt": salt})
        want.append(hashlib.pbkdf2_hmac("sha256", password, salt, r, 32))
    return jobs, want
