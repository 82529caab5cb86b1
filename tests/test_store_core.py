"""The chunk CRC algebra on the CPU (csrc/crc_core.h: the raw register update, the multiplication by x^(8k) mod P, and the fold of the raw registers of a
chunk's pieces into the chunk's CRC -- what k_store leaves behind and k_store_fold folds).  tests/store_core/store_host.cpp is a stand-alone program: for
the lengths 0 .. 300 and the piece and tile edges up to 3 MiB + 17 it splits "FDAT" || data at every cut of its list (one-byte pieces, a cut inside the
type, uneven pieces, k_store's 1 MiB pieces) and compares the folded registers with a bitwise CRC-32 of its own; it also runs k_store_fold's 64-lane schedule
(crc_fold_lane) over chunks of 1 .. 200 pieces and of up to 130 MiB + 7 bytes.  Built with g++ alone, once plain and
once under -fsanitize=address,undefined; both are run as programs, nothing is loaded into this process.  This side compares the program's samples
with zlib.crc32."""
import functools
import os
import subprocess
import tempfile
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(tempfile.gettempdir(), "pna_store_core_%d" % os.getuid())


@functools.lru_cache(maxsize=None)
def built() -> str:
    subprocess.run(["make", "-s", "-C", os.path.join(HERE, "store_core"), "OUT=" + OUT, "plain", "san"], check=True)
    return OUT


@functools.lru_cache(maxsize=None)
def run(program: str):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    return subprocess.run([os.path.join(built(), program)], capture_output=True, text=True, env=env)


def message(n: int) -> bytes:
    """"FDAT" || data of the program's length-n case: data byte i = ((i * 2654435761 mod 2^32) >> 13 ^ n) & 255"""
    i = np.arange(n, dtype=np.uint64)
    return b"FDAT" + ((((i * 2654435761) & 0xFFFFFFFF) >> 13) ^ n).astype(np.uint8).tobytes()


def test_every_cut_folds_to_the_bitwise_crc():
    r = run("store_host")
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("4820 checks, 0 bad"), r.stdout[-400:]


def test_samples_agree_with_zlib():
    r = run("store_host")
    samples = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("sample ")]
    assert [int(s[1]) for s in samples] == [0, 1, 300, 4097, 1048577, 3145745]
    for _s, n, crc in samples:
        assert int(crc, 16) == zlib.crc32(message(int(n))), n


def test_lane_schedule_agrees_with_zlib():
    """k_store_fold's schedule (crc_fold_lane on 64 lanes, pieces of 1 MiB): chunks of up to 64 pieces, of more, and of more with a short last piece"""
    r = run("store_host")
    lanes = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("lanes ")]
    assert [int(s[1]) for s in lanes] == [(3 << 20) + 17, 64 << 20, (64 << 20) + 5, (65 << 20) - 16, 65 << 20, (130 << 20) + 7]
    for _s, n, crc in lanes:
        assert int(crc, 16) == zlib.crc32(message(int(n))), n


def test_sanitizer_program():
    r = run("store_host_san")
    assert r.returncode == 0, r.stdout + r.stderr
    assert "4820 checks, 0 bad" in r.stdout and r.stdout == run("store_host").stdout
