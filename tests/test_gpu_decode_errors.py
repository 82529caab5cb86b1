"""The decoders' error contract: what a failing decompress_batch call returns -- (return code, pna_gpu_last_error text) -- for a fixed list of small bad
inputs, compared with tests/golden/decode_errors.json.  The fixture was recorded on an MI355X with the library as it stood BEFORE the decoders' host side
was cut into stages (`python tests/test_gpu_decode_errors.py --record`), so that the cut is held to every code and every text, byte for byte.

Every case runs on a fresh context with default options (the fallback case sets its two options), every input is at most 3 MiB.  Inputs come from
codec.corpus_file with fixed seeds, from this library's own encoder (deterministic: the oracle's model is bit-exact with it), and from the system's
libzstd / zlib / liblzma (the stdlib's lzma module, as tests/xz_cases.py uses it); a case whose writer is absent is skipped.

Masked numbers: none.  Two recordings of the unchanged library gave the same text for every case, `produced N of` included, so the comparison is exact."""
import json
import lzma
import os
import sys
import zlib

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "decode_errors.json")
MIB = 1 << 20
LIBZSTD_CASES = {"zstd foreign two frames hold more than the entry"}   # the cases whose input the system libzstd writes: skipped where it is absent


def _flip(b, at):
    return b[:at] + bytes([b[at] ^ 0x5A]) + b[at + 1:]


def _cases(pna, codec):
    """[(name, algo, payloads, raw sizes, options)] -- the writers run once, every case is a list of host payloads for decompress_batch"""
    import torch  # noqa: F401  (shares its HIP runtime with the extension)
    out = []
    raws = [codec.corpus_file(0, 7101, 100000), codec.corpus_file(1, 7102, 200000), codec.corpus_file(2, 7103, 50000)]
    two_mib = codec.corpus_file(0, 7104, 2 * MIB)
    with pna.Context(0) as enc:
        enc.set_option("latency_max_mib", 0)
        own = enc.compress_batch(raws)
        enc.set_option("single_frame", 1)
        single = enc.compress_batch([two_mib], level=1)[0]
    sizes = [len(r) for r in raws]
    out.append(("zstd flipped byte in the middle entry", pna.ALGO_ZSTD, [own[0], _flip(own[1], len(own[1]) // 2), own[2]], sizes, {}))
    out.append(("zstd truncated frame", pna.ALGO_ZSTD, [own[1][:len(own[1]) * 2 // 3]], [sizes[1]], {}))
    out.append(("zstd raw size minus one", pna.ALGO_ZSTD, [own[1]], [sizes[1] - 1], {}))
    out.append(("zstd raw size plus one", pna.ALGO_ZSTD, [own[1]], [sizes[1] + 1], {}))
    if codec.system_libzstd() is not None:
        two = codec.libzstd_compress(raws[0], 3) + codec.libzstd_compress(raws[1], 3)
        out.append(("zstd foreign two frames hold more than the entry", pna.ALGO_ZSTD, [two], [sizes[0] + sizes[1] - 10], {}))
    out.append(("zstd one-workgroup fallback refused", pna.ALGO_ZSTD, [single], [len(two_mib)], {"zdec_serial": 1, "zdec_fallback_max_mib": 1}))
    out.append(("zstd garbage", pna.ALGO_ZSTD, [codec.corpus_file(2, 7105, 4096)], [10000], {}))
    text300k = codec.corpus_file(0, 7106, 300 << 10)
    z = zlib.compress(text300k, 6)
    out.append(("zlib flipped byte", pna.ALGO_DEFLATE, [_flip(z, len(z) // 2)], [len(text300k)], {}))
    out.append(("zlib wrong adler-32", pna.ALGO_DEFLATE, [z[:-1] + bytes([z[-1] ^ 0xFF])], [len(text300k)], {}))
    out.append(("zlib raw size minus one", pna.ALGO_DEFLATE, [z], [len(text300k) - 1], {}))
    out.append(("zlib raw size plus one", pna.ALGO_DEFLATE, [z], [len(text300k) + 1], {}))
    co = zlib.compressobj(6, zlib.DEFLATED, 15, 8, zlib.Z_DEFAULT_STRATEGY, text300k[:1000])
    out.append(("zlib preset dictionary", pna.ALGO_DEFLATE, [co.compress(text300k[:50000]) + co.flush()], [50000], {}))
    x = lzma.compress(text300k, format=lzma.FORMAT_XZ, check=lzma.CHECK_CRC64, preset=6)
    out.append(("xz raw size minus one", pna.ALGO_XZ, [x], [len(text300k) - 1], {}))
    out.append(("xz damaged block", pna.ALGO_XZ, [_flip(x, len(x) // 2)], [len(text300k)], {}))
    return out


def _outcome(pna, case):
    """[return code, pna_gpu_last_error text] of the case's decompress_batch call on a fresh context: PnaGpuError carries the code, and the text behind its prefix"""
    name, algo, payloads, sizes, options = case
    with pna.Context(0) as ctx:
        for k, v in options.items():
            ctx.set_option(k, v)
        try:
            ctx.decompress_batch(payloads, sizes, algo=algo)
        except pna.PnaGpuError as e:
            prefix = f"pna_gpu error {e.code}: "
            assert str(e).startswith(prefix)
            return [e.code, str(e)[len(prefix):]]
    return [0, ""]


@pytest.fixture(scope="module")
def cases(pna, codec):
    return {c[0]: c for c in _cases(pna, codec)}


RECORDED = {}
if os.path.exists(FIXTURE):
    with open(FIXTURE) as _f:
        RECORDED = json.load(_f)


@pytest.mark.parametrize("name", sorted(RECORDED))
def test_failing_call_returns_the_recorded_code_and_text(pna, codec, cases, name):
    if name in LIBZSTD_CASES and codec.system_libzstd() is None:
        pytest.skip("the writer of this case's input (system libzstd) is absent")
    got = _outcome(pna, cases[name])                            # (a recorded case that _cases no longer makes fails here)
    print(name, got)
    assert got[0] != 0, "the call must fail"
    assert got == RECORDED[name]


def test_every_case_is_recorded(cases):
    assert set(cases) <= set(RECORDED) and len(RECORDED) >= 13


if __name__ == "__main__":
    if len(sys.argv) < 2 or sys.argv[1] != "--record":
        sys.exit("usage: test_gpu_decode_errors.py --record [file]   (run it with the library whose behaviour is the contract)")
    sys.path.insert(0, ROOT)
    import importlib
    pna_mod = importlib.import_module("portable-network-archive_amd")
    from oracle import codec as codec_mod
    rec = {c[0]: _outcome(pna_mod, c) for c in _cases(pna_mod, codec_mod)}
    with open(sys.argv[2] if len(sys.argv) > 2 else FIXTURE, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    for k in sorted(rec):
        print(k, rec[k])
