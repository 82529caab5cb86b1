"""Stored blocks as chunk starts of the chunk decoder (k_ispec's stored trial, k_inflate's chunk mode).  zlib and miniz_oxide write STORED blocks for
incompressible data; such a stream has no dynamic block header to split at, and until stored blocks were block starts it was walked by one wave (about
107 s per GiB).  Every stream here must decode byte-exact through the chunk decoder -- known size, open size, measured size -- and damage must be refused
or decode differently."""
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MIB = 1 << 20


def _random(n, seed):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def _deflate(data, level, piece=16 * MIB):
    co = zlib.compressobj(level)
    return b"".join([co.compress(data[a:a + piece]) for a in range(0, len(data), piece)] + [co.flush()])


def _stored_only():
    raw = _random(96 * MIB + 12345, 1)
    return raw, zlib.compress(raw, 0)


def _mixed(codec):
    """1 MiB stretches of random bytes (stored blocks) and corpus text (dynamic blocks), one after the other."""
    text = codec.corpus_file(0, 77, 8 * MIB)
    parts = []
    for k in range(16):
        parts.append(_random(MIB + 17 * k, 100 + k) if k % 2 == 0 else text[(k // 2) * MIB:(k // 2 + 1) * MIB - 3 * k])
    raw = b"".join(parts)
    return raw, _deflate(raw, 6)


def _lookalike_dyn(codec):
    """The first bytes of a raw deflate stream of text: a non-final dynamic block header that passes k_ispec's trial."""
    co = zlib.compressobj(6, zlib.DEFLATED, -15)
    d = co.compress(codec.corpus_file(0, 5, 2 * MIB)) + co.flush()
    assert d[0] & 7 == 4                                         # BFINAL 0, BTYPE 2
    return d[:600]


def _lookalike_stored():
    """A stored block header (zero byte, LEN, NLEN) whose 40 bytes are followed by another such header: what k_ispec's stored trial accepts."""
    return b"\x00\x28\x00\xd7\xff" + bytes(range(40)) + b"\x00\x10\x00\xef\xff" + bytes(16)


def _planted(codec):
    """Stored data with block-header look-alikes planted in it, one per 256 KiB, alternately dynamic and stored: false starts the chain repair must drop."""
    raw = bytearray(_random(64 * MIB, 7))
    dyn, sto = _lookalike_dyn(codec), _lookalike_stored()
    for k, at in enumerate(range(100000, len(raw) - 4096, 256 * 1024)):
        la = dyn if k % 2 == 0 else sto
        raw[at:at + len(la)] = la
    raw = bytes(raw)
    return raw, zlib.compress(raw, 0)


def _shapes(codec):
    return {"stored_only": _stored_only, "mixed": lambda: _mixed(codec), "planted": lambda: _planted(codec)}


@pytest.fixture(scope="module", params=["stored_only", "mixed", "planted"])
def stream(request, codec):
    raw, comp = _shapes(codec)[request.param]()
    assert zlib.decompress(comp) == raw
    return request.param, raw, comp


def _dev(b):
    import torch
    return torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()


def test_known_size_decodes_in_chunks(gpu_ctx, pna, stream):
    import torch
    _, raw, comp = stream
    d_src, want = _dev(comp), _dev(raw)
    out = torch.zeros(len(raw) + 64, dtype=torch.uint8, device="cuda")
    gpu_ctx.decompress_batch_device(d_src.data_ptr(), [0], [len(comp)], out.data_ptr(), [0], [len(raw)], algo=pna.ALGO_DEFLATE)
    assert gpu_ctx.timing().lz_match_launches == 1                   # (the streams that went through the chunk decoder)
    assert torch.equal(out[:len(raw)], want)


def test_open_size_decodes_in_chunks(gpu_ctx, pna, stream):
    import torch
    _, raw, comp = stream
    d_src, want = _dev(comp), _dev(raw)
    assert gpu_ctx.open_size_device(d_src.data_ptr(), 0, len(comp), algo=pna.ALGO_DEFLATE) == (len(raw), True)
    out = torch.zeros(len(raw) + 4096, dtype=torch.uint8, device="cuda")
    got = gpu_ctx.inflate_open_device(d_src.data_ptr(), 0, len(comp), out.data_ptr(), 0, len(raw) + 4096)
    assert gpu_ctx.timing().lz_match_launches == 1
    assert got == len(raw)
    assert torch.equal(out[:len(raw)], want)


def _stored_headers(comp):
    """Byte positions of the stored block headers of a level-0 zlib stream (each on a byte boundary, LEN / NLEN behind it)."""
    pos, out = 2, []
    while True:
        out.append(pos)
        n = comp[pos + 1] | comp[pos + 2] << 8
        if comp[pos] & 1:
            return out
        pos += 5 + n


@pytest.mark.parametrize("where", ["len", "nlen", "btype", "bfinal", "data"])
def test_damage_is_refused_or_decodes_differently(gpu_ctx, pna, where):
    import torch
    raw, comp = _stored_only()
    heads = _stored_headers(comp)
    h = heads[len(heads) // 2]
    at, bit = {"len": (h + 1, 0x04), "nlen": (h + 4, 0x20), "btype": (h, 0x02), "bfinal": (h, 0x01), "data": (h + 5 + 3000, 0x10)}[where]
    bad = bytearray(comp)
    bad[at] ^= bit
    d_src, want = _dev(bytes(bad)), _dev(raw)
    out = torch.zeros(len(raw) + 4096, dtype=torch.uint8, device="cuda")
    for call in ("known", "open"):
        out.zero_()
        try:
            if call == "known":
                gpu_ctx.decompress_batch_device(d_src.data_ptr(), [0], [len(comp)], out.data_ptr(), [0], [len(raw)], algo=pna.ALGO_DEFLATE)
                got = len(raw)
            else:
                got = gpu_ctx.inflate_open_device(d_src.data_ptr(), 0, len(comp), out.data_ptr(), 0, len(raw) + 4096)
            same = got == len(raw) and torch.equal(out[:len(raw)], want)
        except pna.PnaGpuError:
            same = False
        assert not same, call
