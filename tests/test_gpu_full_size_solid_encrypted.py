"""`pna create --solid --aes ctr|gcm` beyond the device form's limit (run with -m gpu): one inner entry of 2.3 GiB from PAGEABLE host memory through
pna_gpu_create_solid_archive_enc_host (pna_gpu_create_solid_archive_enc_device refuses inner entries of 2 GiB and more).  Every chunk CRC is checked,
the SDAT bodies are decrypted by the oracle (GCM: every segment tag and the final flag), zlib decodes the result as one stream and it is compared piece
by piece with the oracle writer's inner entries; page-locked memory stays within the header's bound."""
import ctypes
import struct
import zlib

import pytest

pytestmark = pytest.mark.gpu

GIB = 1 << 30


def _pinned(ctx):
    ctx._L.pna_gpu_debug_pinned_bytes.restype = ctypes.c_uint64
    ctx._L.pna_gpu_debug_pinned_bytes.argtypes = [ctypes.c_void_p]
    return ctx._L.pna_gpu_debug_pinned_bytes(ctx._h)


@pytest.mark.parametrize("mode", ["ctr", "gcm"])
def test_encrypted_solid_entry_beyond_2gib(big_ctx, pna, pf, codec, mode):
    import numpy as np
    import torch
    ctx = big_ctx
    free, _ = torch.cuda.mem_get_info()
    assert free >= 16 * GIB, f"the full-size case needs 16 GiB of free HBM, found {free >> 30} GiB: an MI355X has 288 GB"
    L = 2 * GIB + (300 << 20) + 4321
    big = np.zeros(L, dtype=np.uint8)                                          # mostly zeros (the oracle decrypts every byte of the output) ...
    for i, o in enumerate(range(0, L - (1 << 18), 61 << 20)):                  # ... with text every 61 MiB
        big[o:o + (1 << 18)] = np.frombuffer(codec.corpus_file(i % 2, 9700 + i, 1 << 18), dtype=np.uint8)
    small = [codec.corpus_file(0, 9690, 100000), b"", codec.corpus_file(1, 9691, 70000)]
    views = [small[0], memoryview(big), small[1], small[2]]
    names = ["x/head.txt", "x/big.bin", "x/empty", "x/tail.txt"]
    key, phsf = pna.kdf_pbkdf2_sha256(b"password", bytes(range(16)), 1000)
    G = 1 << 20
    cipher = pna.Cipher(key, phsf, pna.MODE_CTR if mode == "ctr" else pna.MODE_GCM, ivs=bytes(range(16)) if mode == "ctr" else bytes(range(39)),
                        gcm_segment_size=G if mode == "gcm" else 0)
    W = 64 << 20
    ctx.set_option("solid_win_mib", W >> 20)
    arc = ctx.create_solid_archive_enc_host(names, views, algo=pna.ALGO_DEFLATE, cipher=cipher)
    assert _pinned(ctx) <= 6 * W + 3 * G, _pinned(ctx)                    # four window slots (grown with headroom) and the GCM carry room: not the entry

    # ---- structure and every chunk CRC (the oracle's reader checks them), then the oracle's decryption
    (so,) = pf.read_archive(arc)[1]
    assert (so.encryption, so.cipher_mode) == (1, 1 if mode == "ctr" else 2)
    if mode == "ctr":
        comp = codec.decrypt_payload(1, 1, key, so.data)
    else:
        bodies = [d for ty, d in so.chunks if ty == b"SDAT"]
        assert len(bodies) > 2 and all(len(b) == G + 16 for b in bodies[1:-1])      # the stream header, then full segments but the last
        comp = codec.decrypt_payload_gcm(key, so.data, b"SHED", pf.solid_header_bytes(pna.ALGO_DEFLATE, 1, 2), phsf.encode())

    # ---- the inner stream, piece by piece from the oracle's writer
    def expected_pieces():
        for nm, v in zip(names, views):
            v = np.frombuffer(v, dtype=np.uint8)
            hdr = pf.write_chunk(b"FHED", pf.file_entry_header(0, pf.sanitize_name(nm))) + pf.write_chunk(b"fSIZ", pf.fsiz_bytes(len(v)))
            yield np.frombuffer(hdr, dtype=np.uint8)
            if len(v):
                yield np.frombuffer(struct.pack(">I", len(v)) + b"FDAT", dtype=np.uint8)
                crc = zlib.crc32(b"FDAT")
                for a in range(0, len(v), 256 << 20):
                    crc = zlib.crc32(v[a:a + (256 << 20)], crc)
                    yield v[a:a + (256 << 20)]
                yield np.frombuffer(struct.pack(">I", crc), dtype=np.uint8)
            yield np.frombuffer(pf.write_chunk(b"FEND"), dtype=np.uint8)
    want = expected_pieces()
    cur = [np.zeros(0, dtype=np.uint8)]
    seen = [0]

    def check(out):
        o = np.frombuffer(out, dtype=np.uint8)
        while len(o):
            while not len(cur[0]):
                cur[0] = next(want)
            k = min(len(o), len(cur[0]))
            assert np.array_equal(o[:k], cur[0][:k]), seen[0]
            o, cur[0], seen[0] = o[k:], cur[0][k:], seen[0] + k
    d = zlib.decompressobj()
    for a in range(0, len(comp), 1 << 20):
        while True:
            out = d.decompress(comp[a:a + (1 << 20)] if not d.unconsumed_tail else d.unconsumed_tail, 64 << 20)
            check(out)
            if not d.unconsumed_tail:
                break
    check(d.flush())
    assert d.eof and d.unused_data == b"" and not len(cur[0]) and next(want, None) is None
    assert seen[0] > L
    ctx.set_option("solid_win_mib", 256)
