"""The mode bodies of k_cipher.hip (ctr_body, cbc_enc_body, cbc_dec_body), which AES-256 and Camellia-256 share: one case list, run under both
ciphers, against the CPU models -- oracle/codec.py (oracle/cipher_model.c) for AES, tests/camellia_cases.py (csrc/camellia_core.h) for Camellia.
Integer work: bit-exact.  The shapes are the smallest at which the shared code can go wrong and that no other test asserts already:

  * CTR through cipher_apply_device under an IV whose low 8 bytes are all 0xFF, stream bytes 0 .. 48: the 64-bit carry into the high half fires at
    block 1, and the range ends in a partial block.
  * CTR units that start inside a keystream block, under the same IV: archives written with max_chunk_size 17, whose FDAT chunk k is the CTR unit at
    stream position 17 k (layout_entries).  Payloads of 18, 32 and 40 bytes give units at position 17 of length 1 (inside block 1), 15 (block 1 from
    its second byte to its end) and 17 (a clipped head in block 1, a clipped tail in block 2), all in the block whose counter carried.
  * CBC decryption through the extract driver (its only entry point) of ciphertexts of exactly 16, 4 096 and 4 112 bytes -- one block, one full
    256-block step, and the carry through LDS into a second step -- and one with its last ciphertext byte flipped: the bad-padding error.

Asserted elsewhere for both ciphers, and therefore not repeated: CBC encryption of lengths 0, 15, 16, 17 and CTR ranges of 256 KiB + 1 bytes (two
units) -- test_gpu_cipher.py::test_cbc_encrypt_equals_oracle / test_ctr_ranges_equal_oracle, test_gpu_camellia.py::test_cbc_encrypt_equals_cpu_core /
test_ctr_ranges_equal_cpu_core.  One shape of the list cannot be produced: a unit at stream position 17 of length 31.  A unit's position is
k * max_chunk_size + a multiple of 256 KiB (chunked archives), a multiple of 256 KiB (cipher_apply_device, GCM segments), or where a solid window's
compressed output happens to begin; position 17 therefore needs max_chunk_size 17 (or 1), which bounds the length by 17."""
import zlib

import pytest

import camellia_cases as C

pytestmark = pytest.mark.gpu

PW = b"password"
CARRY_IV = bytes(8) + b"\xff" * 8
CT_LENS = [16, 4096, 4112]


@pytest.fixture(scope="module")
def ctx(pna):
    import torch  # noqa: F401  (shares its HIP runtime with the extension)
    c = pna.Context(0)
    c.set_option("camellia", 1)
    yield c
    c.close()


@pytest.fixture(scope="module")
def keyed(pna):
    return pna.kdf_pbkdf2_sha256(PW, bytes(range(16)), 1000)           # (key, phsf) that the read side derives again from the password


class Model:
    """the CPU model of one cipher"""
    def __init__(self, pna, codec, name):
        self.enc = pna.ENC_CAMELLIA if name == "camellia" else pna.ENC_AES
        self.ctr = C.ctr if name == "camellia" else codec.aes_ctr
        self.cbc_decrypt = C.cbc_decrypt if name == "camellia" else codec.aes_cbc_decrypt


@pytest.fixture(params=["aes", "camellia"])
def model(request, pna, codec):
    return Model(pna, codec, request.param)


def test_ctr_carry_into_the_high_half(pna, ctx, codec, model, keyed):
    import torch
    key, phsf = keyed
    data = codec.corpus_file(2, 31, 49)
    flat = b"\xA5" * 3 + data + b"\xA5" * 12                          # an odd byte offset in the buffer, guard bytes around
    buf = torch.frombuffer(bytearray(flat), dtype=torch.uint8).cuda()
    ci = pna.Cipher(key, phsf, pna.MODE_CTR, ivs=CARRY_IV, encryption=model.enc)
    ctx.cipher_apply_device(ci, buf.data_ptr(), [3], [49])
    got = bytes(buf.cpu().numpy())
    want = model.ctr(key, CARRY_IV, data)
    assert got == b"\xA5" * 3 + want + b"\xA5" * 12
    # block 1's counter is 2^64: the keystream of bytes 16 .. 48 is that of the IV 0..0 1 0..0 from its start
    assert want[16:] == model.ctr(key, bytes(7) + b"\x01" + bytes(8), data[16:])


def stored_entries(pna, ctx, codec, seed, payload_lens):
    """Incompressible entries whose stored zlib streams (deflate level 0) have exactly the given lengths"""
    over = len(ctx.compress_batch([codec.corpus_file(2, 40, 1000)], algo=pna.ALGO_DEFLATE, level=0)[0]) - 1000
    assert 0 < over <= 12
    ents = [codec.corpus_file(2, seed + i, n - over) for i, n in enumerate(payload_lens)]
    payloads = ctx.compress_batch(ents, algo=pna.ALGO_DEFLATE, level=0)
    assert [len(p) for p in payloads] == list(payload_lens)
    return ents, payloads


def test_ctr_units_inside_a_keystream_block(pna, ctx, pf, codec, model, keyed):
    key, phsf = keyed
    lens = [18, 32, 40]
    ents, payloads = stored_entries(pna, ctx, codec, 60, lens)
    names = ["u/%d" % n for n in lens]
    ci = pna.Cipher(key, phsf, pna.MODE_CTR, ivs=CARRY_IV * len(lens), encryption=model.enc)
    arc = pna.create_archive_chunked(ctx, names, ents, 17, algo=pna.ALGO_DEFLATE, level=0, cipher=ci)
    items = pf.read_archive(arc)[1]
    # FDAT(iv), then the ciphertext in chunks of 17 bytes: chunk k is the unit at stream position 17 k
    chunks = [[d for ty, d in it.chunks if ty == b"FDAT"] for it in items]
    assert [[len(d) for d in ch] for ch in chunks] == [[16, 17, 1], [16, 17, 15], [16, 17, 17, 6]]
    for ch, pl in zip(chunks, payloads):
        assert ch[0] == CARRY_IV
        for k, d in enumerate(ch[1:]):
            assert d == model.ctr(key, CARRY_IV, pl[17 * k:17 * k + len(d)], pos=17 * k), (len(pl), k)
        assert b"".join(ch[1:]) == model.ctr(key, CARRY_IV, pl)
    assert pna.extract_archive(ctx, arc, PW) == [(n, 0, e) for n, e in zip(names, ents)]


@pytest.fixture(scope="module")
def stored(pna, ctx, codec):
    """... one byte short of the wanted ciphertext lengths: a padding of one byte"""
    return stored_entries(pna, ctx, codec, 41, [n - 1 for n in CT_LENS])[0]


def test_cbc_decrypt_steps_and_padding(pna, ctx, pf, codec, model, keyed, stored):
    key, phsf = keyed
    names = ["s/%d" % n for n in CT_LENS]
    ivs = bytes(range(48))
    ci = pna.Cipher(key, phsf, pna.MODE_CBC, ivs=ivs, encryption=model.enc)
    arc = pna.create_archive_encrypted(ctx, names, stored, b"", algo=pna.ALGO_DEFLATE, level=0, cipher=ci)
    items = pf.read_archive(arc)[1]
    # the data chunks hold IV || ciphertext: the ciphertexts have the lengths this test is about
    assert [len(it.data) - 16 for it in items] == CT_LENS
    for i, (it, e) in enumerate(zip(items, stored)):
        assert it.data[:16] == ivs[16 * i:16 * i + 16] and (it.encryption, it.cipher_mode) == (model.enc, pna.MODE_CBC)
        plain = model.cbc_decrypt(key, it.data[:16], it.data[16:])
        assert len(plain) == CT_LENS[i] - 1 and codec.decode_payload(pna.ALGO_DEFLATE, plain, len(e) + 64) == e
    assert pna.extract_archive(ctx, arc, PW) == [(n, 0, e) for n, e in zip(names, stored)]
    # the last ciphertext byte of the two-step entry flipped, its chunk CRC repaired: the padding check of the last block says so
    body = [d for ty, d in items[2].chunks if ty == b"FDAT"][-1]
    at = arc.index(body)
    bad = bytearray(arc); bad[at + len(body) - 1] ^= 1
    bad[at + len(body):at + len(body) + 4] = (zlib.crc32(bytes(bad[at:at + len(body)]), zlib.crc32(b"FDAT")) & 0xFFFFFFFF).to_bytes(4, "big")
    with pytest.raises(ValueError):
        model.cbc_decrypt(key, items[2].data[:16], items[2].data[16:-1] + bytes([items[2].data[-1] ^ 1]))
    with pytest.raises(pna.PnaGpuError) as ei:
        pna.extract_archive(ctx, bytes(bad), PW)
    assert ei.value.code == -2 and "CBC: bad length or padding" in str(ei.value)
