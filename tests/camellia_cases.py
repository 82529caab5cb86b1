"""Camellia-256 on the CPU for the tests: csrc/camellia_core.h built with g++ alone (tests/camellia_core) and loaded with ctypes -- the model that
tests/test_camellia_core.py pins against openssl's answers and the reference's archives, and that tests/test_gpu_camellia.py holds the device against.
GCM STREAM's key derivation, nonces and segmenting are the oracle's (oracle/codec.py, cipher-independent); GHASH is written out here."""
import ctypes
import functools
import json
import os
import subprocess
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
OUT = os.path.join(tempfile.gettempdir(), "pna_camellia_core_%d" % os.getuid())
ENC_CAMELLIA = 2


@functools.lru_cache(maxsize=None)
def built() -> str:
    subprocess.run(["make", "-s", "-C", os.path.join(HERE, "camellia_core"), "OUT=" + OUT, "lib", "san"], check=True)
    return OUT


@functools.lru_cache(maxsize=None)
def lib():
    L = ctypes.CDLL(os.path.join(built(), "libcam_host.so"))
    L.cam_cbc_dec_c.restype = ctypes.c_long
    return L


@functools.lru_cache(maxsize=None)
def kat():
    with open(os.path.join(GOLDEN, "camellia_kat.json")) as f:
        return json.load(f)["cases"]


def schedule(key: bytes):
    out = (ctypes.c_uint32 * 68)()
    lib().cam_expand_c(bytes(key), out)
    return out


def dec_schedule(sched):
    out = (ctypes.c_uint32 * 68)()
    lib().cam_dec_key_c(sched, out)
    return out


def block(sched, data: bytes) -> bytes:
    """the table form: one block under a schedule (the encryption order encrypts, the decrypt order decrypts)"""
    out = ctypes.create_string_buffer(16)
    lib().cam_block_c(sched, bytes(data), out)
    return out.raw


def ref_block(key: bytes, data: bytes, decrypt: bool = False) -> bytes:
    """the byte-wise form"""
    out = ctypes.create_string_buffer(16)
    lib().cam_ref_block_c(bytes(key), int(decrypt), bytes(data), out)
    return out.raw


def ecb(key: bytes, data: bytes, decrypt: bool = False) -> bytes:
    out = ctypes.create_string_buffer(max(len(data), 1))
    lib().cam_ecb_c(bytes(key), int(decrypt), bytes(data), ctypes.c_size_t(len(data) // 16), out)
    return out.raw[:len(data)]


def ctr(key: bytes, iv: bytes, data: bytes, pos: int = 0) -> bytes:
    buf = ctypes.create_string_buffer(bytes(data), max(len(data), 1))
    lib().cam_ctr_c(bytes(key), bytes(iv), ctypes.c_uint64(pos), buf, ctypes.c_size_t(len(data)))
    return buf.raw[:len(data)]


def cbc_encrypt(key: bytes, iv: bytes, data: bytes) -> bytes:
    n = (len(data) // 16 + 1) * 16
    out = ctypes.create_string_buffer(n)
    lib().cam_cbc_enc_c(bytes(key), bytes(iv), bytes(data), ctypes.c_size_t(len(data)), out)
    return out.raw


def cbc_decrypt(key: bytes, iv: bytes, data: bytes) -> bytes:
    out = ctypes.create_string_buffer(max(len(data), 1))
    n = lib().cam_cbc_dec_c(bytes(key), bytes(iv), bytes(data), ctypes.c_size_t(len(data)), out)
    if n < 0:
        raise ValueError("CBC: bad length or padding")
    return out.raw[:n]


def gmul(x: int, y: int) -> int:
    z, v = 0, x
    for i in range(128):
        if (y >> (127 - i)) & 1:
            z ^= v
        v = (v >> 1) ^ ((0xE1 << 120) if v & 1 else 0)
    return z


def ghash(h: int, c: bytes) -> int:
    """GHASH with the multiples of H by every byte value at every byte position taken from a table of 16 x 256 entries (built from 128 shifts of H)"""
    sh = [h]
    for _ in range(127):
        v = sh[-1]
        sh.append((v >> 1) ^ ((0xE1 << 120) if v & 1 else 0))
    tab = []
    for pos in range(16):
        row = [0] * 256
        for b in range(8):
            m = sh[8 * pos + b]
            bit = 0x80 >> b
            for v in range(256):
                if v & bit:
                    row[v] ^= m
        tab.append(row)

    def mul_h(x: int) -> int:
        z = 0
        for pos, byte in enumerate(x.to_bytes(16, "big")):
            z ^= tab[pos][byte]
        return z
    y = 0
    pad = bytes(c) + bytes(-len(c) % 16)
    for i in range(0, len(pad), 16):
        y = mul_h(y ^ int.from_bytes(pad[i:i + 16], "big"))
    return mul_h(y ^ (len(c) * 8))


def gcm_open(key: bytes, nonce: bytes, ct: bytes, tag: bytes) -> bytes:
    """GCM with a 96-bit nonce and no associated data over Camellia: H = E(K, 0), J0 = nonce || 1, data from counter 2, tag = GHASH ^ E(K, J0)"""
    sched = schedule(key)
    h = int.from_bytes(block(sched, bytes(16)), "big")
    ej0 = int.from_bytes(block(sched, bytes(nonce) + b"\0\0\0\1"), "big")
    if (ghash(h, ct) ^ ej0).to_bytes(16, "big") != bytes(tag):
        raise ValueError("GCM: authentication failure")
    return ctr(key, bytes(nonce) + b"\0\0\0\2", ct)


def gcm_stream_open(codec, k_master: bytes, data: bytes, header_type: bytes, header_body: bytes, phsf: bytes) -> bytes:
    """decrypt_reader's GCM arm (lib/src/entry/read.rs:105-140) with Camellia under it: the oracle's stream header, key confirmation, stream key and
    segment nonces; every segment's tag is verified"""
    hd = bytes(data[:75])
    salt, prefix, seg = hd[:32], hd[32:39], int.from_bytes(hd[39:43], "big")
    if hd[43:75] != codec.key_confirmation(k_master):
        raise ValueError("GCM STREAM: key confirmation failed")
    ks = codec.derive_stream_key(k_master, salt, prefix, seg, header_type, header_body, phsf)
    body, out, counter = bytes(data[75:]), bytearray(), 0
    while body:
        piece, body = body[:seg + 16], body[seg + 16:]
        out += gcm_open(ks, codec.segment_nonce(prefix, counter, not body), piece[:-16], piece[-16:])
        counter += 1
    return bytes(out)


def decrypt_stream(codec, item, password: bytes = b"password") -> bytes:
    """the compressed bytes of a Camellia entry or solid stream of oracle.pna_format's reading (ParsedEntry / ParsedSolid)"""
    assert item.encryption == ENC_CAMELLIA
    phsf = [d for ty, d in item.chunks if ty == b"PHSF"][0]
    km = codec.derive_key_from_phsf(phsf.decode(), password)
    if item.cipher_mode == 2:
        return gcm_stream_open(codec, km, item.data, item.chunks[0][0], item.chunks[0][1], phsf)
    iv, body = bytes(item.data[:16]), bytes(item.data[16:])
    return ctr(km, iv, body) if item.cipher_mode == 1 else cbc_decrypt(km, iv, body)
