"""The password hashes of pna_create_archive_encrypted_ex (no GPU needed): Argon2id with the argon2 crate's defaults, written in the reference's PHC
form (lib/src/entry/options.rs:164, lib/src/hash.rs:6-33), and PBKDF2-SHA256 with a round count; the oracle derives the same key from the PHSF."""
import base64

import pytest


def test_argon2id_phsf_and_key(pna, codec):
    salt = bytes(range(16))
    key, phsf = pna.kdf_derive("argon2id", b"password", salt)
    assert phsf == "$argon2id$v=19$m=19456,t=2,p=1$" + base64.b64encode(salt).decode().rstrip("=")
    assert len(key) == 32 and codec.derive_key_from_phsf(phsf, b"password") == key
    assert key == pna.kdf_argon2(2, b"password", salt, 2, 19456, 1)
    assert pna.kdf_derive("argon2id", b"other", salt)[0] != key


def test_pbkdf2_phsf_and_key(pna, codec):
    salt = bytes(range(16))
    key, phsf = pna.kdf_derive("pbkdf2", b"password", salt, rounds=1000)
    assert (key, phsf) == pna.kdf_pbkdf2_sha256(b"password", salt, 1000)
    assert phsf.startswith("$pbkdf2-sha256$i=1000,l=32$") and codec.derive_key_from_phsf(phsf, b"password") == key


def test_encrypted_ex_entry_point_without_a_device(pna):
    import ctypes
    L = pna.load_library()
    for sym in ("pna_create_archive_encrypted_ex", "pna_kdf_derive", "pna_gpu_create_solid_archive_enc_host"):
        assert sym in pna.EXPORTS and getattr(L, sym)
    cb = pna.SINK_FN(lambda u, b, k: 0)
    rc = L.pna_create_archive_encrypted_ex(None, pna.ALGO_ZSTD, 3, 1, 0, None, None, None, b"pw", 2, pna.MODE_GCM, 0, 0, cb, None)
    assert rc == pna.E_NODEVICE
    key = ctypes.create_string_buffer(32); phsf = ctypes.create_string_buffer(256)
    assert L.pna_kdf_derive(7, b"pw", 2, b"salt", 4, 0, key, phsf, 256) == pna.E_INVAL        # an unknown KDF
    assert L.pna_kdf_derive(0, b"pw", 2, b"salt", 4, 0, key, phsf, 8) == pna.E_DSTSIZE        # no room for the PHSF
    with pytest.raises(ValueError):
        pna.kdf_derive("scrypt", b"pw", b"salt")
    with pytest.raises(ValueError):
        pna.create_archive_encrypted(None, [], [], b"pw", solid=True, kdf="scrypt")
