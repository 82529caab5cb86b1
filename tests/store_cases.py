"""Entry lists and expected bytes for the stored create paths (PNA_ALGO_STORE on the archive entry points: k_store / k_store_fold).  A helper, not a test.

The expected bytes never come from the code under test: every record is the oracle's (oracle/pna_format.py write_normal_entry /
write_encrypted_file_entry over flatten_writer's cut), the cipher layer is the oracle's AES (oracle/codec.py: aes_ctr, aes_cbc_encrypt,
gcm_stream_encrypt, stream_header_bytes, derive_stream_key -- pinned by the reference's fixtures) with fixed IVs / salts; Camellia's is
tests/camellia_cases.py (csrc/camellia_core.h on the CPU, pinned by openssl's answers), its GCM seal written out here from that module's parts.
Records of entries that are not files are tests/tree_cases.py's."""
import functools

import numpy as np

import tree_cases as tc

FILE, DIR, SYMLINK, HARDLINK = tc.FILE, tc.DIR, tc.SYMLINK, tc.HARDLINK
MIB = 1 << 20
# k_frame_wave's 16 380-byte edge with and without the type, one piece, a piece edge, three-plus pieces per chunk
SIZES = [0, 1, 15, 16, 17, 63, 64, 65, 4095, 4096, 16376, 16377, 16380, 16381, 65539, MIB - 1, MIB, MIB + 1, 2 * MIB + 5, 3 * MIB + 17]
SMALL_SIZES = [s for s in SIZES if s <= 4096]
CAMELLIA_SIZES = [0, 15, 16, 17, 4095, 4096, 65539]          # (the CPU GHASH of this file is slow: the Camellia cases stay small)
# name lengths 1 .. 40 for SIZES, chosen so that the payloads' archive offsets take all 16 residues mod 16 (asserted by the tests from the expectation)
NAME_LENS = [40, 1, 2, 11, 10, 9, 11, 10, 9, 10, 9, 17, 16, 13, 11, 5, 9, 2, 2, 2]


@functools.lru_cache(maxsize=None)
def data_of(n: int, seed: int = 0) -> bytes:
    return np.random.RandomState(1000 + 7 * seed + n % 9973).bytes(n) if n else b""


def name_of(i: int, length: int) -> str:
    """a unique name of exactly `length` characters for entry i"""
    if length < 3:
        return ("abcdefghijklmnopqrstuvwxyz"[i] + "x")[:length]
    return ("s%02d" % i + "abcdefghijklmnopqrstuvwxyz0123456789-_ABCDEFGHIJ")[:length]


def entry_list(sizes=SIZES):
    """[(name, data)]: names of NAME_LENS' lengths (unique), data by size"""
    out = [(name_of(i, NAME_LENS[i % len(NAME_LENS)]), data_of(n, i)) for i, n in enumerate(sizes)]
    assert len({n for n, _d in out}) == len(out)
    return out


class CipherCfg:
    """key, PHSF string, mode ("ctr" | "cbc" | "gcm"), encryption (1 AES, 2 Camellia), per-entry IVs (16 bytes; GCM: salt(32) || nonce prefix(7)), GCM segment size"""

    def __init__(self, key, phsf, mode, n, encryption=1, gcm_segment_size=0):
        self.key, self.phsf, self.mode, self.encryption, self.gcm_segment_size = key, phsf, mode, encryption, gcm_segment_size
        self.per = 39 if mode == "gcm" else 16
        self.ivs = bytes((11 * i + 5 + 3 * self.per) & 255 for i in range(self.per * max(n, 1)))

    @property
    def mode_byte(self):
        return {"cbc": 0, "ctr": 1, "gcm": 2}[self.mode]

    @property
    def seg(self):
        return self.gcm_segment_size or (1 << 20)

    def iv(self, i):
        return self.ivs[self.per * i:self.per * (i + 1)]

    def product(self, pna):
        return pna.Cipher(self.key, self.phsf, {"cbc": pna.MODE_CBC, "ctr": pna.MODE_CTR, "gcm": pna.MODE_GCM}[self.mode], self.encryption, ivs=self.ivs,
                          gcm_segment_size=self.gcm_segment_size)


def _cam_gcm_seal(cc, key, nonce, data):
    sched = cc.schedule(key)
    h = int.from_bytes(cc.block(sched, bytes(16)), "big")
    ej0 = int.from_bytes(cc.block(sched, bytes(nonce) + b"\0\0\0\1"), "big")
    ct = cc.ctr(key, bytes(nonce) + b"\0\0\0\2", data)
    return ct, (cc.ghash(h, ct) ^ ej0).to_bytes(16, "big")


def gcm_stream_seal(codec, cfg, ks, prefix, data):
    """GcmEncryptWriter's segmenting (oracle/codec.py gcm_stream_encrypt) over either block cipher"""
    if cfg.encryption == 1:
        return codec.gcm_stream_encrypt(ks, prefix, cfg.seg, data)
    import camellia_cases as cc
    out, counter, pos = bytearray(), 0, 0
    while len(data) - pos > cfg.seg:
        c, t = _cam_gcm_seal(cc, ks, codec.segment_nonce(prefix, counter, False), data[pos:pos + cfg.seg])
        out += c + t; pos += cfg.seg; counter += 1
    c, t = _cam_gcm_seal(cc, ks, codec.segment_nonce(prefix, counter, True), data[pos:])
    return bytes(out + c + t)


def cipher_stream(pf, codec, cfg, i, name, data):
    """(data-stream prefix, ciphertext) of entry i: the IV and the encrypted bytes, or GCM STREAM's 75-byte header and its segments with their tags"""
    iv = cfg.iv(i)
    if cfg.mode == "gcm":
        salt, prefix = iv[:32], iv[32:]
        header = codec.stream_header_bytes(salt, prefix, cfg.seg, cfg.key)
        fhed = pf.entry_header_bytes(pf.KIND_FILE, 0, cfg.encryption, 2, pf.sanitize_name(name))
        ks = codec.derive_stream_key(cfg.key, salt, prefix, cfg.seg, b"FHED", fhed, cfg.phsf.encode())
        return header, gcm_stream_seal(codec, cfg, ks, prefix, data)
    if cfg.encryption == 1:
        return iv, (codec.aes_ctr(cfg.key, iv, data) if cfg.mode == "ctr" else codec.aes_cbc_encrypt(cfg.key, iv, data))
    import camellia_cases as cc
    return iv, (cc.ctr(cfg.key, iv, data) if cfg.mode == "ctr" else cc.cbc_encrypt(cfg.key, iv, data))


def _with_meta(pf, record, extra, facets):
    """FHED | fSIZ | rest -> FHED | extra | fSIZ | facets | rest (NormalEntry::write_chunks_to)"""
    if not extra and not facets:
        return record
    chunks = [(ty, d) for ty, d, _ in pf.read_chunks(record, 0)]
    out = bytearray(pf.write_chunk(*chunks[0])) + extra
    assert chunks[1][0] == b"fSIZ"
    out += pf.write_chunk(*chunks[1]) + facets
    for ty, d in chunks[2:]:
        out += pf.write_chunk(ty, d)
    return bytes(out)


def file_record(pf, codec, i, name, data, mcs=0, cfg=None, extra=b"", facets=b""):
    """(record, number of FDAT chunks that hold payload) of a stored file entry"""
    mx = mcs if mcs else pf.MAX_CHUNK_DATA_LENGTH
    if cfg is None:
        pieces = pf.flatten_writer([data], mx)
        rec = pf.write_normal_entry(pf.file_entry_header(0, pf.sanitize_name(name)), pieces, len(data), tc.blob_chunks(pf, extra), tc.blob_chunks(pf, facets))
        return rec, len(pieces)
    prefix, ct = cipher_stream(pf, codec, cfg, i, name, data)
    rec = pf.write_encrypted_file_entry(0, cfg.encryption, cfg.mode_byte, pf.sanitize_name(name), cfg.phsf, prefix, ct, len(data), mx)
    return _with_meta(pf, rec, extra, facets), len(pf.flatten_writer([ct], mx))


def expected_archive(pf, codec, entries, mcs=0, cfg=None, extra=None, facets=None, kinds=None, head=True, tail=True):
    """entries: [(name, data)]; kinds: None or [kind] (a link's data is its target).  Returns (bytes, [offset of every record] + [end of the records],
    payload FDAT chunks of the files, [archive offset of every file's first payload byte])"""
    out, offs, nchunks, pay = bytearray(pf.write_archive_header(0) if head else b""), [], 0, []
    for i, (name, data) in enumerate(entries):
        offs.append(len(out))
        ex, fa = (b"" if extra is None else extra[i]), (b"" if facets is None else facets[i])
        k = FILE if kinds is None else kinds[i]
        if k != FILE:
            out += tc.nonfile_record(pf, k, name, data, ex, fa, mcs)
            continue
        rec, nc = file_record(pf, codec, i, name, data, mcs, cfg, ex, fa)
        if nc:                                                    # the first payload chunk: the nc-th FDAT from the record's end
            fd = [(ty, pos - 12 - len(d)) for ty, d, pos in pf.read_chunks(rec, 0) if ty == b"FDAT"]
            pay.append(len(out) + fd[-nc][1] + 8)
        out += rec
        nchunks += nc
    offs.append(len(out))
    if tail:
        out += pf.finalize_archive()
    return bytes(out), offs, nchunks, pay


def read_back(pf, codec, archive, cfg, password_key=None):
    """the files' plain bytes of an archive through the oracle's reader (every chunk CRC checked), the cipher layer undone"""
    out = []
    for it in pf.read_archive(archive)[1]:
        if it.kind != FILE:
            out.append(None)
            continue
        assert it.compression == 0
        if it.encryption == 0:
            out.append(it.data)
        elif it.encryption == 1 and it.cipher_mode == 2:
            phsf = [d for ty, d in it.chunks if ty == b"PHSF"][0]
            out.append(codec.decrypt_payload_gcm(cfg.key, it.data, it.chunks[0][0], it.chunks[0][1], phsf))
        elif it.encryption == 1:
            out.append(codec.decrypt_payload(1, it.cipher_mode, cfg.key, it.data))
        else:
            import camellia_cases as cc
            phsf = [d for ty, d in it.chunks if ty == b"PHSF"][0]
            if it.cipher_mode == 2:
                out.append(cc.gcm_stream_open(codec, cfg.key, it.data, it.chunks[0][0], it.chunks[0][1], phsf))
            else:
                iv, body = bytes(it.data[:16]), bytes(it.data[16:])
                out.append(cc.ctr(cfg.key, iv, body) if it.cipher_mode == 1 else cc.cbc_decrypt(cfg.key, iv, body))
    return out


def tree_entries():
    """directories, a symbolic link, a hard link and stored files: (kind, name, bytes)"""
    return [
        (DIR, "t", b""),
        (FILE, "t/empty", b""),
        (FILE, "t/seventeen", data_of(17, 50)),
        (SYMLINK, "t/link", b"seventeen"),
        (FILE, "t/big.bin", data_of(MIB + 1, 51)),
        (DIR, "t/a", b""),
        (HARDLINK, "t/a/hard", b"t/big.bin"),
        (FILE, "t/a/page", data_of(4096, 52)),
        (SYMLINK, "t/a/far", (b"../" * 400)[:1100]),
        (DIR, "t/z", b""),
    ]


def meta_blobs(pf, n):
    extra = [pf.write_chunk(b"usRc", b"e%d" % i) for i in range(n)]
    facets = [pf.write_chunk(b"mTIM", (1700000000 + i).to_bytes(8, "big")) + pf.write_chunk(b"fPRM", b"\x01\xa4" + bytes([i & 255])) for i in range(n)]
    return extra, facets


def expected_solid(pf, codec, tree, mcs=0, cfg=None, extra=None, facets=None):
    """tree: [(kind, name, bytes)].  The stored solid archive: SHED(compression 0, ..) | [PHSF] | [SDAT(iv / stream header)] | SDAT* | SEND around the
    oracle's serialisation of the inner records, the stream cut into SDAT chunks of max_chunk_size bytes (GCM STREAM: one chunk per segment, its tag
    behind it).  Returns (archive, inner stream)."""
    inner = tc.inner_stream(pf, tree, extra, facets, mcs)
    mx = mcs if mcs else pf.MAX_CHUNK_DATA_LENGTH
    out = bytearray(pf.write_archive_header(0))
    if cfg is None:
        out += pf.write_chunk(b"SHED", pf.solid_header_bytes(0))
        pieces = [inner[o:o + mx] for o in range(0, len(inner), mx)]
    else:
        assert cfg.encryption == 1
        shed = pf.solid_header_bytes(0, cfg.encryption, cfg.mode_byte)
        out += pf.write_chunk(b"SHED", shed) + pf.write_chunk(b"PHSF", cfg.phsf.encode())
        iv = cfg.iv(0)
        if cfg.mode == "gcm":
            salt, prefix = iv[:32], iv[32:]
            out += pf.write_chunk(b"SDAT", codec.stream_header_bytes(salt, prefix, cfg.seg, cfg.key))
            ks = codec.derive_stream_key(cfg.key, salt, prefix, cfg.seg, b"SHED", shed, cfg.phsf.encode())
            body = codec.gcm_stream_encrypt(ks, prefix, cfg.seg, inner)
            pieces = [body[o:o + cfg.seg + 16] for o in range(0, len(body), cfg.seg + 16)]
        else:
            out += pf.write_chunk(b"SDAT", iv)
            ct = codec.aes_ctr(cfg.key, iv, inner)
            pieces = [ct[o:o + mx] for o in range(0, len(ct), mx)]
    for p in pieces:
        out += pf.write_chunk(b"SDAT", p)
    out += pf.write_chunk(b"SEND") + pf.finalize_archive()
    return bytes(out), inner


def solid_stream_back(pf, codec, archive, cfg):
    """the decoded inner stream of a stored solid archive through the oracle's reader"""
    (so,) = pf.read_archive(archive)[1]
    assert so.compression == 0
    if so.encryption == 0:
        return so.data
    phsf = [d for ty, d in so.chunks if ty == b"PHSF"][0]
    if so.cipher_mode == 2:
        return codec.decrypt_payload_gcm(cfg.key, so.data, so.chunks[0][0], so.chunks[0][1], phsf)
    return codec.decrypt_payload(1, so.cipher_mode, cfg.key, so.data)


def size_tree(sizes=SIZES):
    return [(FILE, n, d) for n, d in entry_list(sizes)]
