"""`pna verify` on the device (pna_gpu_verify_archive_host): one verdict per entry, the walk going on after damage -- the reference's verify.rs and its
CLI tests (verify_with_stream_corruption, verify_with_fast_on_stream_corruption, ...) as far as this library's driver takes them."""
import os
import struct
import subprocess
import sys
import zlib

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
PW = b"password"
PNA_E_INVAL = -2


@pytest.fixture(scope="module")
def ctx(pna):
    import torch  # noqa: F401
    c = pna.Context(0)
    yield c
    c.close()


def chunks(buf):
    """(offset of the length field, type, data offset, data length) of every chunk behind the signature"""
    pos, out = 8, []
    while pos + 12 <= len(buf):
        n = struct.unpack(">I", buf[pos:pos + 4])[0]
        out.append((pos, buf[pos + 4:pos + 8], pos + 8, n))
        pos += 12 + n
    return out


def entry_chunks(buf):
    """per entry (FHED .. FEND): its chunks"""
    ents, cur = [], None
    for ch in chunks(buf):
        if ch[1] == b"FHED":
            cur = [ch]
        elif cur is not None:
            cur.append(ch)
            if ch[1] == b"FEND":
                ents.append(cur); cur = None
    return ents


def fix_crc(buf, ch):
    pos, ty, d, n = ch
    buf[d + n:d + n + 4] = struct.pack(">I", zlib.crc32(bytes(buf[pos + 4:d + n])) & 0xFFFFFFFF)


def payload(buf, ent):
    return b"".join(bytes(buf[d:d + n]) for _, ty, d, n in ent if ty == b"FDAT")


def statuses(recs):
    return [r[2] for r in recs]


def data(i, n=20000):
    from oracle import codec
    return codec.corpus_file(i % 3, i, n)


def make(pna, ctx, n, mode=None, algo=None, size=20000):
    algo = pna.ALGO_ZSTD if algo is None else algo
    names = [f"d/f{i}" for i in range(n)]
    ents = [data(i, size) for i in range(n)]
    if mode is None:
        return pna.create_archive(ctx, names, ents, algo=algo), names, ents
    return pna.create_archive_encrypted(ctx, names, ents, PW, algo=algo, mode=mode, rounds=1000), names, ents


def goldens():
    return sorted(f for f in os.listdir(GOLDEN) if f.endswith(".pna") and not f.startswith("multipart"))


@pytest.mark.parametrize("fname", goldens())
def test_golden_fixtures(pna, ctx, fname):
    arc = open(os.path.join(GOLDEN, fname), "rb").read()
    want = [(n, len(d)) for n, _k, d in pna.extract_archive(ctx, arc, PW)]
    recs, s = pna.verify_archive(ctx, arc, PW)
    assert s["rc"] == 0 and s["failed"] == 0 and s["broken"] == 0
    assert all(r[2] == pna.VERIFY_OK for r in recs), recs
    assert [(r[0], r[4]) for r in recs] == want
    recs, s = pna.verify_archive(ctx, arc)                     # no password: encrypted entries / blocks are skipped, nothing fails
    assert s["failed"] == 0 and s["rc"] == 0
    if "aes" in fname:
        assert s["skipped"] >= 1 and all(r[2] == pna.VERIFY_SKIPPED for r in recs)
    else:
        assert all(r[2] == pna.VERIFY_OK for r in recs)
    recs, s = pna.verify_archive(ctx, arc, fast=True)
    assert s["failed"] == 0 and all(r[2] == pna.VERIFY_OK for r in recs) and s["total"] == len(recs)
    assert len(recs) >= 1 or fname == "empty.pna"


def test_golden_multipart(pna, ctx):
    parts = [open(os.path.join(GOLDEN, f"multipart.part{k}.pna"), "rb").read() for k in (1, 2)]
    want = [(n, len(d)) for n, _k, d in pna.extract_archive(ctx, pna.join_parts(parts))]
    for fast in (False, True):
        recs, s = pna.verify_archive(ctx, parts, fast=fast)
        assert s["rc"] == 0 and s["failed"] == 0 and all(r[2] == pna.VERIFY_OK for r in recs)
        assert [r[0] for r in recs] == [n for n, _ in want]
        if not fast:
            assert [r[4] for r in recs] == [l for _, l in want]
    recs, s = pna.verify_archive(ctx, parts[:1])             # the second part missing: the structure breaks off
    assert s["rc"] == PNA_E_INVAL and s["broken"] == 1


@pytest.mark.parametrize("kind", ["zstd", "deflate", "ctr", "cbc", "gcm"])
def test_crc_damage(pna, ctx, kind):
    mode = {"ctr": pna.MODE_CTR, "cbc": pna.MODE_CBC, "gcm": pna.MODE_GCM}.get(kind)
    arc, names, _ = make(pna, ctx, 64, mode, pna.ALGO_DEFLATE if kind == "deflate" else None)
    buf = bytearray(arc)
    ents = entry_chunks(buf)
    bad = {0, 31, 32, 63}
    for i in bad:
        _, ty, d, n = [c for c in ents[i] if c[1] == b"FDAT"][0]
        buf[d + n // 2] ^= 0x40
    for fast in (False, True):
        recs, s = pna.verify_archive(ctx, bytes(buf), PW, fast=fast)
        assert s["rc"] == 0 and len(recs) == 64
        assert [i for i, r in enumerate(recs) if r[2] != pna.VERIFY_OK] == sorted(bad)
        assert all(recs[i][2] == pna.VERIFY_BAD_CRC for i in bad)
        assert s["failed"] == 4 and s["ok"] == 60
        assert [r[0] for r in recs] == names


def _corrupt_stream(buf, ent, algo, raw_len, reject=None):
    """a stream corruption the independent decoder rejects, the chunk CRC repaired.  deflate: a byte in the middle and the Adler-32; zstd: a byte inside
    the compressed blocks (magic and frame header left intact, so the frame is placed and executed), the first position from the middle on that the
    oracle's decoder (or `reject`) refuses"""
    fd = [c for c in ent if c[1] == b"FDAT"]
    _, ty, d, n = fd[0]
    if algo == "deflate":
        buf[d + n // 2] ^= 0xFF
        _, ty2, d2, n2 = fd[-1]
        buf[d2 + n2 - 1] ^= 0x5A                                # the Adler-32 as well: no decoder can accept it
    else:
        from oracle import codec
        assert len(fd) == 1
        reject = reject or (lambda z: codec.zstd_decompress(z, raw_len))
        for k in list(range(n // 2, n - 8)) + list(range(32, n // 2)):
            buf[d + k] ^= 0xFF
            try:
                out = reject(bytes(buf[d:d + n]))
            except (ValueError, RuntimeError):
                break
            buf[d + k] ^= 0xFF
        else:
            raise AssertionError("no rejected corruption found")
    for c in fd:
        fix_crc(buf, c)


@pytest.mark.parametrize("algo", ["zstd", "deflate"])
def test_stream_damage(pna, ctx, codec, algo):
    arc, names, ents = make(pna, ctx, 16, None, pna.ALGO_DEFLATE if algo == "deflate" else None)
    buf = bytearray(arc)
    ech = entry_chunks(buf)
    b = 4                                                       # (a text entry: compressed blocks, not raw ones)
    _corrupt_stream(buf, ech[b], algo, len(ents[b]))
    p = payload(buf, ech[b])
    with pytest.raises(Exception):
        if algo == "deflate":
            zlib.decompress(p)
        else:
            codec.zstd_decompress(p, len(ents[b]))
    recs, s = pna.verify_archive(ctx, bytes(buf))
    assert s["rc"] == 0 and [i for i, r in enumerate(recs) if r[2] != pna.VERIFY_OK] == [b] and recs[b][2] == pna.VERIFY_BAD_STREAM
    assert [r[4] for i, r in enumerate(recs) if i != b] == [len(e) for i, e in enumerate(ents) if i != b]
    recs, s = pna.verify_archive(ctx, bytes(buf), fast=True)
    assert all(r[2] == pna.VERIFY_OK for r in recs) and s["failed"] == 0


def test_stream_damage_large_foreign(pna, ctx, codec, pf):
    """one stdlib-zlib stream and one libzstd frame of 256 MiB and more between good entries: the chunked inflate and the parallel zstd paths"""
    big = (data(1, 1 << 20) * 300)[: 300 << 20]
    z = zlib.compress(big, 1)
    zs = codec.libzstd_compress_checksum(big, 1)                # (Content_Checksum: the XXH64 check runs on the executed output)
    small = [data(i) for i in range(4)]
    body = pf.write_normal_entry(pf.file_entry_header(1, "a"), [zlib.compress(small[0])], len(small[0]))
    body += pf.write_normal_entry(pf.file_entry_header(1, "bigz"), [z], len(big))
    body += pf.write_normal_entry(pf.file_entry_header(1, "b"), [zlib.compress(small[1])], len(small[1]))
    body += pf.write_normal_entry(pf.file_entry_header(2, "bigzs"), [zs], len(big))
    body += pf.write_normal_entry(pf.file_entry_header(1, "c"), [zlib.compress(small[2])], len(small[2]))
    arc = pf.write_archive_header() + body + pf.finalize_archive()
    recs, s = pna.verify_archive(ctx, arc)
    assert s["failed"] == 0 and [r[4] for r in recs] == [len(small[0]), len(big), len(small[1]), len(big), len(small[2])]
    buf = bytearray(arc)
    ech = entry_chunks(buf)
    _corrupt_stream(buf, ech[1], "deflate", len(big))
    _corrupt_stream(buf, ech[3], "zstd", len(big), reject=lambda z: codec.libzstd_decompress_stream(z, len(big)))
    recs, s = pna.verify_archive(ctx, bytes(buf))
    assert statuses(recs) == [0, pna.VERIFY_BAD_STREAM, 0, pna.VERIFY_BAD_STREAM, 0] and s["failed"] == 2


def test_authentication(pna, ctx):
    for mode in (pna.MODE_GCM, pna.MODE_CBC, pna.MODE_CTR):
        arc, _, _ = make(pna, ctx, 8, mode)
        recs, s = pna.verify_archive(ctx, arc, b"wrong password")
        assert s["failed"] == 8 and s["rc"] == 0
        for r in recs:
            if mode == pna.MODE_GCM:
                assert r[2] == pna.VERIFY_BAD_AUTH and not (r[3] & pna.VERIFY_UNAUTHENTICATED)
            elif mode == pna.MODE_CBC:
                assert r[2] in (pna.VERIFY_BAD_DECRYPT, pna.VERIFY_BAD_STREAM) and r[3] & pna.VERIFY_UNAUTHENTICATED
            else:
                assert r[2] == pna.VERIFY_BAD_STREAM and r[3] & pna.VERIFY_UNAUTHENTICATED
        assert s["unauthenticated_failure"] == (0 if mode == pna.MODE_GCM else 1)
    arc, _, _ = make(pna, ctx, 8, pna.MODE_GCM)
    buf = bytearray(arc)
    ent = entry_chunks(buf)[3]
    fd = max((c for c in ent if c[1] == b"FDAT"), key=lambda c: c[3])     # (the 75-byte stream header is a chunk of its own)
    _, _, d, n = fd
    buf[d + n // 2] ^= 0x01                                     # a ciphertext bit
    fix_crc(buf, fd)
    recs, s = pna.verify_archive(ctx, bytes(buf), PW)
    assert [r[2] for r in recs] == [0, 0, 0, pna.VERIFY_BAD_AUTH, 0, 0, 0, 0]


def test_headers_and_structure(pna, ctx):
    arc, names, _ = make(pna, ctx, 6)
    buf = bytearray(arc)
    pos, ty, d, n = entry_chunks(buf)[2][0]
    buf[d + 7] ^= 0x20                                          # a byte of the FHED name, its CRC left alone
    recs, s = pna.verify_archive(ctx, bytes(buf))
    assert s["rc"] == 0 and len(recs) == 6
    assert recs[2][0] is None and recs[2][1] == pna.VERIFY_KIND_BROKEN and recs[2][2] == pna.VERIFY_BAD_CRC
    assert [r[2] for i, r in enumerate(recs) if i != 2] == [0] * 5 and [r[0] for i, r in enumerate(recs) if i != 2] == names[:2] + names[3:]

    sol = bytearray(open(os.path.join(GOLDEN, "solid_zstd.pna"), "rb").read())
    sd = [c for c in chunks(sol) if c[1] == b"SDAT"][0]
    sol[sd[2] + sd[3] // 2] ^= 0x10
    for fast in (False, True):
        recs, s = pna.verify_archive(ctx, bytes(sol), fast=fast)
        assert recs == [r for r in recs if r[1] == pna.VERIFY_KIND_SOLID] and len(recs) == 1 and recs[0][2] == pna.VERIFY_BAD_CRC

    ech = entry_chunks(bytearray(arc))
    cut = ech[4][2][0] + 5                                      # inside entry 4's data
    recs, s = pna.verify_archive(ctx, arc[:cut])
    assert s["rc"] == PNA_E_INVAL and s["broken"] == 1
    assert [r[0] for r in recs] == names[:4] and all(r[2] == 0 for r in recs)


@pytest.mark.parametrize("delta", [1234, -1234])
@pytest.mark.parametrize("algo", ["zstd", "deflate"])
def test_size_hint(pna, ctx, algo, delta):
    arc, names, ents = make(pna, ctx, 5, None, pna.ALGO_DEFLATE if algo == "deflate" else None)
    buf = bytearray(arc)
    fs = [c for c in entry_chunks(buf)[1] if c[1] == b"fSIZ"][0]
    _, _, d, n = fs
    buf[d:d + n] = (len(ents[1]) + delta).to_bytes(n, "big")
    fix_crc(buf, fs)
    recs, s = pna.verify_archive(ctx, bytes(buf))
    assert s["failed"] == 0
    assert recs[1][2] == pna.VERIFY_OK and recs[1][3] & pna.VERIFY_SIZE_HINT and recs[1][4] == len(ents[1])
    assert all(r[3] == 0 for i, r in enumerate(recs) if i != 1)


@pytest.mark.parametrize("algo", ["zstd", "deflate"])
def test_isolation_at_scale(pna, ctx, algo):
    n = 4096
    names = [f"f{i}" for i in range(n)]
    from oracle import codec
    base = [codec.corpus_file(k % 2, k, 256 << 10) for k in range(64)]      # text kinds: every stream has compressed blocks to damage
    ents = [base[i % 64] for i in range(n)]
    arc = pna.create_archive(ctx, names, ents, algo=pna.ALGO_DEFLATE if algo == "deflate" else pna.ALGO_ZSTD)
    buf = bytearray(arc)
    ech = entry_chunks(buf)
    bad = list(range(0, n, 7))
    for i in bad:
        _corrupt_stream(buf, ech[i], algo, len(ents[i]))
    recs, s = pna.verify_archive(ctx, bytes(buf))
    assert s["rc"] == 0 and len(recs) == n
    assert [i for i, r in enumerate(recs) if r[2] != pna.VERIFY_OK] == bad
    assert all(recs[i][2] == pna.VERIFY_BAD_STREAM for i in bad)


CHILD = r"""
import resource, sys, time
sys.path.insert(0, sys.argv[1])
import importlib, torch
pna = importlib.import_module("portable-network-archive_amd")
arc = open(sys.argv[2], "rb").read()
with pna.Context(0) as ctx:
    pna.verify_archive(ctx, arc[:0] + open(sys.argv[3], "rb").read())        # warm the context on a small archive
    r0 = resource.getrusage(resource.RUSAGE_SELF).ru_maxrss
    recs, s = pna.verify_archive(ctx, arc)
    r1 = resource.getrusage(resource.RUSAGE_SELF).ru_maxrss
    assert s["failed"] == 0 and s["rc"] == 0, s
    n = [0]
    def cb(_u, i, name, kind, d, l):
        n[0] += l
        return 0
    rc = ctx._L.pna_gpu_extract_archive_host(ctx._h, arc, len(arc), None, 0, pna.ENTRY_FN(cb), None)
    r2 = resource.getrusage(resource.RUSAGE_SELF).ru_maxrss
    assert rc == 0
print("RSS_KIB", r1 - r0, r2 - r1, sum(r[4] for r in recs), n[0])
"""


def test_no_decoded_bytes_on_host(pna, ctx, tmp_path):
    n = 1024
    base = [data(k, 4 << 20) for k in range(16)]
    ents = [base[i % 16] for i in range(n)]                     # 4 GiB decoded
    arc = pna.create_archive(ctx, [f"f{i}" for i in range(n)], ents)
    del ents, base
    p = tmp_path / "big.pna"; p.write_bytes(arc)
    small = tmp_path / "small.pna"; small.write_bytes(make(pna, ctx, 4)[0])
    del arc
    out = subprocess.run(["timeout", "-k", "10", "300", sys.executable, "-c", CHILD, ROOT, str(p), str(small)], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-3000:]
    line = [l for l in out.stdout.splitlines() if l.startswith("RSS_KIB")][0].split()
    grow_verify, grow_extract, vbytes, xbytes = (int(v) for v in line[1:])
    assert vbytes == xbytes == 4 << 30
    assert grow_verify < (1 << 20), grow_verify                   # KiB: under 1 GiB
    assert grow_extract >= (1 << 20), grow_extract               # extract: its windows of decoded bytes in host memory


def _splice(*archives):
    """one archive from the entries of several (their chunks between AHED and AEND)"""
    return archives[0][:28] + b"".join(a[28:-12] for a in archives) + archives[0][-12:]


@pytest.mark.parametrize("closing", [b"FEND", b"SEND"])
def test_damaged_end_chunk_fails_only_its_entry(pna, ctx, closing):
    """a flipped type byte of an FEND / SEND (its CRC then fails): that entry or block fails, the ones behind it do not"""
    a1, n1, _ = make(pna, ctx, 4)
    sol = pna.create_archive(ctx, ["s0", "s1", "s2"], [data(i) for i in range(3)], solid=True)
    a2, n2, _ = make(pna, ctx, 4)
    buf = bytearray(_splice(a1, sol, a2))
    ends = [c for c in chunks(buf) if c[1] == closing]
    pos = ends[2 if closing == b"FEND" else 0][0]              # entry 2's FEND, or the solid block's SEND
    buf[pos + 7] ^= 0x01
    for fast in (False, True):
        recs, s = pna.verify_archive(ctx, bytes(buf), fast=fast)
        assert s["rc"] == 0 and s["broken"] == 0 and s["failed"] == 1
        bad = [i for i, r in enumerate(recs) if r[2] != pna.VERIFY_OK]
        assert len(bad) == 1 and recs[bad[0]][2] == pna.VERIFY_BAD_CRC
        if closing == b"FEND":
            assert bad == [2] and recs[2][0] == n1[2]
        else:
            assert recs[bad[0]][1] == pna.VERIFY_KIND_SOLID and bad == [4]
        assert [r[0] for r in recs[bad[0] + 1:]][-4:] == n2


def test_many_cbc_key_groups(pna, ctx, codec, pf):
    """1 500 CBC entries, each with a PHSF of its own (the reference draws a salt per entry): one key group per entry in one window, one bad padding"""
    n, bad = 1500, 1100
    body = b""
    for i in range(n):
        raw = data(i, 3000)
        key, phsf = pna.kdf_pbkdf2_sha256(PW, i.to_bytes(16, "little"), 1)
        iv = bytes([i & 0xFF]) * 16
        z = zlib.compress(raw)
        if i == bad:                                            # a PKCS#7 padding no decryptor accepts: the last plaintext byte 0
            plain = z + bytes(16 - len(z) % 16)
            ct = codec.aes_cbc_encrypt(key, iv, plain)[:len(plain)]
        else:
            ct = codec.aes_cbc_encrypt(key, iv, z)
        body += pf.write_encrypted_file_entry(pna.ALGO_DEFLATE, pna.ENC_AES, pna.MODE_CBC, f"c{i}", phsf, iv, ct, len(raw))
    arc = pf.write_archive_header() + body + pf.finalize_archive()
    recs, s = pna.verify_archive(ctx, arc, PW)
    assert s["rc"] == 0 and len(recs) == n and s["failed"] == 1
    assert [i for i, r in enumerate(recs) if r[2] != pna.VERIFY_OK] == [bad]
    assert recs[bad][2] == pna.VERIFY_BAD_DECRYPT and recs[bad][3] & pna.VERIFY_UNAUTHENTICATED
    assert all(r[4] == 3000 for i, r in enumerate(recs) if i != bad)


def test_argument_checks_with_a_context(pna, ctx):
    """the argument checks behind the null-context one (the CPU file can only pass a null context: no device there)"""
    import ctypes
    L = ctx._L
    arc = make(pna, ctx, 2)[0]
    parts = (ctypes.c_char_p * 1)(arc)
    lens = (ctypes.c_size_t * 1)(len(arc))
    cb = pna.VERIFY_FN(lambda *a: 0)
    f = L.pna_gpu_verify_archive_host
    assert f(ctx._h, parts, lens, 1, None, 0, 0, cb, None, None) == 0
    assert f(ctx._h, None, lens, 1, None, 0, 0, cb, None, None) == PNA_E_INVAL                       # null parts
    assert f(ctx._h, parts, None, 1, None, 0, 0, cb, None, None) == PNA_E_INVAL                       # null lengths
    assert f(ctx._h, parts, lens, 0, None, 0, 0, cb, None, None) == PNA_E_INVAL                       # no part
    assert f(ctx._h, parts, lens, 1, None, 0, 0, ctypes.cast(None, pna.VERIFY_FN), None, None) == PNA_E_INVAL   # null cb
    assert f(ctx._h, parts, lens, 1, None, 5, 0, cb, None, None) == PNA_E_INVAL                       # a length without a password
    assert f(ctx._h, parts, lens, 1, None, 0, 4, cb, None, None) == PNA_E_INVAL                       # an unknown flag
