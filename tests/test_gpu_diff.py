"""`pna diff` on the device (pna_gpu_diff_archive_host, k_diff): the archive's entries against the host's files -- which differ, and from which byte.
Every expectation is computed here from the plain bytes (numpy first difference); archives whose layout matters are written with oracle/pna_format.py."""
import ctypes
import os
import struct
import subprocess
import sys
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
PW = b"password"
PNA_E_INVAL, PNA_E_SINK = -2, -6
MIB = 1 << 20


@pytest.fixture(scope="module")
def ctx(pna):
    import torch  # noqa: F401
    c = pna.Context(0)
    yield c
    c.close()


def data(i, n=20000):
    from oracle import codec
    return codec.corpus_file(i % 3, i, n)


def first_difference(a, b):
    """offset of the first differing byte; the shorter length where one is a strict prefix of the other; None when equal"""
    n = min(len(a), len(b))
    if n == 0:
        return None if len(a) == len(b) else 0
    ne = np.flatnonzero(np.frombuffer(a, np.uint8, n) != np.frombuffer(b, np.uint8, n))
    if len(ne):
        return int(ne[0])
    return None if len(a) == len(b) else n


def flip(buf, *offs):
    b = bytearray(buf)
    for o in offs:
        b[o] ^= 0x5A
    return bytes(b)


def chunks(buf):
    pos, out = 8, []
    while pos + 12 <= len(buf):
        n = struct.unpack(">I", buf[pos:pos + 4])[0]
        out.append((pos, bytes(buf[pos + 4:pos + 8]), pos + 8, n))
        pos += 12 + n
    return out


def entry_chunks(buf):
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


def golden_files():
    out = {}
    for d, _, fs in os.walk(os.path.join(GOLDEN, "raw")):
        for f in fs:
            p = os.path.join(d, f)
            out[os.path.relpath(p, GOLDEN).replace(os.sep, "/")] = open(p, "rb").read()
    return out


FIXTURES = ["zstd.pna", "deflate.pna", "zstd_keep_all.pna", "zstd_aes_ctr.pna", "zstd_aes_cbc.pna", "zstd_aes_gcm.pna", "solid_zstd.pna", "solid_deflate.pna",
            "solid_zstd_aes_ctr.pna", "solid_zstd_aes_cbc.pna", "solid_zstd_aes_gcm.pna"]


@pytest.mark.parametrize("fname", FIXTURES)
def test_golden_fixtures(pna, ctx, fname):
    arc = open(os.path.join(GOLDEN, fname), "rb").read()
    files = golden_files()
    recs, s = pna.diff_archive(ctx, arc, files, PW)
    assert s["rc"] == 0 and s["damaged"] == 0 and s["skipped"] == 0 and len(recs) >= 5
    for r in recs:
        assert r.status == (pna.DIFF_SAME if r.name in files else pna.DIFF_MISSING), r
        assert r.first_diff is None and (r.status != pna.DIFF_SAME or r.size == len(files[r.name]))
    assert {r.name for r in recs} >= {"raw/images/icon.png", "raw/text.txt", "raw/empty.txt"}
    assert s["same"] == sum(r.status == pna.DIFF_SAME for r in recs) and s["differ"] == len(recs) - s["same"] and s["total"] == len(recs)
    at = len(files["raw/images/icon.png"]) * 2 // 3
    changed = dict(files); changed["raw/images/icon.png"] = flip(files["raw/images/icon.png"], at)
    recs2, s2 = pna.diff_archive(ctx, arc, changed, PW)
    assert [r for r in recs2 if r.status == pna.DIFF_CONTENTS_DIFFER] == [r for r in recs2 if r.name == "raw/images/icon.png"]
    assert [r.first_diff for r in recs2 if r.name == "raw/images/icon.png"] == [at]
    assert [(r.name, r.status) for r in recs2 if r.name != "raw/images/icon.png"] == [(r.name, r.status) for r in recs if r.name != "raw/images/icon.png"]


def test_golden_multipart(pna, ctx, pf, codec):
    """the split fixture, read part by part in place: its entries are no files of tests/golden/raw (MISSING); against their own content, read by the oracle, SAME"""
    parts = [open(os.path.join(GOLDEN, f"multipart.part{k}.pna"), "rb").read() for k in (1, 2)]
    files = golden_files()
    recs, s = pna.diff_archive(ctx, parts, files)
    assert s["rc"] == 0 and len(recs) >= 1 and all(r.status == (pna.DIFF_SAME if r.name in files else pna.DIFF_MISSING) for r in recs)
    joined = pf.write_archive_header() + b"".join(pf.write_chunk(ty, d) for ty, d in pf.join_parts(parts)) + pf.finalize_archive()
    own = {pf.sanitize_name(e.name): codec.decode_payload(e.compression, e.data, 1 << 26) for e in pf.read_archive(joined)[1]}
    assert len(own) == len(recs) and sum(len(v) for v in own.values()) > len(parts[0])      # (the entry spans the parts)
    recs, s = pna.diff_archive(ctx, parts, own)
    assert [(r.name, r.status, r.size) for r in recs] == [(n, pna.DIFF_SAME, len(d)) for n, d in own.items()]
    name, d = max(own.items(), key=lambda kv: len(kv[1]))
    recs, s = pna.diff_archive(ctx, parts, {**own, name: flip(d, len(d) - 2)})
    assert [(r.status, r.first_diff) for r in recs if r.name == name] == [(pna.DIFF_CONTENTS_DIFFER, len(d) - 2)] and s["differ"] == 1
    recs, s = pna.diff_archive(ctx, parts[:1], own)                  # the second part missing: the structure breaks off
    assert s["rc"] == PNA_E_INVAL and s["broken"] == 1


def one_entry_cases(n, slot):
    tile = 16384                                                     # pna.DIFF_TILE
    return sorted({0, 1, 15, 16, 17, tile - 1, tile, tile + 1, slot - 1, slot, slot + 1, 2 * slot - 1, 2 * slot, 2 * slot + 1, n - 1})


@pytest.mark.parametrize("algo", ["zstd", "deflate", "store"])
def test_first_diff_exact(pna, ctx, pf, algo):
    assert pna.DIFF_TILE == 16384
    ctx.set_option("diff_slot_mib", 1)
    try:
        n = 2 * MIB + 12345
        raw = (data(1, 1 << 18) * 9)[:n]
        a = {"zstd": pna.ALGO_ZSTD, "deflate": pna.ALGO_DEFLATE, "store": 0}[algo]
        arc = pna.create_archive(ctx, ["d/one"], [raw], algo=a) if a else \
            pf.write_archive_header() + pf.write_normal_entry(pf.file_entry_header(0, "d/one"), [raw[:MIB + 3], raw[MIB + 3:]], len(raw)) + pf.finalize_archive()
        recs, s = pna.diff_archive(ctx, arc, {"d/one": raw})
        assert [(r.name, r.status, r.first_diff, r.size) for r in recs] == [("d/one", pna.DIFF_SAME, None, n)] and s["same"] == 1
        for off in one_entry_cases(n, MIB):
            other = flip(raw, off)
            recs, _ = pna.diff_archive(ctx, arc, {"d/one": other})
            assert first_difference(raw, other) == off
            assert (recs[0].status, recs[0].first_diff) == (pna.DIFF_CONTENTS_DIFFER, off), off
        for a_, b_ in ((5, 70000), (70000, MIB + 9), (16383, 16384), (MIB - 1, n - 1)):           # two differences: the first wins
            other = flip(raw, a_, b_)
            recs, _ = pna.diff_archive(ctx, arc, {"d/one": other})
            assert first_difference(raw, other) == a_
            assert (recs[0].status, recs[0].first_diff) == (pna.DIFF_CONTENTS_DIFFER, a_)
    finally:
        ctx.set_option("diff_slot_mib", 256)


@pytest.mark.parametrize("algo", ["zstd", "deflate", "store"])
def test_length_differences(pna, ctx, pf, codec, algo):
    """a file that is a strict prefix / extension of the entry: without fSIZ CONTENTS_DIFFER at the shorter length; with fSIZ SIZE_DIFFERS and no decode"""
    raw = data(4, 300000)
    comp = {"zstd": 2, "deflate": 1, "store": 0}[algo]
    pay = {"zstd": lambda: codec.model_compress(raw, codec.params_for_level(3)), "deflate": lambda: zlib.compress(raw), "store": lambda: raw}[algo]()
    for fsiz in (None, len(raw)):
        arc = pf.write_archive_header() + pf.write_normal_entry(pf.file_entry_header(comp, "x"), [pay], fsiz) + pf.finalize_archive()
        recs, _ = pna.diff_archive(ctx, arc, {"x": raw})
        assert (recs[0].status, recs[0].first_diff, recs[0].size) == (pna.DIFF_SAME, None, len(raw))
        streams_same = pna.diff_stats(ctx)[0]
        assert streams_same == (0 if algo == "store" else 1)
        for other in (raw[:-1], raw[:12345], raw + b"\0", raw + raw[:70000], b""):
            recs, s = pna.diff_archive(ctx, arc, {"x": other})
            if fsiz is None:
                assert (recs[0].status, recs[0].first_diff) == (pna.DIFF_CONTENTS_DIFFER, first_difference(raw, other)), len(other)
                assert first_difference(raw, other) == min(len(raw), len(other))
            else:
                assert (recs[0].status, recs[0].first_diff, recs[0].verify_status) == (pna.DIFF_SIZE_DIFFERS, None, 0)
                assert pna.diff_stats(ctx)[0] == 0 and pna.diff_stats(ctx)[1] == 0          # no stream decoded, no byte compared
            assert s["differ"] == 1
        recs, _ = pna.diff_archive(ctx, arc, {"x": flip(raw, 77)[:-5] if fsiz is None else flip(raw, 77)})
        assert (recs[0].status, recs[0].first_diff) == (pna.DIFF_CONTENTS_DIFFER, 77)


def test_stream_entry_without_fsiz(pna, ctx, pf):
    """an entry written while its data arrived (pna_gpu_stream_entry_*: no fSIZ, many FDAT chunks)"""
    raw = data(2, 500000)
    out = bytearray(pf.write_archive_header())
    L = ctx._L
    sink = pna.SINK_FN(lambda _u, buf, k: (out.extend(ctypes.string_at(buf, k)), 0)[1])
    w = ctypes.c_void_p()
    assert L.pna_gpu_stream_entry_begin(ctx._h, pna.ALGO_ZSTD, 3, b"s/entry", None, 0, 0, sink, None, ctypes.byref(w)) == 0
    assert L.pna_gpu_stream_entry_write(w, raw, len(raw)) == 0 and L.pna_gpu_stream_entry_finish(w) == 0
    arc = bytes(out) + pf.finalize_archive()
    assert pf.read_archive(arc)[1][0].raw_file_size is None
    for other in (raw, raw[:-7], raw + b"tail", flip(raw, 400001)):
        recs, _ = pna.diff_archive(ctx, arc, {"s/entry": other})
        want = first_difference(raw, other)
        assert (recs[0].status, recs[0].first_diff) == ((pna.DIFF_SAME, None) if want is None else (pna.DIFF_CONTENTS_DIFFER, want))


def solid_archive(pf, names, ents, comp=1, fsiz=True, split=None):
    """a solid block of stored inner entries, written by the oracle's writer; returns the archive and every inner entry's data offsets in the stream"""
    plain, starts = bytearray(), []
    for nm, e in zip(names, ents):
        pieces = [e] if not split or len(e) < 2 else [e[:len(e) // split], e[len(e) // split:]]
        ent = pf.write_normal_entry(pf.file_entry_header(0, nm), pieces, len(e) if fsiz else None)
        pos, offs = 0, []
        while pos < len(ent):
            n = struct.unpack(">I", ent[pos:pos + 4])[0]
            if ent[pos + 4:pos + 8] == b"FDAT":
                offs.append(len(plain) + pos + 8)
            pos += 12 + n
        starts.append(offs)
        plain += ent
    z = zlib.compress(bytes(plain)) if comp == 1 else bytes(plain)
    return pf.write_archive_header() + pf.write_solid_entry(comp, [z[:len(z) // 2], z[len(z) // 2:]]) + pf.finalize_archive(), starts


@pytest.mark.parametrize("comp", [1, 0])
def test_alignment_sweep(pna, ctx, pf, comp):
    """inner entries of a solid stream start at any byte: all 16 residues mod 16, each entry differing at its first, a middle and its last byte in turn"""
    names = ["n" + "x" * k for k in range(40)]
    ents = [data(k, 40000 + 36 * k) for k in range(40)]
    arc, starts = solid_archive(pf, names, ents, comp, split=3)
    assert {o[0] % 16 for o in starts} == set(range(16))
    assert len({o[1] % 16 for o in starts}) >= 8                  # the second data piece of an entry has a residue of its own
    files = dict(zip(names, ents))
    recs, s = pna.diff_archive(ctx, arc, files)
    assert [(r.name, r.status, r.first_diff, r.size) for r in recs] == [(n, pna.DIFF_SAME, None, len(e)) for n, e in zip(names, ents)]
    for where in ("first", "middle", "last", "second piece"):
        changed, want = {}, {}
        for k, (n, e) in enumerate(zip(names, ents)):
            off = {"first": 0, "middle": len(e) // 2 + k, "last": len(e) - 1, "second piece": len(e) // 3}[where]
            changed[n] = flip(e, off); want[n] = off
        recs, s = pna.diff_archive(ctx, arc, changed)
        assert [(r.name, r.status, r.first_diff) for r in recs] == [(n, pna.DIFF_CONTENTS_DIFFER, want[n]) for n in names], where
    # lengths inside a solid block: fSIZ present -> SIZE_DIFFERS; absent -> CONTENTS_DIFFER at the shorter length
    arc2, _ = solid_archive(pf, names, ents, comp, fsiz=False)
    short = {n: (e[:-3] if k % 2 else e + b"++") for k, (n, e) in enumerate(zip(names, ents))}
    recs, _ = pna.diff_archive(ctx, arc, short)
    assert all(r.status == pna.DIFF_SIZE_DIFFERS and r.first_diff is None for r in recs)
    recs, _ = pna.diff_archive(ctx, arc2, short)
    assert [(r.status, r.first_diff) for r in recs] == [(pna.DIFF_CONTENTS_DIFFER, min(len(e), len(short[n]))) for n, e in zip(names, ents)]


@pytest.mark.parametrize("algo", ["zstd", "deflate"])
def test_isolation_at_scale(pna, ctx, algo):
    n = 100000
    rng = np.random.default_rng(7)
    lens = rng.integers(50, 5001, n)
    lens[rng.choice(n, 50, replace=False)] = 0                         # zero-length entries
    pool = np.frombuffer((data(0, 1 << 20) + data(1, 1 << 20)), np.uint8)
    start = rng.integers(0, len(pool) - 5001, n)
    ents = [pool[s:s + l].tobytes() for s, l in zip(start, lens)]
    names = [f"t/{i % 100}/f{i}" for i in range(n)]
    arc = pna.create_archive(ctx, names, ents, algo=pna.ALGO_DEFLATE if algo == "deflate" else pna.ALGO_ZSTD)
    files, want, ignore = {}, {}, set()
    pick = rng.permutation(n)
    for j, i in enumerate(pick):
        i = int(i); e = ents[i]
        if j < 1000 and len(e):                                        # ~1 %: one flipped byte
            off = int(rng.integers(0, len(e))); files[names[i]] = flip(e, off); want[names[i]] = (pna.DIFF_CONTENTS_DIFFER, off)
        elif j < 2000:                                                 # ~1 %: missing
            want[names[i]] = (pna.DIFF_MISSING, None)
        elif j < 2010:
            ignore.add(names[i]); want[names[i]] = (pna.DIFF_NOT_COMPARED, None)
        elif j < 2030:                                                 # the file empty, the entry not (fSIZ present: size differs) -- or both empty
            files[names[i]] = b""; want[names[i]] = (pna.DIFF_SIZE_DIFFERS, None) if len(e) else (pna.DIFF_SAME, None)
        else:
            files[names[i]] = e; want[names[i]] = (pna.DIFF_SAME, None)

    def source(idx, path, kind, stored):
        assert path == names[idx] and stored in (len(ents[idx]), None)
        if path in ignore:
            return pna.DIFF_FS_IGNORE, None
        d = files.get(path)
        return (pna.DIFF_FS_MISSING, None) if d is None else (pna.DIFF_FS_FILE, d)
    recs, s = pna.diff_archive(ctx, arc, source)
    assert len(recs) == n and s["rc"] == 0 and s["damaged"] == 0
    bad = [(r, want[r.name]) for r in recs if (r.status, r.first_diff) != want[r.name]]
    assert not bad, bad[:5]
    assert [r.name for r in recs] == names
    assert s["same"] == sum(1 for v in want.values() if v[0] == pna.DIFF_SAME) and s["not_compared"] == 10


def _corrupt_stream(buf, ent, algo, raw_len):
    from oracle import codec
    fd = [c for c in ent if c[1] == b"FDAT"]
    _, ty, d, n = fd[0]
    if algo == "deflate":
        buf[d + n // 2] ^= 0xFF
        _, _, d2, n2 = fd[-1]
        buf[d2 + n2 - 1] ^= 0x5A
    else:
        for k in list(range(n // 2, n - 8)) + list(range(32, n // 2)):
            buf[d + k] ^= 0xFF
            try:
                codec.zstd_decompress(bytes(buf[d:d + n]), raw_len)
            except (ValueError, RuntimeError):
                break
            buf[d + k] ^= 0xFF
        else:
            raise AssertionError("no rejected corruption found")
    for c in fd:
        fix_crc(buf, c)


def check_against_verify(pna, ctx, arc, files, password, bad, names):
    """the entries in `bad` are DAMAGED with the status and flag verify gives them on the same bytes; every other entry is SAME"""
    vrecs, _ = pna.verify_archive(ctx, arc, password)
    recs, s = pna.diff_archive(ctx, arc, files, password)
    assert [r.name for r in recs] == names and len(vrecs) == len(recs)
    for i, (r, v) in enumerate(zip(recs, vrecs)):
        if i in bad:
            assert v[2] not in (pna.VERIFY_OK, pna.VERIFY_SKIPPED)
            assert (r.status, r.verify_status, r.flags & pna.VERIFY_UNAUTHENTICATED, r.first_diff) == (pna.DIFF_DAMAGED, v[2], v[3] & pna.VERIFY_UNAUTHENTICATED, None), (i, r, v)
        else:
            assert (r.status, r.verify_status, r.first_diff) == (pna.DIFF_SAME, 0, None) and v[2] == pna.VERIFY_OK, (i, r, v)
    assert s["damaged"] == len(bad) and s["same"] == len(recs) - len(bad)
    return recs


@pytest.mark.parametrize("algo", ["zstd", "deflate"])
def test_damage_crc_and_stream(pna, ctx, algo):
    n = 16
    names = [f"d/f{i}" for i in range(n)]
    ents = [data(i) for i in range(n)]
    arc = pna.create_archive(ctx, names, ents, algo=pna.ALGO_DEFLATE if algo == "deflate" else pna.ALGO_ZSTD)
    files = dict(zip(names, ents))
    buf = bytearray(arc)
    ech = entry_chunks(buf)
    _, _, d, ln = [c for c in ech[3] if c[1] == b"FDAT"][0]
    buf[d + ln // 2] ^= 0x40                                          # a payload byte: the chunk CRC fails
    _corrupt_stream(buf, ech[7], algo, len(ents[7]))                  # a corrupt stream under a repaired CRC
    recs = check_against_verify(pna, ctx, bytes(buf), files, None, {3, 7}, names)
    assert recs[3].verify_status == pna.VERIFY_BAD_CRC and recs[7].verify_status == pna.VERIFY_BAD_STREAM
    # entries settled on the host keep their status and carry the CRC finding
    files2 = dict(files); del files2[names[3]]
    recs, _ = pna.diff_archive(ctx, bytes(buf), files2)
    assert (recs[3].status, recs[3].verify_status) == (pna.DIFF_MISSING, pna.VERIFY_BAD_CRC)
    assert (recs[4].status, recs[4].verify_status) == (pna.DIFF_SAME, 0)


def test_damage_encrypted(pna, ctx):
    n = 8
    names = [f"e/f{i}" for i in range(n)]
    ents = [data(i) for i in range(n)]
    files = dict(zip(names, ents))
    for mode in (pna.MODE_CTR, pna.MODE_CBC, pna.MODE_GCM):
        arc = pna.create_archive_encrypted(ctx, names, ents, PW, mode=mode, rounds=1000)
        check_against_verify(pna, ctx, arc, files, PW, set(), names)
        recs = check_against_verify(pna, ctx, arc, files, b"wrong password", set(range(n)), names)
        if mode == pna.MODE_GCM:
            assert all(r.verify_status == pna.VERIFY_BAD_AUTH and not r.flags for r in recs)
        recs, s = pna.diff_archive(ctx, arc, files)                    # no password
        assert all(r.status == pna.DIFF_SKIPPED and r.first_diff is None for r in recs) and s["skipped"] == n
        changed = dict(files); changed[names[5]] = flip(ents[5], 9999)
        recs, _ = pna.diff_archive(ctx, arc, changed, PW)
        assert [(r.status, r.first_diff) for r in recs] == [(pna.DIFF_CONTENTS_DIFFER, 9999) if i == 5 else (pna.DIFF_SAME, None) for i in range(n)]
    arc = pna.create_archive_encrypted(ctx, names, ents, PW, mode=pna.MODE_GCM, rounds=1000)
    buf = bytearray(arc)
    fd = max((c for c in entry_chunks(buf)[3] if c[1] == b"FDAT"), key=lambda c: c[3])
    buf[fd[2] + fd[3] // 2] ^= 0x01                                   # a ciphertext bit under a repaired CRC: the segment's tag
    fix_crc(buf, fd)
    recs = check_against_verify(pna, ctx, bytes(buf), files, PW, {3}, names)
    assert recs[3].verify_status == pna.VERIFY_BAD_AUTH
    sol = bytearray(open(os.path.join(GOLDEN, "solid_zstd.pna"), "rb").read())
    sd = [c for c in chunks(sol) if c[1] == b"SDAT"][0]
    sol[sd[2] + sd[3] // 2] ^= 0x10
    recs, s = pna.diff_archive(ctx, bytes(sol), golden_files())
    assert [(r.kind, r.status, r.verify_status) for r in recs] == [(pna.VERIFY_KIND_SOLID, pna.DIFF_DAMAGED, pna.VERIFY_BAD_CRC)]
    recs, s = pna.diff_archive(ctx, open(os.path.join(GOLDEN, "solid_zstd_aes_ctr.pna"), "rb").read(), golden_files())
    assert [(r.kind, r.status) for r in recs] == [(pna.VERIFY_KIND_SOLID, pna.DIFF_SKIPPED)]


def test_kinds(pna, ctx, pf):
    """symlink entries equal / different; directory and hard-link entries are not compared, the hard link's target is delivered; type mismatches"""
    KIND_SYMLINK, KIND_HARDLINK = 2, 3
    target = b"../some/where/else.txt"
    body = pf.write_normal_entry(pf.dir_entry_header("d"), [], None)
    body += pf.write_normal_entry(pf.entry_header_bytes(KIND_SYMLINK, 0, 0, 1, "d/link"), [target], None)
    body += pf.write_normal_entry(pf.entry_header_bytes(KIND_SYMLINK, 1, 0, 1, "d/zlink"), [zlib.compress(target)], None)
    body += pf.write_normal_entry(pf.entry_header_bytes(KIND_HARDLINK, 0, 0, 1, "d/hard"), [b"d/file"], None)
    body += pf.write_normal_entry(pf.entry_header_bytes(KIND_HARDLINK, 1, 0, 1, "d/zhard"), [zlib.compress(b"d/other-file")], None)
    body += pf.write_normal_entry(pf.file_entry_header(1, "d/file"), [zlib.compress(data(1))], len(data(1)))
    arc = pf.write_archive_header() + body + pf.finalize_archive()
    fs = {"d": (pna.DIFF_FS_DIR, None), "d/link": (pna.DIFF_FS_SYMLINK, target), "d/zlink": (pna.DIFF_FS_SYMLINK, target[:5] + b"X" + target[6:]),
          "d/hard": (pna.DIFF_FS_FILE, data(1)), "d/zhard": (pna.DIFF_FS_FILE, b"whatever"), "d/file": (pna.DIFF_FS_FILE, data(1))}
    recs, s = pna.diff_archive(ctx, arc, lambda i, p, k, st: fs[p])
    assert [(r.name, r.status, r.first_diff, r.link_target) for r in recs] == [
        ("d", pna.DIFF_NOT_COMPARED, None, None), ("d/link", pna.DIFF_SAME, None, None), ("d/zlink", pna.DIFF_SYMLINK_DIFFERS, 5, None),
        ("d/hard", pna.DIFF_NOT_COMPARED, None, b"d/file"), ("d/zhard", pna.DIFF_NOT_COMPARED, None, b"d/other-file"), ("d/file", pna.DIFF_SAME, None, None)]
    assert s["not_compared"] == 3 and s["differ"] == 1 and s["same"] == 2
    fs2 = {"d": (pna.DIFF_FS_FILE, b"x"), "d/link": (pna.DIFF_FS_FILE, target), "d/zlink": (pna.DIFF_FS_SYMLINK, target + b"/"),
           "d/hard": (pna.DIFF_FS_DIR, None), "d/zhard": (pna.DIFF_FS_MISSING, None), "d/file": (pna.DIFF_FS_OTHER, None)}
    recs, s = pna.diff_archive(ctx, arc, lambda i, p, k, st: fs2[p])
    assert [(r.status, r.first_diff, r.link_target) for r in recs] == [
        (pna.DIFF_TYPE_MISMATCH, None, None), (pna.DIFF_TYPE_MISMATCH, None, None), (pna.DIFF_SYMLINK_DIFFERS, len(target), None),
        (pna.DIFF_TYPE_MISMATCH, None, None), (pna.DIFF_MISSING, None, None), (pna.DIFF_TYPE_MISMATCH, None, None)]


def test_slots_pieces_and_pinned_bound(pna, ctx):
    """an entry larger than two slots, slots of 1 MiB: pieces and slot recycling; the page-locked memory stays at two slots while 256 MiB are compared"""
    c2 = pna.Context(0)
    try:
        c2.set_option("diff_slot_mib", 1)
        big = (data(0, 1 << 20) * 6)[:5 * MIB + 777]
        n = 256
        ents = [big] + [data(i, MIB) for i in range(1, n)]
        names = [f"p/f{i}" for i in range(n)]
        arc = pna.create_archive(c2, names, ents)
        c2._L.pna_gpu_debug_pinned_bytes.restype = ctypes.c_uint64
        before = c2._L.pna_gpu_debug_pinned_bytes(c2._h)
        files = dict(zip(names, ents))
        files[names[0]] = flip(big, 3 * MIB + 5, 4 * MIB)
        files[names[9]] = flip(ents[9], MIB - 1)
        files[names[200]] = flip(ents[200], 0)
        recs, s = pna.diff_archive(c2, arc, files)
        want = {0: 3 * MIB + 5, 9: MIB - 1, 200: 0}
        assert [(r.status, r.first_diff) for r in recs] == [(pna.DIFF_CONTENTS_DIFFER, want[i]) if i in want else (pna.DIFF_SAME, None) for i in range(n)]
        grown = c2._L.pna_gpu_debug_pinned_bytes(c2._h) - before
        assert 0 < grown <= 2 * MIB, grown                            # the documented bound: two slots of diff_slot_mib
        assert pna.diff_stats(c2)[1] == sum(len(e) for e in ents)
    finally:
        c2.close()


def test_lent_buffer_is_compared_in_place(pna, ctx):
    """file bytes inside a pna_gpu_host_alloc buffer are copied to the device from there (no staging), mixed with bytes elsewhere"""
    n = 12
    ents = [data(i, 100000 + i) for i in range(n)]
    names = [f"l/f{i}" for i in range(n)]
    arc = pna.create_archive(ctx, names, ents)
    slot = pna.HostSlot(ctx, 4 * MIB)
    try:
        where, pos = {}, 0
        for i in range(0, n, 2):                                      # every other file lies in the page-locked buffer, at odd addresses
            e = ents[i] if i != 4 else flip(ents[i], 4242)
            pos += 3
            slot.view[pos:pos + len(e)] = e
            where[names[i]] = (slot.ptr + pos, len(e)); pos += len(e)

        def source(idx, path, kind, stored):
            return pna.DIFF_FS_FILE, where.get(path, ents[idx] if idx != 7 else flip(ents[idx], 1))
        recs, s = pna.diff_archive(ctx, arc, source)
        want = {4: 4242, 7: 1}
        assert [(r.status, r.first_diff) for r in recs] == [(pna.DIFF_CONTENTS_DIFFER, want[i]) if i in want else (pna.DIFF_SAME, None) for i in range(n)]
    finally:
        slot.free()


CHILD = r"""
import resource, sys
sys.path.insert(0, sys.argv[1])
import importlib, torch
pna = importlib.import_module("portable-network-archive_amd")
from oracle import codec
base = [codec.corpus_file(k % 3, k, 4 << 20) for k in range(16)]
arc = open(sys.argv[2], "rb").read()
with pna.Context(0) as ctx:
    ctx.set_option("diff_slot_mib", 64)
    small = pna.create_archive(ctx, ["f0", "f1"], base[:2])
    pna.diff_archive(ctx, small, {"f0": base[0], "f1": base[1]})            # warm the context on a small archive
    r0 = resource.getrusage(resource.RUSAGE_SELF).ru_maxrss
    recs, s = pna.diff_archive(ctx, arc, lambda i, p, k, st: (pna.DIFF_FS_FILE, base[i % 16]))
    r1 = resource.getrusage(resource.RUSAGE_SELF).ru_maxrss
    assert s["same"] == len(recs) == 1024 and s["rc"] == 0, s
print("RSS_KIB", r1 - r0, sum(r.size for r in recs))
"""


def test_no_decoded_bytes_on_host(pna, ctx, tmp_path):
    """4 GiB of decoded entries compared: the process grows by the two slots and the window's workspace, not by the decoded bytes"""
    n = 1024
    base = [data(k, 4 << 20) for k in range(16)]
    arc = pna.create_archive(ctx, [f"f{i}" for i in range(n)], [base[i % 16] for i in range(n)])
    p = tmp_path / "big.pna"; p.write_bytes(arc)
    del arc
    out = subprocess.run(["timeout", "-k", "10", "300", sys.executable, "-c", CHILD, ROOT, str(p)], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-3000:]
    line = [l for l in out.stdout.splitlines() if l.startswith("RSS_KIB")][0].split()
    grow, nbytes = int(line[1]), int(line[2])
    assert nbytes == 4 << 30
    assert grow < (1 << 20), grow                                      # KiB: under 1 GiB


def test_callback_errors(pna, ctx):
    n = 6
    names = [f"c/f{i}" for i in range(n)]
    ents = [data(i) for i in range(n)]
    arc = pna.create_archive(ctx, names, ents)
    parts = (ctypes.c_char_p * 1)(arc)
    lens = (ctypes.c_size_t * 1)(len(arc))
    keep = []

    def src(_u, idx, name, kind, stored, out):
        keep.append(ents[idx])
        out[0].fs_kind, out[0].data, out[0].len = pna.DIFF_FS_FILE, ctypes.cast(ctypes.c_char_p(ents[idx]), ctypes.c_void_p).value, len(ents[idx])
        return 0
    seen = []
    f = ctx._L.pna_gpu_diff_archive_host
    summ = pna.DiffSummary()
    assert f(ctx._h, parts, lens, 1, None, 0, pna.DIFF_SOURCE_FN(src), pna.DIFF_FN(lambda _u, i, *a: (seen.append(i), 1 if i == 2 else 0)[1]), None, ctypes.byref(summ)) == PNA_E_SINK
    assert seen == [0, 1, 2]
    assert f(ctx._h, parts, lens, 1, None, 0, pna.DIFF_SOURCE_FN(lambda _u, i, *a: 1 if i == 3 else src(_u, i, *a)), pna.DIFF_FN(lambda *a: 0), None, None) == PNA_E_SINK
    recs, s = pna.diff_archive(ctx, arc, dict(zip(names, ents)))      # the context works on
    assert s["same"] == n and s["rc"] == 0
    with pytest.raises(KeyError):                                      # an exception in a Python source is raised, not swallowed
        pna.diff_archive(ctx, arc, lambda i, p, k, st: {}[p])
    recs, s = pna.diff_archive(ctx, arc, dict(zip(names, ents)))
    assert s["same"] == n


def test_argument_checks_with_a_context(pna, ctx):
    L = ctx._L
    arc = pna.create_archive(ctx, ["a", "b"], [data(0), data(1)])
    parts = (ctypes.c_char_p * 1)(arc)
    lens = (ctypes.c_size_t * 1)(len(arc))
    src = pna.DIFF_SOURCE_FN(lambda *a: 0)                              # (fills nothing: every entry is missing)
    cb = pna.DIFF_FN(lambda *a: 0)
    f = L.pna_gpu_diff_archive_host
    summ = pna.DiffSummary()
    assert f(ctx._h, parts, lens, 1, None, 0, src, cb, None, ctypes.byref(summ)) == 0 and summ.differ == 2 and summ.total == 2
    assert f(ctx._h, None, lens, 1, None, 0, src, cb, None, None) == PNA_E_INVAL
    assert f(ctx._h, parts, None, 1, None, 0, src, cb, None, None) == PNA_E_INVAL
    assert f(ctx._h, parts, lens, 0, None, 0, src, cb, None, None) == PNA_E_INVAL
    assert f(ctx._h, parts, lens, 1, None, 0, ctypes.cast(None, pna.DIFF_SOURCE_FN), cb, None, None) == PNA_E_INVAL
    assert f(ctx._h, parts, lens, 1, None, 0, src, ctypes.cast(None, pna.DIFF_FN), None, None) == PNA_E_INVAL
    assert f(ctx._h, parts, lens, 1, None, 5, src, cb, None, None) == PNA_E_INVAL
    recs, s = pna.diff_archive(ctx, arc[:len(arc) - 30], {"a": data(0), "b": data(1)})     # cut inside the last entry: the structure breaks off
    assert s["rc"] == PNA_E_INVAL and s["broken"] == 1 and [r.status for r in recs] == [pna.DIFF_SAME]
