"""pna_gpu_extract_select_host and k_pick: chosen entries of an archive, to host memory or to device memory of the caller's.
Every expectation is computed from plain bytes (tests/golden/raw, oracle.codec.corpus_file), from archives written by oracle/pna_format.py or the
library's own create calls, and from extract_archive for equality with the path that hands out every entry."""
import ctypes
import os
import struct
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
PW = b"password"
PNA_E_INVAL, PNA_E_SINK = -2, -6
MIB = 1 << 20
GUARD = 64
SIZES = [0, 1, 15, 16, 17, 4095, 20000, MIB + 3] + [20000] * 32


@pytest.fixture(scope="module")
def ctx(pna):
    import torch  # noqa: F401
    c = pna.Context(0)
    yield c
    c.close()


def data(i, n=20000):
    from oracle import codec
    return codec.corpus_file(i % 3, i, n)


def golden(name):
    return open(os.path.join(GOLDEN, name), "rb").read()


def golden_files():
    out = {}
    for d, _, fs in os.walk(os.path.join(GOLDEN, "raw")):
        for f in fs:
            p = os.path.join(d, f)
            out[os.path.relpath(p, GOLDEN).replace(os.sep, "/")] = open(p, "rb").read()
    return out


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


def flip_fdat(arc, entry):
    """one byte flipped in the middle of the entry's (first) FDAT chunk"""
    fd = [ch for ch in entry_chunks(arc)[entry] if ch[1] == b"FDAT"][0]
    b = bytearray(arc)
    b[fd[2] + fd[3] // 2] ^= 0x5A
    return bytes(b)


class Guarded:
    """destinations carved from one tensor pre-filled with 0xA5, GUARD bytes between neighbours, each at a chosen offset mod 16"""

    def __init__(self, lens, mods):
        import torch
        self.pos, at = [], GUARD
        for n, m in zip(lens, mods):
            at += (m - at) % 16
            self.pos.append(at)
            at += n + GUARD
        self.t = torch.full((at + 32,), 0xA5, dtype=torch.uint8, device="cuda")
        assert self.t.data_ptr() % 16 == 0
        self.lens = list(lens)

    def tensor(self, k, cap=None):
        return self.t[self.pos[k]:self.pos[k] + (self.lens[k] if cap is None else cap)]

    def check(self, contents):
        """contents[k]: the bytes expected in destination k (None: untouched); everything else is still 0xA5"""
        want = np.full(self.t.numel(), 0xA5, np.uint8)
        for k, c in enumerate(contents):
            if c is not None:
                want[self.pos[k]:self.pos[k] + len(c)] = np.frombuffer(c, np.uint8)
        got = self.t.cpu().numpy()
        bad = np.flatnonzero(got != want)
        assert len(bad) == 0, ("first wrong byte at", int(bad[0]), "of", len(bad))


# ---- 1. k_pick alone
def test_k_pick_alignment_grid(pna, ctx):
    import torch
    T = pna.PICK_TILE
    assert T == 16384
    lengths = [0, 1, 15, 16, 17, 63, 64, 65, T - 1, T, T + 1, 3 * T + 5]
    rng = np.random.RandomState(5)
    cases = [(s, d, lengths[(s + d + j) % 12]) for s in range(16) for d in range(16) for j in range(12)]     # every length at every (source, destination) offset mod 16
    src_pos, at = [], 16
    for s, _, n in cases:
        at += (s - at) % 16
        src_pos.append(at)
        at += n + 3
    host = rng.randint(0, 256, at + 32, dtype=np.uint8)
    src = torch.from_numpy(host).cuda()
    g = Guarded([n for _, _, n in cases], [d for _, d, _ in cases])
    assert {(p % 16, q % 16) for p, q in zip(src_pos, g.pos)} == {(s, d) for s in range(16) for d in range(16)}
    pna.pick_device(ctx, src, src_pos, [g.t.data_ptr() + p for p in g.pos], [n for _, _, n in cases])
    g.check([host[p:p + n].tobytes() for p, (_, _, n) in zip(src_pos, cases)])
    assert pna.extract_stats(ctx)[3] == sum(n for _, _, n in cases)


def test_k_pick_one_large_piece(pna, ctx):
    import torch
    n = 40 * MIB + 3
    src = torch.randint(0, 256, (n + 64,), dtype=torch.uint8, device="cuda")
    g = Guarded([n], [9])
    pna.pick_device(ctx, src, [7], [g.t.data_ptr() + g.pos[0]], [n])
    assert torch.equal(g.tensor(0), src[7:7 + n])
    assert bool((g.t[:g.pos[0]] == 0xA5).all()) and bool((g.t[g.pos[0] + n:] == 0xA5).all())


# ---- 2. / 3. subsets of a 40-entry archive
_ARCS = {}


def archive40(pna, ctx, pf, algo):
    if algo not in _ARCS:
        ents = [(data(i, 1 << 18) * 5)[:n] if n > (1 << 18) else data(i, n) for i, n in enumerate(SIZES)]
        names = ["d/e%02d" % i for i in range(len(ents))]
        if algo == "store":
            arc = pf.write_archive_header() + b"".join(pf.write_normal_entry(pf.file_entry_header(0, nm), [e] if e else [], len(e))
                                                       for nm, e in zip(names, ents)) + pf.finalize_archive()
        else:
            arc = pna.create_archive(ctx, names, ents, algo={"zstd": pna.ALGO_ZSTD, "deflate": pna.ALGO_DEFLATE}[algo])
        ref = pna.extract_archive(ctx, arc)
        assert [(nm, 0, e) for nm, e in zip(names, ents)] == ref
        _ARCS[algo] = (arc, names, ents)
    return _ARCS[algo]


@pytest.mark.parametrize("algo", ["zstd", "deflate", "store"])
def test_subset_to_host(pna, ctx, pf, algo):
    arc, names, ents = archive40(pna, ctx, pf, algo)
    asked = []

    def sel(i, name, kind, stored):
        asked.append((i, name, kind, stored))
        return "host" if i % 3 == 0 else None
    recs, s = pna.extract_select(ctx, arc, sel)
    picked = list(range(0, 40, 3))
    assert asked == [(i, names[i], 0, len(ents[i])) for i in range(40)]
    assert recs == [(i, names[i], 0, pna.EXTRACT_OK, ents[i], len(ents[i])) for i in picked]
    assert s == {"total": 40, "selected": len(picked), "to_host": len(picked), "to_device": 0, "too_small": 0}
    up, streams, kdf, moved, _ = pna.extract_stats(ctx)
    assert streams == len(picked) and kdf == 0 and moved == 0
    lst = pna.list_entries(arc)
    assert len(lst) == 40
    plan = pna.extract_plan_runs([e[2] for e in lst], [e[3] for e in lst], [i % 3 == 0 for i in range(40)])
    print("uploaded", up, "planned", sum(n for _, n in plan), "archive", len(arc))
    assert 0 < up <= sum(n for _, n in plan) and up < len(arc)
    recs, s = pna.extract_select(ctx, arc, lambda *a: None)
    assert recs == [] and s["total"] == 40 and s["selected"] == 0
    assert pna.extract_stats(ctx)[:2] == (0, 0)


@pytest.mark.parametrize("algo", ["zstd", "deflate", "store"])
def test_subset_to_device(pna, ctx, pf, algo):
    arc, names, ents = archive40(pna, ctx, pf, algo)
    picked = [i for i in range(40) if i % 3]
    g = Guarded([len(ents[i]) for i in picked], [(5 * k + 3) % 16 for k in range(len(picked))])
    assert len({p % 16 for p in g.pos}) == 16
    slot = {i: k for k, i in enumerate(picked)}
    recs, s = pna.extract_select(ctx, arc, lambda i, *a: g.tensor(slot[i]) if i in slot else None)
    assert [(r[0], r[1], r[3], r[5]) for r in recs] == [(i, names[i], pna.EXTRACT_OK, len(ents[i])) for i in picked]
    assert all(r[4].data_ptr() == g.t.data_ptr() + g.pos[slot[r[0]]] for r in recs)
    g.check([ents[i] for i in picked])
    assert pna.extract_stats(ctx)[3] == sum(len(ents[i]) for i in picked) and s["to_device"] == len(picked)
    # host and device destinations in one call
    g2 = Guarded([len(ents[i]) for i in picked], [(7 * k + 1) % 16 for k in range(len(picked))])
    recs, s = pna.extract_select(ctx, arc, lambda i, *a: g2.tensor(slot[i]) if i in slot else ("host" if i % 3 == 0 else None))
    assert [r[0] for r in recs] == sorted(picked + list(range(0, 40, 3)))
    assert all(r[4] == ents[r[0]] for r in recs if r[0] % 3 == 0) and s["to_host"] == 14 and s["to_device"] == 26
    g2.check([ents[i] for i in picked])


# ---- 4. TOO_SMALL, entries without fSIZ
def test_too_small(pna, ctx, pf):
    arc, names, ents = archive40(pna, ctx, pf, "zstd")
    picked = [5, 6, 7, 8]                                              # 4 095, 20 000, 1 MiB + 3, 20 000 bytes
    g = Guarded([len(ents[i]) for i in picked], [1, 2, 3, 4])
    caps = {5: None, 6: None, 7: len(ents[7]) - 1, 8: None}
    recs, s = pna.extract_select(ctx, arc, lambda i, *a: g.tensor(picked.index(i), caps[i]) if i in caps else None)
    assert [(r[0], r[3], r[5]) for r in recs] == [(5, 0, 4095), (6, 0, 20000), (7, pna.EXTRACT_TOO_SMALL, MIB + 3), (8, 0, 20000)]
    assert recs[2][4] is None and s["too_small"] == 1 and s["to_device"] == 3
    g.check([ents[5], ents[6], None, ents[8]])


def test_entry_without_fsiz(pna, ctx, pf):
    raw = data(2, 300001)
    out = bytearray(pf.write_archive_header())
    pna.write_file(ctx, out.extend, "s/entry", [raw[:100000], raw[100000:]])
    arc = bytes(out) + pf.finalize_archive()
    assert pf.read_archive(arc)[1][0].raw_file_size is None
    offered = []
    g = Guarded([len(raw), len(raw)], [11, 6])
    recs, _ = pna.extract_select(ctx, arc, lambda i, nm, k, stored: (offered.append(stored), g.tensor(0, len(raw) - 1))[1])
    assert offered == [None] and [(r[3], r[4], r[5]) for r in recs] == [(pna.EXTRACT_TOO_SMALL, None, len(raw))]      # the true size
    g.check([None, None])
    recs, _ = pna.extract_select(ctx, arc, lambda *a: g.tensor(1))
    assert [(r[1], r[3], r[5]) for r in recs] == [("s/entry", pna.EXTRACT_OK, len(raw))]
    g.check([None, raw])
    assert pna.extract_select(ctx, arc, lambda *a: "host")[0][0][4] == raw


# ---- 5. solid blocks
@pytest.mark.parametrize("fname", ["solid_zstd.pna", "solid_deflate.pna"])
def test_solid_golden(pna, ctx, fname):
    files = golden_files()
    dev = ["raw/images/icon.png", "raw/text.txt"]
    host = "raw/images/icon.svg"
    g = Guarded([len(files[n]) for n in dev], [13, 2])
    recs, s = pna.extract_select(ctx, golden(fname), lambda i, nm, k, st: g.tensor(dev.index(nm)) if nm in dev else ("host" if nm == host else None))
    assert sorted(r[1] for r in recs) == sorted(dev + [host]) and s["to_device"] == 2 and s["to_host"] == 1 and s["total"] >= 5
    assert [r[4] for r in recs if r[1] == host] == [files[host]]
    g.check([files[n] for n in dev])
    assert pna.extract_stats(ctx)[1] >= 1                              # a block is one stream


@pytest.mark.parametrize("comp", [1, 0])
def test_solid_inner_entries_at_odd_offsets(pna, ctx, pf, comp):
    ents = [data(k, n) for k, n in enumerate([1, 17, 4097, 16, 0, 70001, 15])]
    names = ["in/n%d" % k for k in range(len(ents))]
    plain = b"".join(pf.write_normal_entry(pf.file_entry_header(0, nm), [e[:len(e) // 3], e[len(e) // 3:]] if len(e) > 1 else ([e] if e else []), len(e))
                     for nm, e in zip(names, ents))
    z = zlib.compress(plain) if comp == 1 else plain
    arc = pf.write_archive_header() + pf.write_solid_entry(comp, [z[:len(z) // 2], z[len(z) // 2:]]) + pf.finalize_archive()
    g = Guarded([len(e) for e in ents], [3 * k % 16 for k in range(len(ents))])
    recs, s = pna.extract_select(ctx, arc, lambda i, *a: g.tensor(i))
    assert [(r[0], r[1], r[3], r[5]) for r in recs] == [(k, names[k], 0, len(ents[k])) for k in range(len(ents))]
    g.check(ents)
    assert pna.extract_stats(ctx)[3] == sum(len(e) for e in ents)
    assert [r[4] for r in pna.extract_select(ctx, arc, lambda *a: "host")[0]] == ents


# ---- 6. encrypted
@pytest.mark.parametrize("fname", ["zstd_aes_ctr.pna", "zstd_aes_cbc.pna", "zstd_aes_gcm.pna", "solid_zstd_aes_gcm.pna"])
def test_encrypted_one_entry_to_device(pna, ctx, fname):
    files = golden_files()
    want = "raw/images/icon.png"
    g = Guarded([len(files[want])], [5])
    recs, s = pna.extract_select(ctx, golden(fname), lambda i, nm, k, st: g.tensor(0) if nm == want else None, PW)
    assert [(r[1], r[3], r[5]) for r in recs] == [(want, 0, len(files[want]))]
    g.check([files[want]])
    assert pna.extract_stats(ctx)[2] == 1                              # one PHSF string, derived once


def test_wrong_password(pna, ctx):
    recs, s = pna.extract_select(ctx, golden("zstd_aes_ctr.pna"), lambda *a: None, b"wrong")
    assert recs == [] and s["total"] >= 5 and pna.extract_stats(ctx)[2] == 0      # nothing selected: no key derived, PNA_OK
    with pytest.raises(pna.PnaGpuError) as e:
        pna.extract_select(ctx, golden("zstd_aes_gcm.pna"), lambda i, nm, k, st: "host" if nm == "raw/text.txt" else None, b"wrong")
    assert e.value.code == PNA_E_INVAL


# ---- 7. parts
def test_golden_multipart(pna, ctx):
    parts = [golden(f"multipart.part{k}.pna") for k in (1, 2)]
    ref = pna.extract_archive(ctx, pna.join_parts(parts))
    assert len(ref) >= 1
    recs, _ = pna.extract_select(ctx, parts, lambda *a: "host")
    assert [(r[1], r[2], r[4]) for r in recs] == ref
    g = Guarded([len(d) for _, _, d in ref], [(3 + 5 * k) % 16 for k in range(len(ref))])
    recs, _ = pna.extract_select(ctx, parts, lambda i, *a: g.tensor(i))
    assert [r[3] for r in recs] == [0] * len(ref)
    g.check([d for _, _, d in ref])
    with pytest.raises(pna.PnaGpuError) as e:
        pna.extract_select(ctx, parts[:1], lambda *a: "host")
    assert e.value.code == PNA_E_INVAL


def test_entry_spanning_parts(pna, ctx, pf):
    rng = np.random.RandomState(11)
    ents = [rng.randint(0, 256, 100000, dtype=np.uint8).tobytes() for _ in range(3)]
    arc = pf.write_archive_header() + b"".join(pf.write_normal_entry(pf.file_entry_header(0, "p%d" % k), [e], len(e)) for k, e in enumerate(ents)) + pf.finalize_archive()
    parts = pna.split_archive(arc, 120000)
    assert len(parts) >= 3 and pna.extract_archive(ctx, pna.join_parts(parts)) == [("p%d" % k, 0, e) for k, e in enumerate(ents)]
    # entry 1's data starts in the first part and ends in the second
    assert sum(1 for ch in chunks(parts[0]) if ch[1] == b"FDAT") == 2 and any(ch[1] == b"FDAT" for ch in chunks(parts[1]))
    g = Guarded([100000], [7])
    recs, _ = pna.extract_select(ctx, parts, lambda i, *a: g.tensor(0) if i == 1 else None)
    assert [(r[0], r[3], r[5]) for r in recs] == [(1, 0, 100000)]
    g.check([ents[1]])
    with pytest.raises(pna.PnaGpuError) as e:
        pna.extract_select(ctx, parts[:-1], lambda *a: None)
    assert e.value.code == PNA_E_INVAL


# ---- 8. damage, callback failures
def raw_call(pna, ctx, arc, sel, flags=0):
    """the C entry point with a select callback of the test's own: (rc, records)"""
    recs = []
    parts, lens = (ctypes.c_char_p * 1)(arc), (ctypes.c_size_t * 1)(len(arc))
    cb = pna.EXTRACT_RECORD_FN(lambda _u, i, nm, k, st, d, n: (recs.append((i, st, n)), 0)[1])
    rc = ctx._L.pna_gpu_extract_select_host(ctx._h, parts, lens, 1, None, 0, flags, pna.EXTRACT_SELECT_FN(sel), cb, None, None)
    return rc, recs


def test_damage(pna, ctx, pf):
    arc, names, ents = archive40(pna, ctx, pf, "zstd")
    bad = flip_fdat(arc, 10)
    sel = lambda i, *a: "host" if i in (9, 12) else None                # noqa: E731
    recs, _ = pna.extract_select(ctx, bad, sel)                       # damage in an entry that is not selected: not looked at ...
    assert [(r[0], r[4]) for r in recs] == [(9, ents[9]), (12, ents[12])]
    with pytest.raises(pna.PnaGpuError) as e:                          # ... unless every data chunk is to be checked
        pna.extract_select(ctx, bad, sel, check_all=True)
    assert e.value.code == PNA_E_INVAL
    assert [r[0] for r in pna.extract_select(ctx, arc, sel, check_all=True)[0]] == [9, 12]
    assert pna.extract_stats(ctx)[1] == 2                              # (checked, not decoded)
    for check_all in (False, True):
        with pytest.raises(pna.PnaGpuError) as e:
            pna.extract_select(ctx, flip_fdat(arc, 12), sel, check_all=check_all)
        assert e.value.code == PNA_E_INVAL


def test_callback_failures(pna, ctx, pf):
    import torch
    arc, names, ents = archive40(pna, ctx, pf, "store")

    def boom(i, *a):
        if i == 4:
            raise KeyError("no")
        return "host"
    with pytest.raises(pna.PnaGpuError) as e:
        pna.extract_select(ctx, arc, boom)
    assert e.value.code == PNA_E_SINK and isinstance(e.value.__cause__, KeyError)
    assert raw_call(pna, ctx, arc, lambda _u, i, nm, k, st, out: 1 if i == 2 else 0) == (PNA_E_SINK, [])
    dst = torch.empty(64, dtype=torch.uint8, device="cuda")

    def null_dst(_u, i, nm, k, st, out):
        out[0].where, out[0].d_dst, out[0].cap = pna.EXTRACT_DEVICE, None, 16
        return 0
    assert raw_call(pna, ctx, arc, null_dst)[0] == PNA_E_INVAL

    def odd_where(_u, i, nm, k, st, out):
        out[0].where = 3
        return 0
    assert raw_call(pna, ctx, arc, odd_where)[0] == PNA_E_INVAL
    assert raw_call(pna, ctx, arc, lambda *a: 0, flags=2)[0] == PNA_E_INVAL       # an unknown flag

    def small(_u, i, nm, k, st, out):                                  # entry 3 (16 bytes) into 64 bytes, entry 0 (empty) into a null destination of no bytes
        if i == 3:
            out[0].where, out[0].d_dst, out[0].cap = pna.EXTRACT_DEVICE, dst.data_ptr(), 64
        elif i == 0:
            out[0].where = pna.EXTRACT_DEVICE
        return 0
    assert raw_call(pna, ctx, arc, small) == (0, [(0, 0, 0), (3, 0, 16)])
    assert dst[:16].cpu().numpy().tobytes() == ents[3]


# ---- 9. windows are cut by the bytes uploaded
def test_sparse_windows(pna, ctx, pf):
    base = data(1, 1 << 18) * 4
    ents = [struct.pack("<Q", i) + base[8:] for i in range(600)]
    arc = pf.write_archive_header() + b"".join(pf.write_normal_entry(pf.file_entry_header(0, "w%03d" % i), [e], MIB) for i, e in enumerate(ents)) + pf.finalize_archive()
    g = Guarded([MIB], [9])
    ctx.set_option("extract_win_mib", 64)
    try:
        recs, _ = pna.extract_select(ctx, arc, lambda i, *a: "host" if i in (0, 599) else (g.tensor(0) if i == 299 else None))
    finally:
        ctx.set_option("extract_win_mib", 1024)
    assert [(r[0], r[1], r[5]) for r in recs] == [(0, "w000", MIB), (299, "w299", MIB), (599, "w599", MIB)]
    assert recs[0][4] == ents[0] and recs[2][4] == ents[599]
    g.check([ents[299]])
    up = pna.extract_stats(ctx)[0]
    assert 3 * MIB <= up < 4 * MIB


# ---- 10. extract_to_device
@pytest.mark.parametrize("fname", ["zstd.pna", "zstd_with_raw_file_size.pna"])
def test_extract_to_device(pna, ctx, pf, fname):
    files = golden_files()
    arc = golden(fname)
    has_size = [e.raw_file_size is not None for e in pf.read_archive(arc)[1]]
    assert all(has_size) if "raw_file_size" in fname else not any(has_size)
    out = pna.extract_to_device(ctx, arc)
    ref = {name: d for name, kind, d in pna.extract_archive(ctx, arc) if kind == 0}
    assert len(out) >= 5 and set(out) == set(ref) and {"raw/images/icon.png", "raw/text.txt", "raw/empty.txt"} <= set(out)
    assert len(set(out) & set(files)) >= 5                              # (the fixture also holds a file that tests/golden/raw does not)
    for name, t in out.items():
        assert t.is_cuda and t.cpu().numpy().tobytes() == ref[name], name
        assert name not in files or ref[name] == files[name], name
    one = pna.extract_to_device(ctx, arc, names=["raw/text.txt"])
    assert list(one) == ["raw/text.txt"] and one["raw/text.txt"].cpu().numpy().tobytes() == files["raw/text.txt"]
