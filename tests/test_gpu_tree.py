"""`pna create some/tree` in one call: the create paths with entry kinds (pna_gpu_create_archive_tree_host / _device and the solid forms) -- directories,
symbolic links and hard links between the files, in walk order (create_entry's four arms, cli/src/command/core.rs:915-977).

Expected bytes (tests/tree_cases.py): archive header + records in order + AEND, a file's record cut out of what the existing
pna_gpu_create_archive_chunked_host writes for the files alone (same options, same IVs), every other record the oracle's.  Solid archives: the SDAT
stream decoded with the oracle must be the oracle's serialisation of the inner records, and the host form must equal the device form."""
import os

import pytest

import tree_cases as tc

pytestmark = pytest.mark.gpu

_cache = {}


def _memo(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def _lists(codec, which):
    return _memo(("list", which), lambda: {"12": tc.entries12, "2500": tc.entries2500}[which](codec))


def _key(pna):
    return _memo("key", lambda: pna.kdf_pbkdf2_sha256(b"password", bytes(range(16)), 1000))


def _cipher(pna, mode, n):
    """None, or the cipher with one IV slot per entry (the slots of entries that are not files stay unused)"""
    if mode is None:
        return None
    key, phsf = _key(pna)
    if mode == "ctr":
        return pna.Cipher(key, phsf, pna.MODE_CTR, ivs=bytes((7 * i + 1) & 255 for i in range(16 * n)))
    return pna.Cipher(key, phsf, pna.MODE_GCM, ivs=bytes((5 * i + 3) & 255 for i in range(39 * n)), gcm_segment_size=65536)


def _upload(entries):
    """the files' bytes in one device buffer at 16-byte aligned offsets; the offsets of the other entries are never read"""
    import torch
    _names, datas, _kinds, _links = tc.tree_args(entries)
    offs, pos = [], 0
    for d in datas:
        offs.append(pos)
        pos = (pos + len(d) + 15) & ~15
    host = bytearray(pos + 8192)
    for o, d in zip(offs, datas):
        host[o:o + len(d)] = d
    src = torch.frombuffer(host, dtype=torch.uint8).cuda()
    return src, offs


def _device_form(pna, ctx, entries, algo, level, cipher=None, extra=None, facets=None, mcs=0, solid=False, kinds_none=False):
    import torch
    names, datas, kinds, links = tc.tree_args(entries)
    lens = [len(d) for d in datas]
    src, offs = _upload(entries)
    bound = pna.solid_archive_tree_bound if solid else pna.archive_tree_bound
    cap = bound(algo, names, lens, kinds, links, cipher=cipher, facets=facets, extra=extra, max_chunk_size=mcs)
    dst = torch.zeros(cap + 64, dtype=torch.uint8, device="cuda")
    total, eoff = ctx.create_archive_tree_device(names, src.data_ptr(), offs, lens, dst.data_ptr(), cap, None if kinds_none else kinds, None if kinds_none else links,
                                                 algo=algo, level=level, cipher=cipher, facets=facets, extra=extra, max_chunk_size=mcs, solid=solid)
    assert total <= cap
    return dst[:total].cpu().numpy().tobytes(), eoff


def _host_form(pna, ctx, entries, algo, level, cipher=None, extra=None, facets=None, mcs=0, solid=False):
    names, datas, kinds, links = tc.tree_args(entries)
    return pna.create_archive_tree(ctx, names, datas, kinds, links, algo=algo, level=level, cipher=cipher, facets=facets, extra=extra, max_chunk_size=mcs, solid=solid)


def _both_forms_equal(pna, ctx, entries, want, offs, algo, level, **kw):
    """host form and device form, the host layout and the device layout (option dev_layout): every one byte-equal to `want`"""
    for dev_layout in (0, 1):
        with ctx.options(dev_layout=(dev_layout, 1)):
            got = _host_form(pna, ctx, entries, algo, level, **kw)
            assert got == want, ("host", dev_layout, len(got), len(want))
            got, eoff = _device_form(pna, ctx, entries, algo, level, **kw)
            assert got == want, ("device", dev_layout, len(got), len(want))
            assert eoff == offs, ("entry_off", dev_layout)


CODECS = {"zstd3": (2, 3), "deflate6": (1, 6), "stored": (1, 0)}          # (algo, level); "stored": deflate 0 = Compression::none(), the codec stage's stored form
VARIANTS = {"plain": (None, 0), "plain-mcs1000": (None, 1000), "ctr": ("ctr", 0), "ctr-mcs1000": ("ctr", 1000), "gcm": ("gcm", 0)}


@pytest.mark.parametrize("codec_name", list(CODECS))
@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("with_facets", (False, True))
def test_twelve_entries_byte_equal(pna, pf, codec, gpu_ctx, codec_name, variant, with_facets):
    """The 12-entry list (first and last are directories; an empty file next to a directory; a 2 500-byte link target) on both forms and both layouts.
    With a cipher the file records are the files-only call's and the link records stay unencrypted: both follow from equality with the expected archive."""
    algo, level = CODECS[codec_name]
    mode, mcs = VARIANTS[variant]
    entries = _lists(codec, "12")
    cipher = _cipher(pna, mode, len(entries))
    extra, facets = tc.facet_blobs(pf, entries) if with_facets else (None, None)
    want, offs = tc.expected_archive(pna, pf, gpu_ctx, entries, algo, level, cipher, extra, facets, mcs)
    _both_forms_equal(pna, gpu_ctx, entries, want, offs, algo, level, cipher=cipher, extra=extra, facets=facets, mcs=mcs)
    items = pf.read_archive(want)[1]                                     # (the expected archive itself reads back: kinds, names, and links in the clear)
    assert [(it.kind, it.name) for it in items] == [(k, pf.sanitize_name(n)) for k, n, _d in entries]
    for it, (k, _n, d) in zip(items, entries):
        if k != tc.FILE:
            assert (it.data, it.encryption, it.raw_file_size) == (d, 0, None)
            if k != tc.DIR and mcs:
                assert [len(x) for t, x in it.chunks if t == b"FDAT"] == [len(p) for p in pf.flatten_writer([d], mcs)]
        else:
            assert it.encryption == (0 if mode is None else 1)


@pytest.mark.parametrize("mode", (None, "ctr", "gcm"))
def test_no_file_among_the_entries(pna, pf, gpu_ctx, mode):
    """All 12 entries are directories and links: no segment, so no codec, write or framing launch -- the archive is the oracle's records"""
    entries = tc.entries_nonfiles12()
    cipher = _cipher(pna, mode, len(entries))
    for mcs in (0, 1000):
        if mode == "gcm" and mcs:
            continue
        want, offs = tc.expected_archive(pna, pf, gpu_ctx, entries, 2, 3, cipher, None, None, mcs)
        assert want == pf.write_archive_header(0) + b"".join(tc.nonfile_record(pf, k, n, d, max_chunk_size=mcs) for k, n, d in entries) + pf.finalize_archive()
        _both_forms_equal(pna, gpu_ctx, entries, want, offs, 2, 3, cipher=cipher, mcs=mcs)
        _both_forms_equal(pna, gpu_ctx, entries, want, offs, 1, 6, cipher=cipher, mcs=mcs)


@pytest.mark.parametrize("codec_name", ("zstd3", "deflate6"))
def test_many_entries_cross_the_layout_workgroups(pna, pf, codec, gpu_ctx, codec_name):
    """2 500 entries, every third a 100-byte file: k_layout scans 1 024 entries per workgroup, k_frame_wave frames the small payloads"""
    algo, level = CODECS[codec_name]
    entries = _lists(codec, "2500")
    want, offs = tc.expected_archive(pna, pf, gpu_ctx, entries, algo, level)
    _both_forms_equal(pna, gpu_ctx, entries, want, offs, algo, level)


def test_sub_batch_edges(pna, pf, codec, gpu_ctx):
    """The host form with the smallest sub-batches (sub_mib = 16).  The cutter counts input bytes, and an entry that is not a file has none: such an entry
    joins the open sub-batch unless that one is already over its size, which only a file larger than the sub-batch brings about.  So the edges that can be
    reached are: a sub-batch that ENDS in a run of directories and links and is followed by files (15 files of 1 MiB + 1 fill one), a sub-batch that STARTS
    with such a run (behind a 17 MiB file), and a sub-batch of nothing else (between two 17 MiB files)."""
    one = codec.corpus_file(0, 7300, (1 << 20) + 1)
    big = (codec.corpus_file(1, 7301, 1 << 20) * 17)[:(17 << 20) + 5]
    run = [(tc.DIR, "s/d0", b""), (tc.SYMLINK, "s/l0", b"f0"), (tc.HARDLINK, "s/h0", b"s/f1"), (tc.DIR, "s/d1", b"")]
    a = [(tc.DIR, "s", b"")] + [(tc.FILE, f"s/f{i}", one) for i in range(15)] + run + [(tc.FILE, f"s/g{i}", one) for i in range(3)] + [(tc.DIR, "s/end", b"")]
    b = [(tc.FILE, "t/big0", big)] + [(k, "t/" + n, d) for k, n, d in run] + [(tc.FILE, "t/big1", big), (tc.SYMLINK, "t/l", b"big0"), (tc.FILE, "t/f", one), (tc.DIR, "t/end", b"")]
    for entries in (a, b):
        with gpu_ctx.options(sub_mib=(16, 256)):
            want, offs = tc.expected_archive(pna, pf, gpu_ctx, entries, 1, 6)
            assert _host_form(pna, gpu_ctx, entries, 1, 6) == want
            got, eoff = _device_form(pna, gpu_ctx, entries, 1, 6)
        assert got == want and eoff == offs


@pytest.mark.parametrize("codec_name", ("zstd3", "deflate6"))
def test_without_kinds_the_counterparts_bytes(pna, pf, codec, gpu_ctx, codec_name):
    """kinds == NULL (and a kind array of files only): byte-equal to create_archive_chunked_host / _device"""
    import torch
    algo, level = CODECS[codec_name]
    files = [e for e in _lists(codec, "12") if e[0] == tc.FILE]
    names, datas, kinds, links = tc.tree_args(files)
    for mode, mcs in ((None, 0), (None, 1000), ("ctr", 1000)):
        cipher = _cipher(pna, mode, len(files))
        want = pna.create_archive_chunked(gpu_ctx, names, datas, mcs, algo=algo, level=level, cipher=cipher)
        assert pna.create_archive_tree(gpu_ctx, names, datas, None, None, algo=algo, level=level, cipher=cipher, max_chunk_size=mcs) == want
        assert pna.create_archive_tree(gpu_ctx, names, datas, kinds, None, algo=algo, level=level, cipher=cipher, max_chunk_size=mcs) == want
        src, offs = _upload(files)
        lens = [len(d) for d in datas]
        cap = pna.archive_chunked_bound(algo, names, lens, mcs, cipher)
        dst = torch.zeros(cap + 64, dtype=torch.uint8, device="cuda")
        total, eoff = gpu_ctx.create_archive_chunked_device(names, src.data_ptr(), offs, lens, dst.data_ptr(), cap, mcs, algo=algo, level=level, cipher=cipher)
        dev_want = dst[:total].cpu().numpy().tobytes()
        got, geoff = _device_form(pna, gpu_ctx, files, algo, level, cipher=cipher, mcs=mcs, kinds_none=True)
        assert got == dev_want and geoff == eoff


@pytest.mark.parametrize("mode", (None, "ctr"))
def test_round_trip_through_the_read_side(pna, pf, codec, gpu_ctx, mode):
    """extract, verify, the oracle's reader and diff see what went in: (kind, name, data) of every entry"""
    entries = _lists(codec, "12")
    cipher = _cipher(pna, mode, len(entries))
    password = b"password" if mode else None
    arc = _host_form(pna, gpu_ctx, entries, 2, 3, cipher=cipher)
    want = [(pf.sanitize_name(n), k, d) for k, n, d in entries]
    assert pna.extract_archive(gpu_ctx, arc, password) == want
    recs, summ = pna.verify_archive(gpu_ctx, arc, password)
    assert [(r[0], r[1], r[2]) for r in recs] == [(n, k, pna.VERIFY_OK) for n, k, _d in want]
    assert summ["ok"] == len(entries) and summ["failed"] == 0 and summ["rc"] == 0
    key = _key(pna)[0]
    for it, (n, k, d) in zip(pf.read_archive(arc)[1], want):
        assert (it.name, it.kind) == (n, k)
        if k != tc.FILE:
            assert it.data == d
        else:
            payload = codec.decrypt_payload(1, 1, key, it.data) if mode else it.data
            assert codec.decode_payload(2, payload, len(d) + 64) == d
    by_name = {n: (k, d) for n, k, d in want}

    def source(_idx, path, _kind, _stored):
        k, d = by_name[path]
        if k == tc.FILE:
            return pna.DIFF_FS_FILE, d
        if k == tc.DIR:
            return pna.DIFF_FS_DIR, None
        if k == tc.SYMLINK:
            return pna.DIFF_FS_SYMLINK, d                           # read_link reports the same target
        return pna.DIFF_FS_FILE, by_name[d.decode()][1]             # a hard link's path is a file on the host
    drecs, dsumm = pna.diff_archive(gpu_ctx, arc, source, password)
    status = {tc.FILE: pna.DIFF_SAME, tc.SYMLINK: pna.DIFF_SAME, tc.DIR: pna.DIFF_NOT_COMPARED, tc.HARDLINK: pna.DIFF_NOT_COMPARED}
    assert [(r.name, r.kind, r.status) for r in drecs] == [(n, k, status[k]) for n, k, _d in want]
    assert [r.link_target for r in drecs if r.kind == tc.HARDLINK] == [d for _n, k, d in want if k == tc.HARDLINK]
    assert dsumm["differ"] == 0 and dsumm["damaged"] == 0


def _straddle_list(pf, codec):
    """a list whose 2 500-byte link record lies across the 1 MiB edge of the inner stream (the first window's end at solid_win_mib = 1), with a directory record
    across the 2 MiB edge behind it"""
    def sized(head, name, seed, end):                                # the file behind `head` whose record ends at stream position `end`
        ln = end - len(tc.inner_stream(pf, head)) - 60
        for _ in range(8):
            at = len(tc.inner_stream(pf, head + [(tc.FILE, name, bytes(ln))]))
            if at == end:
                return (tc.FILE, name, codec.corpus_file(0, seed, ln))
            ln += end - at
        raise AssertionError("no length fits")
    out = [(tc.DIR, "w", b"")]
    out.append(sized(out, "w/first", 7401, (1 << 20) - 1000))
    out.append((tc.SYMLINK, "w/far", (b"../" * 833 + b"y")[:2500]))
    assert len(tc.inner_stream(pf, out[:2])) < (1 << 20) < len(tc.inner_stream(pf, out))
    out.append(sized(out, "w/second", 7402, (2 << 20) - 9))
    out.append((tc.DIR, "w/a-directory-whose-record-lies-across-the-edge", b""))
    assert len(tc.inner_stream(pf, out[:4])) < (2 << 20) < len(tc.inner_stream(pf, out))
    return out + [(tc.HARDLINK, "w/h", b"w/first"), (tc.FILE, "w/tail", codec.corpus_file(1, 7403, 3000)), (tc.DIR, "w/z", b"")]


@pytest.mark.parametrize("codec_name", ("zstd3", "deflate6"))
@pytest.mark.parametrize("mode", (None, "ctr"))
@pytest.mark.parametrize("which", ("12", "2500", "straddle", "12-meta-mcs1000"))
def test_solid_archives(pna, pf, codec, gpu_ctx, codec_name, mode, which):
    """`pna create --solid` of a tree: the records that are not files' stand between the file records of the inner stream.  The device form against the oracle
    (the SDAT stream, decrypted and decoded, is the oracle's serialisation), the host form in windows of 1 MiB -- a record across a window edge -- against
    the device form, and extract reports the kinds."""
    algo, level = CODECS[codec_name]
    entries = _memo(("list", "straddle"), lambda: _straddle_list(pf, codec)) if which == "straddle" else _lists(codec, which.split("-")[0])
    extra, facets = tc.facet_blobs(pf, entries) if "meta" in which else (None, None)
    mcs = 1000 if "mcs1000" in which else 0
    cipher = None
    if mode:
        key, phsf = _key(pna)
        cipher = pna.Cipher(key, phsf, pna.MODE_CTR, ivs=bytes(range(100, 116)))
    dev, _ = _device_form(pna, gpu_ctx, entries, algo, level, cipher=cipher, extra=extra, facets=facets, mcs=mcs, solid=True)
    plain = tc.inner_stream(pf, entries, extra, facets, mcs)
    (so,) = pf.read_archive(dev)[1]
    assert (so.compression, so.encryption) == (algo, 1 if mode else 0)
    comp = codec.decrypt_payload(1, 1, _key(pna)[0], so.data) if mode else so.data
    got_plain = codec.decode_payload(algo, comp, len(plain) + 4096)
    assert got_plain == plain
    assert [(e.kind, e.name, e.data) for e in pf.read_solid_inner(got_plain)] == [(k, pf.sanitize_name(n), d) for k, n, d in entries]
    with gpu_ctx.options(solid_win_mib=(1, 256)):
        host = _host_form(pna, gpu_ctx, entries, algo, level, cipher=cipher, extra=extra, facets=facets, mcs=mcs, solid=True)
    assert host == dev
    assert pna.extract_archive(gpu_ctx, host, b"password" if mode else None) == [(pf.sanitize_name(n), k, d) for k, n, d in entries]
