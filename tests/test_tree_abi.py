"""Entry kinds on the create paths, the part that needs no device: the new symbols, the bounds, the argument checks, and the builder of the records that
are not files' (directory, symbolic link, hard link) against the oracle's writer.

The reference: create_entry's four arms (cli/src/command/core.rs:915-977), EntryHeader::for_dir / for_symlink / for_hard_link (lib/src/entry/header.rs:65-78),
new_link over WriteOptions::store() (lib/src/entry/builder.rs:341-349), no fSIZ unless DataKind::FILE (builder.rs:630-632)."""
import ctypes

import pytest

import tree_cases as tc

NEW_SYMBOLS = ("pna_gpu_create_archive_tree_device", "pna_gpu_create_archive_tree_host", "pna_gpu_archive_tree_bound",
               "pna_gpu_create_solid_archive_tree_device", "pna_gpu_create_solid_archive_tree_host", "pna_gpu_solid_archive_tree_bound",
               "pna_gpu_entry_kinds_check", "pna_archive_entry_record_bytes")


def test_library_exports_the_tree_symbols(pna):
    L = pna.load_library()
    for name in NEW_SYMBOLS:
        assert hasattr(L, name), name
        assert name in pna.EXPORTS, name
    assert (pna.KIND_FILE, pna.KIND_DIRECTORY, pna.KIND_SYMLINK, pna.KIND_HARDLINK) == (0, 1, 2, 3)


def _lists(codec):
    return {"12": tc.entries12(codec), "nonfiles": tc.entries_nonfiles12(), "2500": tc.entries2500(codec)}


@pytest.mark.parametrize("which", ("12", "nonfiles", "2500"))
@pytest.mark.parametrize("mcs", (0, 1000))
@pytest.mark.parametrize("with_meta", (False, True))
def test_bounds_hold_the_oracles_archive(pna, pf, codec, which, mcs, with_meta):
    """The bound is at least the size of the archive whose payloads are as long as a stream may get (pna_gpu_bound) and whose other records are the oracle's."""
    entries = _lists(codec)[which]
    names, datas, kinds, links = tc.tree_args(entries)
    extra, facets = tc.facet_blobs(pf, entries) if with_meta else (None, None)
    for algo in (pna.ALGO_ZSTD, pna.ALGO_DEFLATE):
        size = len(pf.write_archive_header(0)) + len(pf.finalize_archive())
        for i, (k, name, data) in enumerate(entries):
            ex, fa = (extra[i], facets[i]) if with_meta else (b"", b"")
            if k == tc.FILE:
                worst = bytes(pna.bound(algo, len(data)))
                pieces = pf.flatten_writer([worst], mcs if mcs else pf.MAX_CHUNK_DATA_LENGTH) or [b""]
                size += len(pf.write_normal_entry(pf.file_entry_header(algo, pf.sanitize_name(name)), pieces, len(data), tc.blob_chunks(pf, ex), tc.blob_chunks(pf, fa)))
            else:
                size += len(tc.nonfile_record(pf, k, name, data, ex, fa, mcs))
        b = pna.archive_tree_bound(algo, names, [len(d) for d in datas], kinds, links, facets=facets, extra=extra, max_chunk_size=mcs)
        assert b >= size, (algo, b, size)
        # solid: one stream of stored records, compressed as one entry, an SDAT chunk per MiB of it
        plain = len(tc.inner_stream(pf, entries, extra, facets, mcs))
        solid = len(pf.write_archive_header(0)) + 17 + pna.bound(algo, plain) + 12 * (plain // (1 << 20) + 1) + 12 + 12
        sb = pna.solid_archive_tree_bound(algo, names, [len(d) for d in datas], kinds, links, facets=facets, extra=extra, max_chunk_size=mcs)
        assert sb >= solid, (algo, sb, solid)
    # without kinds the bounds are the counterparts' (plus nothing: no blobs, no links)
    lens = [len(d) for d in datas]
    if not with_meta:
        assert pna.archive_tree_bound(pna.ALGO_ZSTD, names, lens, None, None, max_chunk_size=mcs) == pna.archive_chunked_bound(pna.ALGO_ZSTD, names, lens, mcs)
    if not with_meta and not mcs:
        assert pna.solid_archive_tree_bound(pna.ALGO_ZSTD, names, lens, None, None) == pna.solid_archive_enc_bound(pna.ALGO_ZSTD, names, lens, None)


def test_argument_errors_need_no_device(pna):
    E = pna.E_INVAL
    ok_len, kinds, links = [0, 5, 0, 0], [tc.DIR, tc.FILE, tc.SYMLINK, tc.HARDLINK], [None, None, b"to", b"from"]
    assert pna.entry_kinds_check(ok_len, kinds, links) == 0
    assert pna.entry_kinds_check(ok_len, None, None) == 0                                   # all files
    assert pna.entry_kinds_check(ok_len, [tc.DIR, tc.FILE, 4, tc.HARDLINK], links) == E     # unknown kind
    assert pna.entry_kinds_check(ok_len, [tc.DIR, tc.FILE, 255, tc.HARDLINK], links) == E
    assert pna.entry_kinds_check([1, 5, 0, 0], kinds, links) == E                           # a directory with source bytes
    assert pna.entry_kinds_check([0, 5, 0, 7], kinds, links) == E                           # a link with source bytes
    assert pna.entry_kinds_check(ok_len, kinds, [None, None, b"", b"from"]) == E            # an empty target
    assert pna.entry_kinds_check(ok_len, kinds, [None, None, b"to", None]) == E
    assert pna.entry_kinds_check(ok_len, kinds, None) == E                                  # link == NULL with a link kind present
    assert pna.entry_kinds_check([0, 5], [tc.DIR, tc.FILE], None) == 0                      # ... and without one: fine
    # the entry points themselves answer the same before they touch a device (no context here: every call is refused, none may crash)
    L = pna.load_library()
    vp = ctypes.c_void_p
    f = L.pna_gpu_create_archive_tree_host
    f.argtypes = [vp, ctypes.c_int, ctypes.c_int, ctypes.c_size_t, vp, vp, vp, vp, vp, ctypes.c_uint32, vp, ctypes.c_uint32, pna.SINK_FN, vp]
    ks, _keep = pna._kinds_struct(1, [9], None)
    names = (ctypes.c_char_p * 1)(b"x")
    src = (vp * 1)(None)
    lens = (ctypes.c_size_t * 1)(0)
    cb = pna.SINK_FN(lambda *_a: 0)
    assert f(None, pna.ALGO_ZSTD, 3, 1, names, src, lens, None, None, 0, ctypes.byref(ks), 3, cb, None) == E
    with pytest.raises(ValueError):
        pna.entry_record_bytes(tc.SYMLINK, "l", b"")
    with pytest.raises(ValueError):
        pna.entry_record_bytes(tc.FILE, "f", b"x")
    with pytest.raises(ValueError):
        pna.entry_record_bytes(4, "f", b"x")


@pytest.mark.parametrize("kind", (tc.DIR, tc.SYMLINK, tc.HARDLINK))
@pytest.mark.parametrize("with_meta", (False, True))
@pytest.mark.parametrize("mcs", (0, 1000, 2500, 2499))
def test_record_builder_equals_the_oracle(pna, pf, kind, with_meta, mcs):
    target = b"" if kind == tc.DIR else bytes((i * 7 + 3) & 255 for i in range(2500))
    extra = pf.write_chunk(b"usRc", b"first") if with_meta else b""
    facets = pf.write_chunk(b"mTIM", (1700000000).to_bytes(8, "big")) + pf.write_chunk(b"fPRM", b"\x01\xa4") if with_meta else b""
    for name in ("plain", "a/./b/../c/", "/rooted/x"):
        got = pna.entry_record_bytes(kind, name, target, extra, facets, mcs)
        assert got == tc.nonfile_record(pf, kind, name, target, extra, facets, mcs)
        (ent,) = pf.read_solid_inner(got)                                                  # one record: FHED .. FEND, every CRC right
        assert (ent.kind, ent.name, ent.data, ent.raw_file_size) == (kind, pf.sanitize_name(name), target, None)
        assert (ent.compression, ent.encryption, ent.cipher_mode) == (0, 0, 0)
        if kind != tc.DIR and mcs == 1000:
            assert [len(d) for t, d in ent.chunks if t == b"FDAT"] == [1000, 1000, 500]


def test_add_dir_writes_the_builders_record(pna, pf):
    """pna_archive_add_dir goes through the one record builder: its bytes are the directory record without metadata"""
    import io
    sink = io.BytesIO()
    a = pna.Archive(sink)
    a.add_dir("some/./dir/")
    a.finalize()
    out = sink.getvalue()
    want = pf.write_archive_header(0) + tc.nonfile_record(pf, tc.DIR, "some/./dir/", b"") + pf.finalize_archive()
    assert bytes(out) == want
    assert pna.entry_record_bytes(tc.DIR, "some/./dir/") == want[len(pf.write_archive_header(0)):-len(pf.finalize_archive())]
