"""Entry lists and expected bytes for the tree create paths (entry kinds: directories, symbolic links, hard links between the files).

The expected bytes never come from the code under test: a file's record is cut out of the archive that the existing
pna_gpu_create_archive_chunked_host writes for the files alone (same context options, same IVs), a record that is not a file's is the oracle's
write_normal_entry over dir_entry_header / entry_header_bytes(kind, 0, 0, 0, ..) with the target cut by flatten_writer."""
import ctypes

FILE, DIR, SYMLINK, HARDLINK = 0, 1, 2, 3


def entries12(codec):
    """The 12-entry list: (kind, name, bytes) -- a file's data, a link's target, b"" for a directory.  First and last are directories."""
    return [
        (DIR, "tree", b""),
        (FILE, "tree/empty", b""),
        (FILE, "tree/one", b"x"),
        (SYMLINK, "tree/link", b"one"),
        (FILE, "tree/big.txt", codec.corpus_file(0, 7101, (1 << 20) + 1)),
        (DIR, "tree/a", b""),
        (DIR, "tree/a/./b/", b""),                                       # (sanitised like a file's name: tree/a/b)
        (HARDLINK, "tree/a/hard", b"tree/big.txt"),
        (FILE, "tree/a/page", codec.corpus_file(1, 7102, 4096)),
        (FILE, "tree/a/mid.bin", codec.corpus_file(2, 7103, 70000)),
        (SYMLINK, "tree/a/far", (b"../" * 833 + b"x")[:2500]),           # a 2 500-byte target: three FDAT chunks at max_chunk_size 1 000
        (DIR, "tree/z", b""),
    ]


def entries_nonfiles12():
    """12 entries, not one file among them"""
    out = []
    for i in range(12):
        k = (DIR, SYMLINK, HARDLINK)[i % 3]
        out.append((k, f"only/{i}", b"" if k == DIR else (b"target-%d/" % i) * (1 + 40 * (i % 4))))
    return out


def entries2500(codec):
    """2 500 entries: i % 3 == 0 a 100-byte file, the rest alternate directory / symbolic link (crosses k_layout's 1 024-entry workgroups, k_frame_wave)"""
    text = codec.corpus_file(0, 7200, 100 * 834)
    out, flip = [], 0
    for i in range(2500):
        if i % 3 == 0:
            out.append((FILE, f"m/{i:04d}.txt", text[100 * (i // 3):100 * (i // 3) + 100]))
        else:
            out.append((DIR, f"m/d{i:04d}", b"") if flip == 0 else (SYMLINK, f"m/l{i:04d}", b"%04d.txt" % (i - i % 3)))
            flip ^= 1
    return out


def facet_blobs(pf, entries):
    """(extra, facets) for every entry, files and others alike: one user chunk in front, two metadata chunks behind (already framed, as the ABI takes them)"""
    extra = [pf.write_chunk(b"usRc", b"e%d" % i) for i in range(len(entries))]
    facets = [pf.write_chunk(b"mTIM", (1700000000 + i).to_bytes(8, "big")) + pf.write_chunk(b"fPRM", b"\x01\xa4" + bytes([i & 255])) for i in range(len(entries))]
    return extra, facets


def blob_chunks(pf, blob):
    return [(ty, d) for ty, d, _ in pf.read_chunks(blob, 0)]


def nonfile_record(pf, kind, name, target, extra=b"", facets=b"", max_chunk_size=0):
    """the oracle's record of a directory or link: FHED(kind, 0, 0, 0) | extra | facets | FDAT* | FEND, no fSIZ"""
    header = pf.dir_entry_header(pf.sanitize_name(name)) if kind == DIR else pf.entry_header_bytes(kind, 0, 0, 0, pf.sanitize_name(name))
    pieces = [] if kind == DIR else pf.flatten_writer([target], max_chunk_size if max_chunk_size else pf.MAX_CHUNK_DATA_LENGTH)
    return pf.write_normal_entry(header, pieces, None, blob_chunks(pf, extra), blob_chunks(pf, facets))


def split_records(pf, archive):
    """the entry records of a non-solid archive, in order: [FHED .. FEND] byte strings"""
    out, start = [], 8 + 20
    for ty, _d, pos in pf.read_chunks(archive, 8):
        if ty == b"AHED":
            start = pos
        elif ty == b"FEND":
            out.append(archive[start:pos]); start = pos
    return out


def files_only_archive(pna, ctx, names, datas, algo, level, cipher, extra, facets, max_chunk_size):
    """pna_gpu_create_archive_chunked_host over the files alone, with their metadata blobs: the existing entry point the file records are cut from"""
    L = pna.load_library()
    n = len(datas)
    out = bytearray()

    def _sink(_u, buf, k):
        out.extend((ctypes.c_char * k).from_address(buf))
        return 0
    cb = pna.SINK_FN(_sink)
    a_names = (ctypes.c_char_p * max(n, 1))(*[s.encode() for s in names])
    a_src = (ctypes.c_void_p * max(n, 1))(*[ctypes.cast(ctypes.c_char_p(b), ctypes.c_void_p) for b in datas])
    a_len = (ctypes.c_size_t * max(n, 1))(*[len(b) for b in datas])
    ms, keep = None, []
    if extra is not None:
        ms = pna.MetaStruct()
        for field, blobs in (("extra", extra), ("facets", facets)):
            arr = (ctypes.c_void_p * max(n, 1))(*[ctypes.cast(ctypes.c_char_p(b), ctypes.c_void_p) for b in blobs])
            lens = (ctypes.c_size_t * max(n, 1))(*[len(b) for b in blobs])
            keep += [arr, lens]
            setattr(ms, field, ctypes.cast(arr, ctypes.POINTER(ctypes.c_void_p)))
            setattr(ms, field + "_len", ctypes.cast(lens, ctypes.POINTER(ctypes.c_size_t)))
    cs = cipher.struct(n) if cipher is not None else None
    f = L.pna_gpu_create_archive_chunked_host
    f.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                  ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, pna.SINK_FN, ctypes.c_void_p]
    rc = f(ctx._h, algo, level, n, a_names, a_src, a_len, ctypes.byref(cs) if cs is not None else None, ctypes.byref(ms) if ms is not None else None,
           max_chunk_size, pna.PART_HEAD | pna.PART_TAIL, cb, None)
    assert rc == 0, (rc, L.pna_gpu_last_error(ctx._h))
    return bytes(out)


def file_cipher(pna, cipher, file_idx, iv_len):
    """the cipher of the files-only call: the same key, the IV slots of the files"""
    if cipher is None:
        return None
    ivs = b"".join(cipher.ivs[iv_len * i:iv_len * i + iv_len] for i in file_idx)
    return pna.Cipher(cipher.key, cipher.phsf, cipher.mode, cipher.encryption, ivs=ivs or bytes(iv_len), gcm_segment_size=cipher.gcm_segment_size)


def expected_archive(pna, pf, ctx, entries, algo, level, cipher=None, extra=None, facets=None, max_chunk_size=0):
    """archive header + records in order + AEND; returns (archive, [offset of every record])"""
    file_idx = [i for i, (k, _n, _d) in enumerate(entries) if k == FILE]
    iv_len = 39 if cipher is not None and cipher.mode == pna.MODE_GCM else 16
    recs = []
    if file_idx:
        arc = files_only_archive(pna, ctx, [entries[i][1] for i in file_idx], [entries[i][2] for i in file_idx], algo, level,
                                 file_cipher(pna, cipher, file_idx, iv_len), None if extra is None else [extra[i] for i in file_idx],
                                 None if facets is None else [facets[i] for i in file_idx], max_chunk_size)
        recs = split_records(pf, arc)
        assert len(recs) == len(file_idx)
    recs = iter(recs)
    out, offs = bytearray(pf.write_archive_header(0)), []
    for i, (k, name, data) in enumerate(entries):
        offs.append(len(out))
        out += next(recs) if k == FILE else nonfile_record(pf, k, name, data, b"" if extra is None else extra[i], b"" if facets is None else facets[i], max_chunk_size)
    offs.append(len(out))
    out += pf.finalize_archive()
    return bytes(out), offs


def tree_args(entries):
    """(names, file bytes per entry, kinds, link targets per entry) as the tree entry points take them"""
    names = [n for _k, n, _d in entries]
    datas = [d if k == FILE else b"" for k, _n, d in entries]
    kinds = [k for k, _n, _d in entries]
    links = [d if k in (SYMLINK, HARDLINK) else None for k, _n, d in entries]
    return names, datas, kinds, links


def inner_stream(pf, entries, extra=None, facets=None, max_chunk_size=0):
    """the oracle's serialisation of a solid archive's inner stream: stored records, the files' among them (FHED | extra | fSIZ | facets | FDAT* | FEND)"""
    out = bytearray()
    mx = max_chunk_size if max_chunk_size else pf.MAX_CHUNK_DATA_LENGTH
    for i, (k, name, data) in enumerate(entries):
        ex, fa = (b"" if extra is None else extra[i]), (b"" if facets is None else facets[i])
        if k == FILE:
            out += pf.write_normal_entry(pf.file_entry_header(0, pf.sanitize_name(name)), pf.flatten_writer([data], mx), len(data), blob_chunks(pf, ex), blob_chunks(pf, fa))
        else:
            out += nonfile_record(pf, k, name, data, ex, fa, max_chunk_size)
    return bytes(out)
