"""`pna create --store` on the device: PNA_ALGO_STORE through the non-solid archive entry points (k_store.hip: k_store's fused copy + CRC and k_store_fold;
under a cipher k_store's copy-only form, the cipher stage and k_frame).

Every case: the bytes equal tests/store_cases.py's expectation (the oracle's records, the oracle's cipher layer, fixed IVs), entry_off -- where the entry
point has it -- equals the expectation's FHED offsets, extract_archive returns the inputs and verify_archive finds every entry in order.
pna_gpu_debug_store_stats shows which form of k_store ran.  Before the feature every call here answered PNA_E_UNSUPPORTED."""
import pytest

import store_cases as sc

pytestmark = pytest.mark.gpu

_cache = {}


def _memo(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def _key(pna):
    return _memo("key", lambda: pna.kdf_pbkdf2_sha256(b"password", bytes(range(16)), 1000))


def _cfg(pna, mode, n, encryption=1, seg=0):
    if mode is None:
        return None
    key, phsf = _key(pna)
    return sc.CipherCfg(key, phsf, mode, n, encryption, seg)


def _want(pf, codec, key, ents, **kw):
    return _memo(("want", key), lambda: sc.expected_archive(pf, codec, ents, **kw))


def _upload(datas, guard=0):
    """the entries in one device buffer at 16-byte aligned offsets"""
    import torch
    offs, pos = [], 0
    for d in datas:
        offs.append(pos)
        pos = (pos + len(d) + 15) & ~15
    host = bytearray(pos + 64)
    for o, d in zip(offs, datas):
        host[o:o + len(d)] = d
    return torch.frombuffer(host, dtype=torch.uint8).cuda(), offs


def _device(pna, ctx, ents, cfg=None, mcs=0, extra=None, facets=None, kinds=None, links=None, part=None):
    """pna_gpu_create_archive_tree_device (the entry point that takes everything): (bytes, entry_off)"""
    import torch
    names, datas = [n for n, _d in ents], [d for _n, d in ents]
    lens = [len(d) for d in datas]
    src, offs = _upload(datas)
    cipher = None if cfg is None else cfg.product(pna)
    cap = pna.archive_tree_bound(pna.ALGO_STORE, names, lens, kinds, links, cipher=cipher, facets=facets, extra=extra, max_chunk_size=mcs)
    dst = torch.zeros(cap + 64, dtype=torch.uint8, device="cuda")
    total, eoff = ctx.create_archive_tree_device(names, src.data_ptr(), offs, lens, dst.data_ptr(), cap, kinds, links, algo=pna.ALGO_STORE, level=7, cipher=cipher,
                                                 facets=facets, extra=extra, max_chunk_size=mcs, **({} if part is None else {"part": part}))
    assert total <= cap
    return dst[:total].cpu().numpy().tobytes(), eoff


def _host(pna, ctx, ents, cfg=None, mcs=0, extra=None, facets=None, kinds=None, links=None, part=None):
    """pna_gpu_create_archive_tree_host"""
    return pna.create_archive_tree(ctx, [n for n, _d in ents], [d for _n, d in ents], kinds, links, algo=pna.ALGO_STORE, cipher=None if cfg is None else cfg.product(pna),
                                   facets=facets, extra=extra, max_chunk_size=mcs, **({} if part is None else {"part": part}))


def _reads_back(pna, ctx, archive, ents, kinds=None, password=None):
    """extract_archive returns the inputs; verify_archive names every entry and finds it in order"""
    got = pna.extract_archive(ctx, archive, password)
    assert [g[2] for g in got] == [d if (kinds is None or kinds[i] == sc.FILE) else g[2] for i, ((_n, d), g) in enumerate(zip(ents, got))]
    assert len(got) == len(ents)
    recs, summ = pna.verify_archive(ctx, archive, password)
    assert summ["rc"] == 0 and len(recs) == len(ents)
    assert all(r[2] == pna.VERIFY_OK for r in recs), [r for r in recs if r[2] != pna.VERIFY_OK][:3]


def test_sizes_plain_both_forms(pna, pf, codec, gpu_ctx):
    """The size list (an empty entry, k_store's table-free form, one tile, the 16 380-byte edge, one piece, a piece edge, three-plus pieces) at destination
    offsets of every residue mod 16, through pna_gpu_create_archive_device, the tree entry point and the host form; the fused form runs"""
    import torch
    ents = sc.entry_list()
    want, offs, nchunks, pay = _want(pf, codec, "plain", ents)
    assert {p % 16 for p in pay} == set(range(16))
    names, datas = [n for n, _d in ents], [d for _n, d in ents]
    src, soff = _upload(datas)
    cap = pna.archive_bound(pna.ALGO_STORE, names, [len(d) for d in datas])
    dst = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    total, eoff = gpu_ctx.create_archive_device(names, src.data_ptr(), soff, [len(d) for d in datas], dst.data_ptr(), cap, algo=pna.ALGO_STORE)
    got = dst[:total].cpu().numpy().tobytes()
    assert got == want and eoff == offs
    fused, copy_only, folded, _ms = pna.store_stats(gpu_ctx)
    assert fused > 0 and copy_only == 0 and folded == nchunks
    assert fused == sum((len(d) + sc.MIB - 1) // sc.MIB for d in datas)
    assert src.cpu().numpy().tobytes()[:soff[-1] + len(datas[-1])] == b"".join(d + bytes(-len(d) % 16) for d in datas)[:soff[-1] + len(datas[-1])]
    got, eoff = _device(pna, gpu_ctx, ents)
    assert got == want and eoff == offs
    assert _host(pna, gpu_ctx, ents) == want
    fused, copy_only, folded, _ms = pna.store_stats(gpu_ctx)
    assert fused > 0 and copy_only == 0 and folded == nchunks
    _reads_back(pna, gpu_ctx, want, ents)
    assert pna.create_archive(None, names, datas, algo=pna.ALGO_STORE) == want      # the host loop, which stays


def test_chunks_of_more_than_64_pieces(pna, pf, gpu_ctx):
    """One chunk of 65 MiB + 5 and one of 129 MiB - 16: more pieces than k_store_fold has lanes, the last one short -- a lane's Horner sum must leave the
    chunk's last piece out (crc_core.h crc_fold_lane).  The FDAT CRC fields are compared with zlib.crc32, verify_archive reads the archive; the stored
    solid stream with the first entry folds the same way."""
    import zlib
    import numpy as np
    import torch
    sizes = [(65 << 20) + 5, (129 << 20) - 16]
    datas = [np.random.RandomState(77 + i).bytes(n) for i, n in enumerate(sizes)]
    names = ["big/a.bin", "big/b"]
    src, soff = _upload(datas)
    cap = pna.archive_bound(pna.ALGO_STORE, names, sizes)
    dst = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    total, eoff = gpu_ctx.create_archive_device(names, src.data_ptr(), soff, sizes, dst.data_ptr(), cap, algo=pna.ALGO_STORE)
    assert pna.store_stats(gpu_ctx)[:3] == (65 + 1 + 129, 0, 2)
    for i, d in enumerate(datas):
        end = eoff[i + 1]                                          # the record ends in CRC(4) | FEND(12)
        tail = dst[end - 16 - len(d) - 8:end].cpu().numpy().tobytes()
        assert tail[:8] == len(d).to_bytes(4, "big") + b"FDAT" and tail[8:8 + 64] == d[:64] and tail[-12:] == pf.write_chunk(b"FEND")
        assert int.from_bytes(tail[-16:-12], "big") == zlib.crc32(d, zlib.crc32(b"FDAT")), i
    arc = dst[:total].cpu().numpy().tobytes()
    recs, summ = pna.verify_archive(gpu_ctx, arc)
    assert summ["rc"] == 0 and [r[2] for r in recs] == [pna.VERIFY_OK] * 2
    del arc
    cap = pna.solid_archive_bound(pna.ALGO_STORE, names[:1], sizes[:1])
    total = gpu_ctx.create_solid_archive_device(names[:1], src.data_ptr(), soff[:1], sizes[:1], dst.data_ptr(), min(cap, dst.numel()), algo=pna.ALGO_STORE)
    recs, summ = pna.verify_archive(gpu_ctx, dst[:total].cpu().numpy().tobytes())
    assert summ["rc"] == 0 and [r[2] for r in recs] == [pna.VERIFY_OK]


def test_unfused_form_writes_the_same_bytes(pna, pf, codec, gpu_ctx):
    """option store_unfused: k_store's copy-only form and k_frame, the form the fused one is measured against"""
    ents = sc.entry_list()
    want, offs, _nc, _pay = _want(pf, codec, "plain", ents)
    with gpu_ctx.options(store_unfused=(1, -1)):
        got, eoff = _device(pna, gpu_ctx, ents)
        fused, copy_only, folded, _ms = pna.store_stats(gpu_ctx)
    assert got == want and eoff == offs and (fused, folded) == (0, 0) and copy_only > 0


@pytest.mark.parametrize("mcs", (5, 16, 17, 4096, 65537, sc.MIB - 1, sc.MIB + 1))
def test_max_chunk_size(pna, pf, codec, gpu_ctx, mcs):
    """Chunks start at any byte of their entry: the source side of k_store is unaligned too, a chunk may be a fraction of a piece (5, 16, 17: hundreds of
    chunks per entry, the entries up to 4 096 bytes) and an entry's pieces end with its chunks (4 096 .. 1 MiB + 1: all entries)"""
    ents = sc.entry_list(sc.SMALL_SIZES if mcs < 4096 else sc.SIZES)
    want, offs, nchunks, _pay = _want(pf, codec, ("mcs", mcs), ents, mcs=mcs)
    with gpu_ctx.options(store_unfused=(0, -1)):                 # the fused form whatever the chunks' size
        got, eoff = _device(pna, gpu_ctx, ents, mcs=mcs)
        assert got == want and eoff == offs
        assert pna.store_stats(gpu_ctx)[:3] == (sum((min(mcs, len(d) - o) + sc.MIB - 1) // sc.MIB for _n, d in ents for o in range(0, len(d), mcs)), 0, nchunks)
        assert _host(pna, gpu_ctx, ents, mcs=mcs) == want
    # the default picks the form by the sub-batch's longest chunk: fused above 1 MiB and up to 4 KiB, the copy-only form and k_frame between
    got, eoff = _device(pna, gpu_ctx, ents, mcs=mcs)
    assert got == want and eoff == offs
    fused, copy_only, folded, _ms = pna.store_stats(gpu_ctx)
    assert (fused > 0 and copy_only == 0 and folded == nchunks) if (mcs <= 4096 or mcs > sc.MIB) else (fused == 0 and folded == 0 and copy_only > 0)
    assert _host(pna, gpu_ctx, ents, mcs=mcs) == want
    _reads_back(pna, gpu_ctx, want, ents)


@pytest.mark.parametrize("mode,seg", (("ctr", 0), ("cbc", 0), ("gcm", 4096), ("gcm", 0)))
@pytest.mark.parametrize("with_meta", (False, True))
def test_aes(pna, pf, codec, gpu_ctx, mode, seg, with_meta):
    """AES-256 in CTR, CBC and GCM STREAM (segments of 4 096 bytes and the default) over the size list -- the empty entry and the 15 / 16 / 17-byte ones
    among them --, with and without metadata chunks: the copy-only form runs, the CRC is k_frame's over the ciphertext"""
    ents = sc.entry_list()
    cfg = _cfg(pna, mode, len(ents), 1, seg)
    extra, facets = sc.meta_blobs(pf, len(ents)) if with_meta else (None, None)
    want, offs, _nc, _pay = _want(pf, codec, ("aes", mode, seg, with_meta), ents, cfg=cfg, extra=extra, facets=facets)
    got, eoff = _device(pna, gpu_ctx, ents, cfg, extra=extra, facets=facets)
    assert got == want and eoff == offs
    fused, copy_only, folded, _ms = pna.store_stats(gpu_ctx)
    assert fused == 0 and folded == 0 and copy_only > 0
    assert _host(pna, gpu_ctx, ents, cfg, extra=extra, facets=facets) == want
    _reads_back(pna, gpu_ctx, want, ents, password=b"password")


def test_ctr_with_chunks(pna, pf, codec, gpu_ctx):
    """CTR may be cut anywhere: the keystream runs on over the chunks (max_chunk_size 65 537, all sizes)"""
    ents = sc.entry_list()
    cfg = _cfg(pna, "ctr", len(ents))
    want, offs, _nc, _pay = _want(pf, codec, "ctr-mcs", ents, cfg=cfg, mcs=65537)
    got, eoff = _device(pna, gpu_ctx, ents, cfg, mcs=65537)
    assert got == want and eoff == offs
    assert _host(pna, gpu_ctx, ents, cfg, mcs=65537) == want
    _reads_back(pna, gpu_ctx, want, ents, password=b"password")


@pytest.mark.parametrize("mode", ("ctr", "cbc", "gcm"))
def test_camellia(pna, pf, codec, gpu_ctx, mode):
    """The same three modes under Camellia-256 on a context with the option set; without it the answer is PNA_E_UNSUPPORTED as for every other algo"""
    ents = sc.entry_list(sc.CAMELLIA_SIZES)
    cfg = _cfg(pna, mode, len(ents), 2, 4096 if mode == "gcm" else 0)
    want, offs, _nc, _pay = _want(pf, codec, ("cam", mode), ents, cfg=cfg)
    with pytest.raises(pna.PnaGpuError) as ei:
        _device(pna, gpu_ctx, ents, cfg)
    assert ei.value.code == pna.E_UNSUPPORTED
    with gpu_ctx.options(camellia=(1, 0)):
        got, eoff = _device(pna, gpu_ctx, ents, cfg)
        assert got == want and eoff == offs
        assert _host(pna, gpu_ctx, ents, cfg) == want
        _reads_back(pna, gpu_ctx, want, ents, password=b"password")


def test_camellia_with_meta(pna, pf, codec, gpu_ctx):
    """Camellia-CTR with metadata chunks around fSIZ"""
    ents = sc.entry_list(sc.CAMELLIA_SIZES)
    cfg = _cfg(pna, "ctr", len(ents), 2)
    extra, facets = sc.meta_blobs(pf, len(ents))
    want, offs, _nc, _pay = _want(pf, codec, ("cam-meta",), ents, cfg=cfg, extra=extra, facets=facets)
    with gpu_ctx.options(camellia=(1, 0)):
        got, eoff = _device(pna, gpu_ctx, ents, cfg, extra=extra, facets=facets)
        assert got == want and eoff == offs
        assert _host(pna, gpu_ctx, ents, cfg, extra=extra, facets=facets) == want


def test_append(pna, pf, codec, gpu_ctx):
    """pna_gpu_append_archive_host reaches the part form unchanged: stored entries appended to a stored archive are the one-call archive"""
    ents = sc.entry_list()
    want, _offs, _nc, _pay = _want(pf, codec, "plain", ents)
    first = _host(pna, gpu_ctx, ents[:7])
    got = pna.append_archive(gpu_ctx, first, [n for n, _d in ents[7:]], [d for _n, d in ents[7:]], algo=pna.ALGO_STORE)
    assert got == want


def test_parts(pna, pf, codec, gpu_ctx):
    """PNA_PART_HEAD alone, neither, PNA_PART_TAIL alone: three shards concatenated are the one-call archive (device and host form)"""
    ents = sc.entry_list()
    want, _offs, _nc, _pay = _want(pf, codec, "plain", ents)
    cuts = ((0, 6, pna.PART_HEAD), (6, 16, 0), (16, len(ents), pna.PART_TAIL))
    assert b"".join(_device(pna, gpu_ctx, ents[a:b], part=p)[0] for a, b, p in cuts) == want
    assert b"".join(_host(pna, gpu_ctx, ents[a:b], part=p) for a, b, p in cuts) == want
    assert _device(pna, gpu_ctx, ents, part=pna.PART_HEAD | pna.PART_TAIL)[0] == want


@pytest.mark.parametrize("mode,mcs", ((None, 0), (None, 1000), ("ctr", 0), ("ctr", 1000), ("gcm", 0)))
def test_tree(pna, pf, codec, gpu_ctx, mode, mcs):
    """Directories, a symbolic link, a hard link and stored files; with a cipher the files are encrypted and the links stay in the clear.  (A GCM entry
    must fit one chunk, as on the compressed paths: no max_chunk_size there.)"""
    tree = sc.tree_entries()
    ents, kinds = [(n, d) for _k, n, d in tree], [k for k, _n, _d in tree]
    _names, datas, tkinds, links = sc.tc.tree_args(tree)
    cfg = _cfg(pna, mode, len(ents), 1, 65536)
    want, offs, _nc, _pay = _want(pf, codec, ("tree", mode, mcs), ents, mcs=mcs, cfg=cfg, kinds=kinds)
    fents = list(zip(_names, datas))
    got, eoff = _device(pna, gpu_ctx, fents, cfg, mcs=mcs, kinds=tkinds, links=links)
    assert got == want and eoff == offs
    assert _host(pna, gpu_ctx, fents, cfg, mcs=mcs, kinds=tkinds, links=links) == want
    got = pna.extract_archive(gpu_ctx, want, b"password" if mode else None)
    assert [(g[0], g[1]) for g in got] == [(pf.sanitize_name(n), k) for k, n, _d in tree]
    assert [g[2] for g, k in zip(got, kinds) if k == sc.FILE] == [d for k, _n, d in tree if k == sc.FILE]
    recs, summ = pna.verify_archive(gpu_ctx, want, b"password" if mode else None)
    assert summ["rc"] == 0 and all(r[2] == pna.VERIFY_OK for r in recs) and len(recs) == len(tree)


def test_several_sub_batches(pna, pf, codec, monkeypatch):
    """The host form with the sub-batch size at its smallest setting (PNA_SUB_MIB = 1 at init): entries beside a sub-batch's edge, the 3 MiB + 17 entry in
    a sub-batch of its own; the bytes are the default's"""
    import torch  # noqa: F401
    ents = sc.entry_list()
    want, _offs, nchunks, _pay = _want(pf, codec, "plain", ents)
    monkeypatch.setenv("PNA_SUB_MIB", "1")
    with pna.Context(0) as ctx:
        assert _host(pna, ctx, ents) == want                      # (the form by every sub-batch's longest chunk: some fused, some not)
        fused, copy_only, folded, _ms = pna.store_stats(ctx)
        assert fused > 0 and copy_only > 0 and 0 < folded < nchunks
        ctx.set_option("store_unfused", 0)
        assert _host(pna, ctx, ents) == want
        assert pna.store_stats(ctx)[1:3] == (0, nchunks)
        cfg = _cfg(pna, "ctr", len(ents))
        assert _host(pna, ctx, ents, cfg) == _want(pf, codec, ("aes", "ctr", 0, False), ents, cfg=cfg)[0]


def test_guard_bytes_and_capacity(pna, pf, codec, gpu_ctx):
    """The destination is a slice of a larger buffer filled with 0xA5: the bytes in front of it and behind its capacity stay untouched and the source is
    unchanged; a capacity one byte below the archive's length is PNA_E_DSTSIZE with the guards still untouched.  (The fused form takes a destination of
    exactly the archive's size.)"""
    import torch
    ents = sc.entry_list()
    want, offs, _nc, _pay = _want(pf, codec, "plain", ents)
    names, datas = [n for n, _d in ents], [d for _n, d in ents]
    lens = [len(d) for d in datas]
    src, soff = _upload(datas)
    before = src.clone()
    G = 4096
    for cap, ok in ((len(want), True), (len(want) - 1, False)):
        big = torch.full((G + len(want) + G + 64,), 0xA5, dtype=torch.uint8, device="cuda")
        d_dst = big.data_ptr() + G
        assert d_dst % 16 == 0
        if ok:
            total, eoff = gpu_ctx.create_archive_device(names, src.data_ptr(), soff, lens, d_dst, cap, algo=pna.ALGO_STORE)
            assert total == len(want) and eoff == offs and big[G:G + total].cpu().numpy().tobytes() == want
        else:
            with pytest.raises(pna.PnaGpuError) as ei:
                gpu_ctx.create_archive_device(names, src.data_ptr(), soff, lens, d_dst, cap, algo=pna.ALGO_STORE)
            assert ei.value.code == pna.E_DSTSIZE
        assert bool((big[:G] == 0xA5).all()) and bool((big[G + cap:] == 0xA5).all())
        assert torch.equal(src, before)


def _solid_device(pna, ctx, tree, cfg=None, mcs=0, extra=None, facets=None):
    import torch
    names, datas, kinds, links = sc.tc.tree_args(tree)
    lens = [len(d) for d in datas]
    src, offs = _upload(datas)
    cipher = None if cfg is None else cfg.product(pna)
    cap = pna.solid_archive_tree_bound(pna.ALGO_STORE, names, lens, kinds, links, cipher=cipher, facets=facets, extra=extra, max_chunk_size=mcs)
    dst = torch.zeros(cap + 64, dtype=torch.uint8, device="cuda")
    total, _none = ctx.create_archive_tree_device(names, src.data_ptr(), offs, lens, dst.data_ptr(), cap, kinds, links, algo=pna.ALGO_STORE, cipher=cipher,
                                                  facets=facets, extra=extra, max_chunk_size=mcs, solid=True)
    assert total <= cap
    return dst[:total].cpu().numpy().tobytes()


def _solid_host(pna, ctx, tree, cfg=None, mcs=0, extra=None, facets=None):
    names, datas, kinds, links = sc.tc.tree_args(tree)
    return pna.create_archive_tree(ctx, names, datas, kinds, links, algo=pna.ALGO_STORE, cipher=None if cfg is None else cfg.product(pna), facets=facets, extra=extra,
                                   max_chunk_size=mcs, solid=True)


SOLID = {"plain": (None, 0, False, False), "plain-mcs": (None, 65537, False, False), "ctr": ("ctr", 0, False, False), "ctr-mcs": ("ctr", 65537, False, False),
         "gcm": ("gcm", 0, False, False), "meta": (None, 65537, True, False), "kinds": (None, 0, False, True), "kinds-ctr-meta": ("ctr", 1000, True, True)}


@pytest.mark.parametrize("case", list(SOLID))
def test_solid(pna, pf, codec, gpu_ctx, case):
    """The stored solid stream over the size list: k_store writes the inner payloads where they stand in the SDAT bodies, the inner FDAT CRCs are the
    fold's (an SDAT cut at 65 537 falls into payloads and CRC fields), CTR and GCM STREAM (segments of 65 536 bytes) run over the stream in place.  The host
    form carries the stream through windows: at solid_win_mib = 1 the 8 MiB stream of the size list is cut into nine (an SDAT chunk spans them all by default:
    its CRC register is chained from window to window; at 65 537 chunks begin and end inside every window), at the default it is one window; both equal the
    device form.  The decoded inner stream is the oracle's serialisation of the records."""
    mode, mcs, with_meta, with_kinds = SOLID[case]
    tree = sc.tree_entries() if with_kinds else sc.size_tree()
    cfg = _cfg(pna, mode, 1, 1, 65536)
    extra, facets = sc.meta_blobs(pf, len(tree)) if with_meta else (None, None)
    want, inner = _memo(("solid", case), lambda: sc.expected_solid(pf, codec, tree, mcs, cfg, extra, facets))
    got = _solid_device(pna, gpu_ctx, tree, cfg, mcs, extra, facets)
    assert got == want
    fused, copy_only, folded, _ms = pna.store_stats(gpu_ctx)
    assert fused > 0 and copy_only == 0 and folded == sum(len(pf.flatten_writer([d], mcs if mcs else pf.MAX_CHUNK_DATA_LENGTH)) for k, _n, d in tree if k == sc.FILE)
    for win in (1, 256):
        with gpu_ctx.options(solid_win_mib=(win, 256)):
            assert _solid_host(pna, gpu_ctx, tree, cfg, mcs, extra, facets) == want, win
            fused, copy_only, _folded, _ms = pna.store_stats(gpu_ctx)      # the window stage ran (k_store's copy-only form, a piece per MiB of a window's chunk parts)
            assert fused == 0 and copy_only >= (len(inner) >> 20 if win == 1 else 1)
    assert sc.solid_stream_back(pf, codec, want, cfg) == inner
    items = pf.read_solid_inner(inner)
    assert [(it.kind, it.name, it.data) for it in items] == [(k, pf.sanitize_name(n), d) for k, n, d in tree]
    if case == "plain":
        assert pna.create_archive(None, [n for _k, n, _d in tree], [d for _k, _n, d in tree], algo=pna.ALGO_STORE, solid=True) == want
    password = b"password" if mode else None
    got = pna.extract_archive(gpu_ctx, want, password)
    assert [(g[0], g[1]) for g in got] == [(pf.sanitize_name(n), k) for k, n, _d in tree]
    assert [g[2] for g, (k, _n, _d) in zip(got, tree) if k == sc.FILE] == [d for k, _n, d in tree if k == sc.FILE]
    recs, summ = pna.verify_archive(gpu_ctx, want, password)
    assert summ["rc"] == 0 and len(recs) == len(tree) and all(r[2] == pna.VERIFY_OK for r in recs)


def test_solid_edges(pna, pf, codec, gpu_ctx):
    """No entries (no SDAT chunk at all, as the host loop writes it), one empty file, and CBC, which stays refused with its text"""
    assert _solid_device(pna, gpu_ctx, []) == sc.expected_solid(pf, codec, [])[0] == pna.create_archive(None, [], [], algo=pna.ALGO_STORE, solid=True)
    one = [(sc.FILE, "e", b"")]
    assert _solid_device(pna, gpu_ctx, one) == _solid_host(pna, gpu_ctx, one) == sc.expected_solid(pf, codec, one)[0]
    gcm = _cfg(pna, "gcm", 1, 1, 4096)
    assert _solid_device(pna, gpu_ctx, [], gcm) == sc.expected_solid(pf, codec, [], cfg=gcm)[0]      # the empty final segment's tag
    with pytest.raises(pna.PnaGpuError) as ei:
        _solid_device(pna, gpu_ctx, sc.size_tree(sc.SMALL_SIZES), _cfg(pna, "cbc", 1))
    assert ei.value.code == pna.E_UNSUPPORTED and "CBC" in str(ei.value)


def test_still_refused(pna, gpu_ctx):
    """compress_batch, compress_solid, the streaming facade, stream_entry and the multi-context create answer PNA_ALGO_STORE as before"""
    for call in (lambda: gpu_ctx.compress_batch([b"abc" * 100], algo=pna.ALGO_STORE),
                 lambda: pna.create_archive_multi([gpu_ctx, gpu_ctx], ["a", "b"], [b"x" * 100, b"y" * 100], algo=pna.ALGO_STORE),
                 lambda: gpu_ctx.compress_solid(b"x" * 1000, algo=pna.ALGO_STORE)):
        with pytest.raises(pna.PnaGpuError) as ei:
            call()
        assert ei.value.code == pna.E_UNSUPPORTED
    import io
    with pytest.raises(pna.PnaGpuError) as ei:
        gpu_ctx.writer(io.BytesIO(), algo=pna.ALGO_STORE)
    assert ei.value.code == pna.E_UNSUPPORTED
    with pytest.raises(pna.PnaGpuError) as ei:
        pna.write_file(gpu_ctx, lambda b: None, "a", [b"x" * 100], algo=pna.ALGO_STORE)
    assert ei.value.code == pna.E_UNSUPPORTED
