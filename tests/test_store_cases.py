"""tests/store_cases.py checked on the CPU: the expectations the GPU tests of the stored create paths (tests/test_gpu_store.py) compare with.

Without a cipher the helper's bytes equal the library's host loop (pna_create_archive with PNA_ALGO_STORE, which needs no GPU); with one, every case reads
back through the oracle's reader -- every chunk CRC checked, the cipher layer undone by the oracle's AES (Camellia: tests/camellia_cases.py, every GCM tag
verified) -- to the inputs.  The bound functions need no context: pna_gpu_*_bound(PNA_ALGO_STORE, ..) >= the expected length for every case."""
import pytest

import store_cases as sc

_cache = {}


def _memo(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def _key(pna):
    return _memo("key", lambda: pna.kdf_pbkdf2_sha256(b"password", bytes(range(16)), 1000))


def _cfg(pna, mode, n, encryption=1, seg=0):
    key, phsf = _key(pna)
    return sc.CipherCfg(key, phsf, mode, n, encryption, seg)


def test_plain_equals_the_host_loop(pna, pf, codec):
    ents = sc.entry_list()
    want, offs, nchunks, pay = sc.expected_archive(pf, codec, ents)
    assert pna.create_archive(None, [n for n, _d in ents], [d for _n, d in ents], algo=pna.ALGO_STORE) == want
    assert nchunks == sum(1 for _n, d in ents if d) and len(offs) == len(ents) + 1
    assert {p % 16 for p in pay} == set(range(16))               # the payloads' archive offsets take every residue mod 16
    assert sorted(len(n) for n, _d in ents)[0] == 1 and max(len(n) for n, _d in ents) == 40
    assert pna.archive_bound(pna.ALGO_STORE, [n for n, _d in ents], [len(d) for _n, d in ents]) >= len(want)
    assert [it.data for it in pf.read_archive(want)[1]] == [d for _n, d in ents]


@pytest.mark.parametrize("mcs", (5, 16, 17, 4096, 65537, sc.MIB - 1, sc.MIB + 1))
def test_chunked_expectation_reads_back(pna, pf, codec, mcs):
    ents = sc.entry_list(sc.SMALL_SIZES if mcs < 4096 else sc.SIZES)
    want, _offs, nchunks, _pay = sc.expected_archive(pf, codec, ents, mcs=mcs)
    items = pf.read_archive(want)[1]
    assert [it.data for it in items] == [d for _n, d in ents]
    assert nchunks == sum((len(d) + mcs - 1) // mcs for _n, d in ents)
    for it, (_n, d) in zip(items, ents):                           # FlattenWriter's cut: every chunk full but the last
        assert [len(x) for t, x in it.chunks if t == b"FDAT"] == [min(mcs, len(d) - o) for o in range(0, len(d), mcs)]
    assert pna.archive_chunked_bound(pna.ALGO_STORE, [n for n, _d in ents], [len(d) for _n, d in ents], mcs) >= len(want)


@pytest.mark.parametrize("mode,seg", (("ctr", 0), ("cbc", 0), ("gcm", 4096), ("gcm", 0)))
@pytest.mark.parametrize("with_meta", (False, True))
def test_encrypted_expectation_reads_back(pna, pf, codec, mode, seg, with_meta):
    ents = sc.entry_list()
    cfg = _cfg(pna, mode, len(ents), 1, seg)
    extra, facets = sc.meta_blobs(pf, len(ents)) if with_meta else (None, None)
    want, _offs, _nc, _pay = sc.expected_archive(pf, codec, ents, cfg=cfg, extra=extra, facets=facets)
    assert sc.read_back(pf, codec, want, cfg) == [d for _n, d in ents]
    items = pf.read_archive(want)[1]
    assert all((it.compression, it.encryption, it.cipher_mode) == (0, 1, cfg.mode_byte) for it in items)
    empty = [x for t, x in items[0].chunks if t == b"FDAT"]       # the empty entry: CTR the IV alone, CBC + one padding block, GCM + the final segment's tag
    assert [len(x) for x in empty] == {"ctr": [16], "cbc": [16, 16], "gcm": [75, 16]}[mode]
    if with_meta:
        assert [t for t, _x in items[3].chunks][:5] == [b"FHED", b"usRc", b"fSIZ", b"mTIM", b"fPRM"]
    names, lens = [n for n, _d in ents], [len(d) for _n, d in ents]
    assert pna.archive_tree_bound(pna.ALGO_STORE, names, lens, cipher=cfg.product(pna), facets=facets, extra=extra) >= len(want)
    assert pna.archive_enc_bound(pna.ALGO_STORE, names, lens, cfg.product(pna)) >= len(want) - sum(len(x) for x in (extra or [])) - sum(len(x) for x in (facets or []))


@pytest.mark.parametrize("mode", ("ctr", "cbc", "gcm"))
def test_camellia_expectation_reads_back(pna, pf, codec, mode):
    ents = sc.entry_list(sc.CAMELLIA_SIZES)
    cfg = _cfg(pna, mode, len(ents), 2, 4096 if mode == "gcm" else 0)
    want, _offs, _nc, _pay = sc.expected_archive(pf, codec, ents, cfg=cfg)
    assert sc.read_back(pf, codec, want, cfg) == [d for _n, d in ents]
    assert all(it.encryption == 2 for it in pf.read_archive(want)[1])


@pytest.mark.parametrize("mode", (None, "ctr", "gcm"))
def test_tree_expectation(pna, pf, codec, mode):
    tree = sc.tree_entries()
    ents, kinds = [(n, d) for _k, n, d in tree], [k for k, _n, _d in tree]
    cfg = None if mode is None else _cfg(pna, mode, len(ents), 1, 65536)
    for mcs in ((0,) if mode == "gcm" else (0, 1000)):
        want, offs, _nc, _pay = sc.expected_archive(pf, codec, ents, mcs=mcs, cfg=cfg, kinds=kinds)
        items = pf.read_archive(want)[1]
        assert [(it.kind, it.name) for it in items] == [(k, pf.sanitize_name(n)) for k, n, _d in tree]
        for it, (k, _n, d) in zip(items, tree):                    # links stay in the clear
            if k != sc.FILE:
                assert (it.data, it.encryption) == (d, 0)
        back = sc.read_back(pf, codec, want, cfg)
        assert [b for b in back if b is not None] == [d for k, _n, d in tree if k == sc.FILE]
        names, datas, tkinds, links = sc.tc.tree_args(tree)
        assert pna.archive_tree_bound(pna.ALGO_STORE, names, [len(d) for d in datas], tkinds, links, cipher=None if cfg is None else cfg.product(pna),
                                      max_chunk_size=mcs) >= len(want)


def test_parts_concatenate(pf, codec):
    ents = sc.entry_list(sc.SMALL_SIZES)
    whole = sc.expected_archive(pf, codec, ents)[0]
    a = sc.expected_archive(pf, codec, ents[:4], head=True, tail=False)[0]
    b = sc.expected_archive(pf, codec, ents[4:7], head=False, tail=False)[0]
    c = sc.expected_archive(pf, codec, ents[7:], head=False, tail=True)[0]
    assert a + b + c == whole


@pytest.mark.parametrize("mode,mcs", ((None, 0), (None, 65537), ("ctr", 65537), ("gcm", 0)))
def test_solid_expectation(pna, pf, codec, mode, mcs):
    tree = sc.size_tree()
    cfg = None if mode is None else _cfg(pna, mode, 1, 1, 65536)
    want, inner = sc.expected_solid(pf, codec, tree, mcs, cfg)
    names, datas = [n for _k, n, _d in tree], [d for _k, _n, d in tree]
    if mode is None and mcs == 0:
        assert pna.create_archive(None, names, datas, algo=pna.ALGO_STORE, solid=True) == want
        assert pna.solid_archive_bound(pna.ALGO_STORE, names, [len(d) for d in datas]) >= len(want)
    assert sc.solid_stream_back(pf, codec, want, cfg) == inner
    assert [(it.name, it.data) for it in pf.read_solid_inner(inner)] == [(pf.sanitize_name(n), d) for n, d in zip(names, datas)]
    assert pna.solid_archive_tree_bound(pna.ALGO_STORE, names, [len(d) for d in datas], cipher=None if cfg is None else cfg.product(pna), max_chunk_size=mcs) >= len(want)
