"""The extract driver on a deflate solid archive of about 8 GiB (pna_gpu_create_solid_archive_host, one inner entry of 3.5 GiB -- the driver reads inner
FDAT chunks below 2^32 - 16 bytes): the SDAT stream is measured on the device (pna_gpu_open_size_device), decoded into a buffer of exactly that size and
every inner entry is compared by hash."""
import ctypes
import hashlib

import pytest

pytestmark = pytest.mark.gpu


def test_deflate_solid_8gib_extracts(big_ctx, pna, pf):
    import numpy as np
    import torch
    free, _ = torch.cuda.mem_get_info()
    assert free >= 120 << 30, f"the full-size case needs 120 GiB of free HBM, found {free >> 30} GiB: an MI355X has 288 GB"
    n1, L = 8192, 1 << 20
    src = torch.empty(n1 * L + 8192, dtype=torch.uint8, device="cuda")
    big_ctx.corpus_fill_device(0, 0, n1, L, L, src.data_ptr())
    host = src[:n1 * L].cpu().numpy()
    del src
    torch.cuda.empty_cache()
    big = 3584 * L + 12345
    cuts = [0, 3000, 3000 + big, 3000 + big + 777, 3000 + big + 777 + 5 * L]
    views = [host[a:b] for a, b in zip(cuts, cuts[1:])]
    pos = cuts[-1]
    while pos + L + 4321 <= n1 * L:
        views.append(host[pos:pos + L + 4321]); pos += L + 4321
    views.insert(2, host[:0])
    names = [f"big/{i:05d}.bin" for i in range(len(views))]
    assert sum(len(v) for v in views) > (8 << 30) - (2 << 20)
    parts = []

    def _sink(_u, buf, k):
        parts.append(np.ctypeslib.as_array(ctypes.cast(buf, ctypes.POINTER(ctypes.c_ubyte)), shape=(k,)).copy())
        return 0
    scb = pna.SINK_FN(_sink)
    n = len(views)
    a_names = (ctypes.c_char_p * n)(*[s.encode() for s in names])
    a_src = (ctypes.c_void_p * n)(*[v.ctypes.data if len(v) else 0 for v in views])
    a_len = (ctypes.c_size_t * n)(*[len(v) for v in views])
    big_ctx._check(big_ctx._L.pna_gpu_create_solid_archive_host(big_ctx._h, pna.ALGO_DEFLATE, pna.LEVEL_DEFAULT, n, a_names, a_src, a_len, scb, None))
    arc = np.concatenate(parts)
    del parts
    want = [(nm, hashlib.sha256(v).digest()) for nm, v in zip(names, views)]
    del views, host
    seen = []

    def _cb(_u, idx, name, kind, data, k):
        h = hashlib.sha256(np.ctypeslib.as_array(ctypes.cast(data, ctypes.POINTER(ctypes.c_ubyte)), shape=(k,)) if k else b"").digest()
        seen.append((name.decode(), h))
        return 0
    cb = pna.ENTRY_FN(_cb)
    big_ctx._check(big_ctx._L.pna_gpu_extract_archive_host(big_ctx._h, arc.ctypes.data_as(ctypes.c_char_p), len(arc), None, 0, cb, None))
    assert len(seen) == len(want)
    for (n_a, h_a), (n_b, h_b) in zip(seen, want):
        assert n_a == n_b and h_a == h_b, n_a
