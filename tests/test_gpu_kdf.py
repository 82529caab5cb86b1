"""Key derivation on the device (k_kdf.hip: k_argon2_fill, k_pbkdf2_sha256; pna_gpu_kdf_batch) and the read-side drivers under option kdf_device.
Keys are compared byte for byte with the host functions pna_kdf_argon2 / pna_kdf_pbkdf2_sha256, which tests/test_kdf_core.py holds against the oracle's
Argon2 and hashlib over the same case list (tests/kdf_cases.py); pna_gpu_debug_kdf_stats proves that a job ran on the device and was not rerouted."""
import base64
import functools
import os

import pytest

import kdf_cases as K
from conftest import GOLDEN, golden

pytestmark = pytest.mark.gpu
PW = b"password"
FIXTURES = ["zstd_aes_ctr.pna", "zstd_aes_cbc.pna", "camellia/zstd_camellia_ctr.pna", "camellia/zstd_camellia_cbc.pna"]


@pytest.fixture(scope="module")
def ctx(pna):
    import torch  # noqa: F401
    c = pna.Context(0)
    c.set_option("camellia", 1)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def host_key(kind, t, m, p, rounds, salt, password=PW):
    """the host function's answer for a job (shared by the tests, never changed)"""
    import importlib
    pna = importlib.import_module("portable-network-archive_amd")
    if kind == K.PBKDF2:
        return pna.kdf_pbkdf2_sha256(password, salt, rounds)[0]
    return pna.kdf_argon2(kind, password, salt, t, m, p)


def want_of(jobs, password=PW):
    return [host_key(j["kind"], j.get("t_cost", 0), j.get("m_cost_kib", 0), j.get("lanes", 0), j.get("rounds", 0), j["salt"], password) for j in jobs]


def case_jobs():
    return K.jobs_one_password(PW)[0]


def argon(m, t=1, p=1, kind=K.ARGON2ID, salt=b"saltsalt"):
    return {"kind": kind, "t_cost": t, "m_cost_kib": m, "lanes": p, "salt": salt}


def test_one_mixed_batch(pna, ctx):
    """every kind, parameter set and PBKDF2 job of the case list side by side in one call"""
    jobs = case_jobs()
    assert len(jobs) == len(K.argon_cases()) + len(K.pbkdf2_cases())
    keys, st = pna.kdf_batch(ctx, PW, jobs)
    assert st == [0] * len(jobs)
    want = want_of(jobs)
    bad = [(i, jobs[i]) for i in range(len(jobs)) if keys[i] != want[i]]
    assert not bad, bad[:5]
    dev, host, rounds, ms = pna.kdf_stats(ctx)
    assert (dev, host) == (len(jobs), 0) and rounds == 1 and ms > 0


def test_password_lengths(pna, ctx):
    """H0's input crosses a BLAKE2b block edge, HMAC's key is hashed first beyond 64 bytes: one small batch per password length"""
    jobs = [argon(16, 2, 1, kind, K._bytes(40 + kind, (8, 16, 48)[kind])) for kind in (0, 1, 2)] + [argon(32, 1, 2), {"kind": K.PBKDF2, "rounds": 3, "salt": b"s" * 52}]
    for n in sorted(set(K.PW_LENS) | {63, 64, 65, 200, 1024}):
        pw = K._bytes(900 + n, n)
        keys, st = pna.kdf_batch(ctx, pw, jobs)
        assert keys == want_of(jobs, pw) and st == [0] * len(jobs), n
        assert pna.kdf_stats(ctx)[:2] == (len(jobs), 0), n


def test_one_job_per_call(pna, ctx):
    jobs = case_jobs()
    want = want_of(jobs)
    for j, w in zip(jobs, want):
        keys, st = pna.kdf_batch(ctx, PW, [j])
        assert keys == [w] and st == [0], j
        assert pna.kdf_stats(ctx)[:2] == (1, 0), j
    assert pna.kdf_batch(ctx, PW, []) == ([], [])


def test_reference_defaults(pna, ctx):
    """argon2id m=19456,t=2,p=1 (the reference's default) and PBKDF2 at 10 000 rounds"""
    jobs = [argon(19456, 2, 1, K.ARGON2ID, K._bytes(70 + i, 16)) for i in range(4)] + [{"kind": K.PBKDF2, "rounds": 10000, "salt": K._bytes(80 + i, 16)} for i in range(2)]
    keys, st = pna.kdf_batch(ctx, PW, jobs)
    assert keys == want_of(jobs) and st == [0] * 6
    assert pna.kdf_stats(ctx)[:3] == (6, 0, 1)
    assert keys[0] == pna.kdf_derive("argon2id", PW, jobs[0]["salt"])[0]


def test_rounds_and_the_cap(pna, ctx):
    jobs = [argon(1024, 1, 1, i % 3, K._bytes(100 + i, 16)) for i in range(64)]
    want = want_of(jobs)
    ctx.set_option("kdf_mem_mib", 8)
    try:
        keys, st = pna.kdf_batch(ctx, PW, jobs)
        assert keys == want and st == [0] * 64
        assert pna.kdf_stats(ctx)[:3] == (64, 0, 8)                  # 8 jobs of 1 MiB fit 8 MiB
        # a job that alone exceeds the cap is the host's; its neighbours stay on the device
        mixed = [jobs[0], argon(8196, 1, 1), jobs[1], argon(16384, 1, 2, K.ARGON2I)]
        keys, st = pna.kdf_batch(ctx, PW, mixed)
        assert keys == want_of(mixed) and st == [0] * 4
        assert pna.kdf_stats(ctx)[:2] == (2, 2)
        keys, st = pna.kdf_batch(ctx, PW, [argon(8192, 1, 1)])       # exactly the cap: one job, one round
        assert keys == want_of([argon(8192, 1, 1)]) and pna.kdf_stats(ctx)[:3] == (1, 0, 1)
    finally:
        ctx.set_option("kdf_mem_mib", 0)
    with pytest.raises(pna.PnaGpuError):
        ctx.set_option("kdf_mem_mib", -1)


def test_jobs_outside_the_device_limits(pna, ctx):
    jobs = [argon(136, 1, 17), argon(128, 1, 16), argon(64, 65, 1), {"kind": K.PBKDF2, "rounds": 5, "salt": b"x" * 65}, argon(64, 1, 1, salt=b"y" * 65), argon(64, 1, 2)]
    keys, st = pna.kdf_batch(ctx, PW, jobs)
    assert keys == want_of(jobs) and st == [0] * 6
    assert pna.kdf_stats(ctx)[:2] == (2, 4)
    pw = K._bytes(5, 1025)                                           # a password beyond 1 024 bytes: everything on the host
    small = [argon(64, 1, 1), {"kind": K.PBKDF2, "rounds": 5, "salt": b"x" * 8}]
    keys, st = pna.kdf_batch(ctx, pw, small)
    assert keys == want_of(small, pw) and pna.kdf_stats(ctx)[:2] == (0, 2)


def test_refused_parameters(pna, ctx):
    jobs = [argon(64, 1, 1), argon(15, 1, 2), {"kind": K.PBKDF2, "rounds": 7, "salt": b"saltsalt"}, argon(64, 0, 1), {"kind": K.PBKDF2, "rounds": 0, "salt": b"s"},
            {"kind": 9, "salt": b"s"}, argon(64, 2, 2)]
    keys, st = pna.kdf_batch(ctx, PW, jobs)
    assert st == [0, pna.E_INVAL, 0, pna.E_INVAL, pna.E_INVAL, pna.E_INVAL, 0]
    good = [0, 2, 6]
    assert [keys[i] for i in good] == want_of([jobs[i] for i in good])
    assert pna.kdf_stats(ctx)[0] == 3
    with pytest.raises(pna.PnaGpuError) as e:
        pna.kdf_batch(ctx, PW, jobs, with_status=False)
    assert e.value.code == pna.E_INVAL


# ---- the read-side drivers under option kdf_device
def golden_files():
    out = {}
    for d, _, fs in os.walk(os.path.join(GOLDEN, "raw")):
        for f in fs:
            p = os.path.join(d, f)
            out[os.path.relpath(p, GOLDEN).replace(os.sep, "/")] = open(p, "rb").read()
    return out


def with_option(ctx, n, fn):
    ctx.set_option("kdf_device", n)
    try:
        return fn()
    finally:
        ctx.set_option("kdf_device", 0)


@pytest.mark.parametrize("fname", FIXTURES)
def test_reference_archives(pna, ctx, fname):
    """9 entries, 9 distinct PHSF strings (m=4096,t=3): one batch of 9 device jobs in every driver, the same results as with the option off"""
    arc, raw = golden(fname), golden_files()
    sel = lambda i, nm, k, st: "host"
    off = (pna.extract_archive(ctx, arc, PW), pna.verify_archive(ctx, arc, PW), pna.extract_select(ctx, arc, sel, PW))
    assert len(off[0]) == 9 and sum(1 for n, _, d in off[0] if raw.get(n) == d) >= 5
    files = {n: d for n, _, d in off[0]}                             # every entry has a file to be compared with: diff needs all nine keys
    for name, call in (("extract", lambda: pna.extract_archive(ctx, arc, PW)), ("verify", lambda: pna.verify_archive(ctx, arc, PW)),
                       ("select", lambda: pna.extract_select(ctx, arc, sel, PW)), ("diff", lambda: pna.diff_archive(ctx, arc, files, PW))):
        pna.kdf_batch(ctx, PW, [])                                   # (the counters back to zero)
        got = with_option(ctx, 1, call)
        assert pna.kdf_stats(ctx)[:2] == (9, 0), name
        if name == "extract":
            assert got == off[0]
        elif name == "verify":
            assert got == off[1] and all(r[2] == pna.VERIFY_OK for r in got[0]) and len(got[0]) == 9
        elif name == "select":
            assert got == off[2] and pna.extract_stats(ctx)[2] == 9
        else:
            recs, s = got
            assert s["rc"] == 0 and len(recs) == 9 and all(r.status == pna.DIFF_SAME for r in recs) and s["same"] == 9
    if "cbc" in fname:                                               # a wrong password fails as it does with the option off
        def wrong():
            try:
                return pna.extract_archive(ctx, arc, b"passw0rd")
            except pna.PnaGpuError as e:
                return (e.code, str(e))
        a, b = wrong(), with_option(ctx, 1, wrong)
        assert a == b and a[0] == pna.E_INVAL
        assert pna.verify_archive(ctx, arc, b"passw0rd") == with_option(ctx, 1, lambda: pna.verify_archive(ctx, arc, b"passw0rd"))


def b64(salt):
    return base64.b64encode(salt).decode().rstrip("=")


@pytest.fixture(scope="module")
def salted(pna, ctx):
    """64 entries, one salt each (argon2id m=64,t=1), written by one part call per entry: (entries, {mode: archive})"""
    ents = [K._bytes(300 + i, 1 + 997 * i % 5000) for i in range(64)]
    arcs = {}
    for mode in (pna.MODE_CTR, pna.MODE_GCM):
        parts = []
        for i, e in enumerate(ents):
            salt = K._bytes(500 + i, 16)
            key = host_key(K.ARGON2ID, 1, 64, 1, 0, salt)
            part = (pna.PART_HEAD if i == 0 else 0) | (pna.PART_TAIL if i == 63 else 0)
            parts.append(pna.create_archive_chunked(ctx, ["e/%02d" % i], [e], 0, cipher=pna.Cipher(key, "$argon2id$v=19$m=64,t=1,p=1$" + b64(salt), mode), part=part))
        arcs[mode] = b"".join(parts)
    return ents, arcs


def test_salt_per_entry(pna, ctx, salted):
    ents, arcs = salted
    want = [("e/%02d" % i, 0, e) for i, e in enumerate(ents)]
    for mode, arc in arcs.items():
        assert pna.extract_archive(ctx, arc, PW) == want
        pna.kdf_batch(ctx, PW, [])
        assert with_option(ctx, 1, lambda: pna.extract_archive(ctx, arc, PW)) == want
        assert pna.kdf_stats(ctx)[:2] == (64, 0)
        assert with_option(ctx, 65, lambda: pna.extract_archive(ctx, arc, PW)) == want     # below the threshold: the host, one string after the other
        assert pna.kdf_stats(ctx)[:3] == (0, 0, 0)
        recs, s = with_option(ctx, 1, lambda: pna.verify_archive(ctx, arc, PW))
        assert s["ok"] == s["total"] == 64 and pna.kdf_stats(ctx)[:2] == (64, 0)


def rewrite_phsf(pf, arc, index, fn):
    out, k = bytearray(arc[:8]), 0
    for ty, data, _ in pf.read_chunks(arc, 8):
        if ty == b"PHSF":
            if k == index:
                data = fn(data)
            k += 1
        out += pf.write_chunk(ty, data)
    return bytes(out)


@pytest.mark.parametrize("what,status", [("p=300", "VERIFY_UNSUPPORTED"), ("m=6x4", "VERIFY_BAD_STRUCTURE")])
def test_one_bad_phsf(pna, pf, ctx, salted, what, status):
    arc = rewrite_phsf(pf, salted[1][pna.MODE_CTR], 17, lambda d: d.replace(b"p=1", what.encode()) if what[0] == "p" else d.replace(b"m=64", what.encode()))
    off = pna.verify_archive(ctx, arc, PW)
    pna.kdf_batch(ctx, PW, [])
    on = with_option(ctx, 1, lambda: pna.verify_archive(ctx, arc, PW))
    assert on == off
    assert pna.kdf_stats(ctx)[:2] == (63, 0)
    recs, s = on
    assert [r[2] for r in recs] == [pna.VERIFY_OK] * 17 + [getattr(pna, status)] + [pna.VERIFY_OK] * 46
    def ex():
        try:
            return pna.extract_archive(ctx, arc, PW)
        except pna.PnaGpuError as e:
            return (e.code, str(e))
    a, b = ex(), with_option(ctx, 1, ex)
    assert a == b and a[0] == (pna.E_UNSUPPORTED if what[0] == "p" else pna.E_INVAL)


def test_extract_select_derives_only_what_it_hands_out(pna, ctx, salted):
    ents, arcs = salted
    pick = {3, 31, 60}
    sel = lambda i, nm, k, st: "host" if i in pick else None
    off = pna.extract_select(ctx, arcs[pna.MODE_CTR], sel, PW)
    assert pna.extract_stats(ctx)[2] == 3
    pna.kdf_batch(ctx, PW, [])
    on = with_option(ctx, 1, lambda: pna.extract_select(ctx, arcs[pna.MODE_CTR], sel, PW))
    assert on == off and [r[4] for r in on[0]] == [ents[i] for i in sorted(pick)]
    assert pna.extract_stats(ctx)[2] == 3 and pna.kdf_stats(ctx)[:2] == (3, 0)
