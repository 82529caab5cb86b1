"""The three routes that parse zstd headers on the device -- the lane-parallel pipeline (k_zparse<false>, the default), the one-workgroup kernel (k_zdec,
zdec_serial = 1) and the header walk of a large frame (k_zparse_a + k_zparse<true>, zexec_par_min_mib = 1 on a single frame of 1 MiB and more) --, held
to what they answered BEFORE their parsing was moved into csrc/zstd_parse_core.h.

Good data: every committed stream of tests/golden/zstd_parse/ (tests/zstd_parse_cases.py: the rare header branches) through the first two routes, this
library's own single frame of 1 MiB + 5 000 bytes through all three; the bytes are the plain text, and pna_gpu_last_decode_forms shows the route.
Damaged data: the damage list of tests/zstd_parse_cases.py on the first 40 bytes of that single frame, every case on every route (one context per
route): (return code, pna_gpu_last_error text, CRC-32 of the bytes where the call succeeded) must equal tests/golden/zstd_parse_routes.json.  That file
was recorded on an MI355X with the library of the commit before the move (`python tests/test_gpu_zstd_parse_routes.py --record`, PNA_GPU_LIB pointing
at that build), so the move is held to every code and every text of every route, byte for byte.  The inputs are the bounds-checked refusals the other
decoder tests exercise; no call decodes more than 1 MiB + 5 000 bytes."""
import json
import os
import sys
import zlib

import pytest

import zstd_parse_cases as Z

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "zstd_parse_routes.json")
ROUTES = {"default": {}, "serial": {"zdec_serial": 1}, "parallel": {"zexec_par_min_mib": 1}}
CUTS = (0, 5, 6, 9, 12, 39)


def _own_single(pna):
    """(frame, plain): this library's encoder, one frame for the whole entry, level 1"""
    import torch  # noqa: F401  (shares its HIP runtime with the extension)
    plain = Z.plain("text1m5000")
    with pna.Context(0) as enc:
        enc.set_option("latency_max_mib", 0)
        enc.set_option("single_frame", 1)
        frame = enc.compress_batch([plain], level=1)[0]
    assert frame[:4] == bytes.fromhex("28b52ffd")
    return frame, plain


def _route_ctx(pna, route):
    ctx = pna.Context(0)
    for k, v in ROUTES[route].items():
        ctx.set_option(k, v)
    return ctx


def _shown(route, forms):
    """the counters a decode call leaves: did the route the test is about take the frame?"""
    if route == "serial":
        return forms.zstd_workgroup_frames >= 1 and forms.zstd_executor_frames == 0
    if route == "parallel":
        return forms.zstd_executor_frames >= 1 and forms.zstd_workgroup_frames == 0
    return forms.zstd_workgroup_frames == 0 and forms.zstd_executor_frames == 0


def _outcome(pna, ctx, payload, size):
    try:
        out = ctx.decompress_batch([payload], [size], algo=pna.ALGO_ZSTD)
    except pna.PnaGpuError as e:
        prefix = f"pna_gpu error {e.code}: "
        assert str(e).startswith(prefix)
        return [e.code, str(e)[len(prefix):], None]
    return [0, "", zlib.crc32(out[0])]


def _record(pna):
    frame, plain = _own_single(pna)
    rec = {}
    for route in ROUTES:
        with _route_ctx(pna, route) as ctx:
            for name, bad in Z.damage_cases(frame, CUTS):
                rec["%s: %s" % (route, name)] = _outcome(pna, ctx, bad, len(plain))
    return rec


@pytest.fixture(scope="module")
def own(pna):
    return _own_single(pna)


RECORDED = {}
if os.path.exists(FIXTURE):
    with open(FIXTURE) as _f:
        RECORDED = json.load(_f)


@pytest.mark.parametrize("route", ["default", "serial"])
def test_fixtures_decode_on_the_route(pna, route):
    assert len(Z.fixtures()) == len(Z.FIXTURE_PLAINS) * len(Z.WRITERS) + 1
    with _route_ctx(pna, route) as ctx:
        for name, stream, plain in Z.fixtures():
            assert ctx.decompress_batch([stream], [len(plain)], algo=pna.ALGO_ZSTD) == [plain], name
            forms = ctx.decode_forms()
            print(route, name, forms.zstd_executor_frames, forms.zstd_workgroup_frames, forms.zstd_listed_entries)
            if name == "fixture_frame_list":                              # (its frames are listed one by one and decoded in calls of their own: that is what shows)
                assert forms.zstd_listed_entries == 1, name
            else:
                assert _shown(route, forms) and forms.zstd_listed_entries == 0, name


@pytest.mark.parametrize("route", sorted(ROUTES))
def test_own_single_frame_decodes_on_the_route(pna, own, route):
    frame, plain = own
    with _route_ctx(pna, route) as ctx:
        assert ctx.decompress_batch([frame], [len(plain)], algo=pna.ALGO_ZSTD) == [plain]
        forms = ctx.decode_forms()
        print(route, forms.zstd_executor_frames, forms.zstd_workgroup_frames)
        assert _shown(route, forms)


@pytest.mark.parametrize("route", sorted(ROUTES))
def test_damaged_headers_get_the_recorded_answer(pna, own, route):
    frame, plain = own
    cases = Z.damage_cases(frame, CUTS)
    assert len(cases) == 8 + 1 + 35 + len(CUTS) + 2
    wrong = []
    with _route_ctx(pna, route) as ctx:
        for name, bad in cases:
            got = _outcome(pna, ctx, bad, len(plain))
            print(route, name, got)
            if got != RECORDED.get("%s: %s" % (route, name)):
                wrong.append((name, got, RECORDED.get("%s: %s" % (route, name))))
    assert not wrong


def test_every_case_is_recorded(own):
    assert set(RECORDED) == {"%s: %s" % (r, n) for r in ROUTES for n, _ in Z.damage_cases(own[0], CUTS)}


if __name__ == "__main__":
    if len(sys.argv) < 2 or sys.argv[1] != "--record":
        sys.exit("usage: test_gpu_zstd_parse_routes.py --record [file]   (run it with the library whose behaviour is the contract)")
    import importlib
    pna_mod = importlib.import_module("portable-network-archive_amd")
    rec = _record(pna_mod)
    with open(sys.argv[2] if len(sys.argv) > 2 else FIXTURE, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    for k in sorted(rec):
        print(k, rec[k])
