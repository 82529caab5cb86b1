"""pna_gpu_extract_select_host: the public declarations, the exported symbols, and pna_extract_plan_runs (host code) pinned on hand-made layouts."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PNA_E_INVAL = -2                                                        # include/pna_gpu.h
SYMBOLS = ("pna_gpu_extract_select_host", "pna_extract_plan_runs", "pna_gpu_debug_extract_stats", "pna_gpu_debug_pick_device")


def header():
    return open(os.path.join(ROOT, "include", "pna_gpu.h")).read()


def test_header_declares_extract_select():
    h = header()
    for name in SYMBOLS:
        assert re.search(r"int\s+%s\s*\(" % name, h), name
    for name in ("pna_extract_dest", "pna_extract_select_fn", "pna_extract_record_fn", "pna_extract_summary", "PNA_EXTRACT_CHECK_ALL",
                 "io::read_chunk"):                                     # (the comment names the departure for skipped entries)
        assert name in h, name


def test_library_exports_extract_select(pna):
    lib = pna.load_library()
    for name in SYMBOLS:
        assert name in pna.EXPORTS
        getattr(lib, name)
    assert ctypes.sizeof(pna.ExtractDest) == 24 and ctypes.sizeof(pna.ExtractSummary) == 40


def test_python_constants_match_the_header(pna):
    h = header()
    for name in ("SKIP", "HOST", "DEVICE", "OK", "TOO_SMALL", "CHECK_ALL", "GAP_MAX"):
        m = re.search(r"#define\s+PNA_EXTRACT_%s\s+(\d+)" % name, h)
        assert m and int(m.group(1)) == getattr(pna, "EXTRACT_" + name), name
    d = open(os.path.join(ROOT, "portable-network-archive_amd", "csrc", "pna_dev.h")).read()
    assert int(re.search(r"PICK_TILE\s*=\s*(\d+)", d).group(1)) == pna.PICK_TILE


def test_null_arguments(pna):
    L = pna.load_library()
    arc = b"\x89PNA\r\n\x1a\n" + bytes(64)
    parts = (ctypes.c_char_p * 1)(arc)
    lens = (ctypes.c_size_t * 1)(len(arc))
    sel = pna.EXTRACT_SELECT_FN(lambda *a: 0)
    cb = pna.EXTRACT_RECORD_FN(lambda *a: 0)
    f = L.pna_gpu_extract_select_host
    # (without a device no context can be made: the other arguments' checks with a real context are in tests/test_gpu_extract_select.py)
    assert f(None, parts, lens, 1, None, 0, 0, sel, cb, None, None) == PNA_E_INVAL
    assert L.pna_gpu_debug_extract_stats(None, None, None, None, None, None) == PNA_E_INVAL
    assert L.pna_gpu_debug_pick_device(None, 0, None, None, None, None, None) == PNA_E_INVAL
    k = ctypes.c_size_t()
    assert L.pna_extract_plan_runs(None, None, None, 3, 0, None, None, ctypes.byref(k)) == PNA_E_INVAL
    assert L.pna_extract_plan_runs(None, None, None, 0, 0, None, None, None) == PNA_E_INVAL


def covered(runs):
    return sum(n for _, n in runs)


def test_plan_runs_layouts(pna):
    G = 1000
    off = [100, 300, 700, 1500, 4000]
    ln = [200, 400, 300, 500, 100]                                  # records 0 | 1 adjacent, 1 | 2 adjacent, 2 .. 3 a gap of 500, 3 .. 4 a gap of 2000
    assert pna.extract_plan_runs(off, ln, [0] * 5, G) == []
    assert pna.extract_plan_runs([], [], [], G) == []
    assert pna.extract_plan_runs(off[:3], ln[:3], [1] * 3, 0) == [(100, 900)]                    # everything wanted and adjacent: one run
    assert pna.extract_plan_runs(off, ln, [1] * 5, G) == [(100, 1900), (4000, 100)]
    assert pna.extract_plan_runs(off, ln, [1, 0, 0, 0, 1], 1 << 40) == [(100, 4000)]
    assert pna.extract_plan_runs(off, ln, [1, 0, 1, 0, 0], 399) == [(100, 200), (700, 300)]
    # two wanted records gap_max apart merge, gap_max + 1 apart do not
    for gap in (0, 1, G - 1, G, G + 1, 5 * G):
        runs = pna.extract_plan_runs([50, 50 + 70 + gap], [70, 30], [1, 1], G)
        assert runs == ([(50, 100 + gap)] if gap <= G else [(50, 70), (120 + gap, 30)]), gap
    # a wanted record of length 0 neither crashes nor opens a run
    assert pna.extract_plan_runs([10, 20, 20, 90], [10, 0, 5, 0], [0, 1, 0, 1], G) == []
    assert pna.extract_plan_runs([10, 20, 20], [10, 0, 5], [1, 1, 1], 0) == [(10, 15)]
    # records out of order are refused
    L = pna.load_library()
    ro, rl, w = (ctypes.c_uint64 * 2)(100, 50), (ctypes.c_uint64 * 2)(10, 10), (ctypes.c_uint8 * 2)(1, 1)
    k = ctypes.c_size_t()
    assert L.pna_extract_plan_runs(ro, rl, w, 2, 0, None, None, ctypes.byref(k)) == PNA_E_INVAL
    ro = (ctypes.c_uint64 * 2)(50, 100)
    assert L.pna_extract_plan_runs(ro, rl, w, 2, 0, None, None, ctypes.byref(k)) == 0 and k.value == 2          # (counting only: no output arrays)


def test_plan_runs_cover_bounds(pna):
    """the runs never cover fewer bytes than the wanted records, never more than those plus the gaps merged, hold every wanted record whole and lie in order"""
    import random
    rnd = random.Random(7)
    for trial in range(200):
        n = rnd.randrange(1, 40)
        G = rnd.choice([0, 1, 64, 1000, 65536])
        off, ln, at = [], [], rnd.randrange(0, 100)
        for _ in range(n):
            off.append(at)
            ln.append(rnd.choice([0, 1, 12, 500, 70000]))
            at += ln[-1] + rnd.choice([0, 0, 1, G, G + 1, 3 * G + 5])
        want = [rnd.random() < 0.4 for _ in range(n)]
        runs = pna.extract_plan_runs(off, ln, want, G)
        live = [i for i in range(n) if want[i] and ln[i]]
        wanted = sum(ln[i] for i in live)
        gaps = sum(off[b] - (off[a] + ln[a]) for a, b in zip(live, live[1:]) if off[b] - (off[a] + ln[a]) <= G)
        assert wanted <= covered(runs) <= wanted + gaps and covered(runs) == wanted + gaps
        assert all(a[0] + a[1] + G < b[0] for a, b in zip(runs, runs[1:]))
        for i in live:
            assert any(o <= off[i] and off[i] + ln[i] <= o + m for o, m in runs), (trial, i)
