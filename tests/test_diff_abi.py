"""`pna diff` (pna_gpu_diff_archive_host): the public declaration, the exported symbols, and the argument checks that run before any device work."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PNA_E_INVAL = -2                                                        # include/pna_gpu.h


def test_header_declares_diff():
    h = open(os.path.join(ROOT, "include", "pna_gpu.h")).read()
    assert re.search(r"int\s+pna_gpu_diff_archive_host\s*\(", h)
    assert re.search(r"int\s+pna_gpu_debug_diff_stats\s*\(", h)
    for name in ("PNA_DIFF_FS_MISSING", "PNA_DIFF_FS_FILE", "PNA_DIFF_FS_DIR", "PNA_DIFF_FS_SYMLINK", "PNA_DIFF_FS_OTHER", "PNA_DIFF_FS_IGNORE",
                 "PNA_DIFF_SAME", "PNA_DIFF_MISSING", "PNA_DIFF_TYPE_MISMATCH", "PNA_DIFF_SIZE_DIFFERS", "PNA_DIFF_CONTENTS_DIFFER",
                 "PNA_DIFF_SYMLINK_DIFFERS", "PNA_DIFF_NOT_COMPARED", "PNA_DIFF_SKIPPED", "PNA_DIFF_DAMAGED",
                 "pna_diff_file", "pna_diff_summary", "pna_diff_source_fn", "pna_diff_fn", "diff_slot_mib", "PNA_DIFF_SLOT_MIB"):
        assert name in h, name


def test_python_constants_match_the_header(pna):
    h = open(os.path.join(ROOT, "include", "pna_gpu.h")).read()
    for name in ("FS_MISSING", "FS_FILE", "FS_DIR", "FS_SYMLINK", "FS_OTHER", "FS_IGNORE", "SAME", "MISSING", "TYPE_MISMATCH", "SIZE_DIFFERS",
                 "CONTENTS_DIFFER", "SYMLINK_DIFFERS", "NOT_COMPARED", "SKIPPED", "DAMAGED"):
        m = re.search(r"#define\s+PNA_DIFF_%s\s+(\d+)" % name, h)
        assert m and int(m.group(1)) == getattr(pna, "DIFF_" + name), name
    d = open(os.path.join(ROOT, "portable-network-archive_amd", "csrc", "pna_dev.h")).read()
    assert int(re.search(r"DIFF_TILE\s*=\s*(\d+)", d).group(1)) == pna.DIFF_TILE


def test_library_exports_diff(pna):
    lib = pna.load_library()
    for name in ("pna_gpu_diff_archive_host", "pna_gpu_debug_diff_stats"):
        assert name in pna.EXPORTS
        getattr(lib, name)
    assert ctypes.sizeof(pna.DiffSummary) == 56 and ctypes.sizeof(pna.DiffFile) == 24


def test_diff_null_arguments(pna):
    L = pna.load_library()
    arc = b"\x89PNA\r\n\x1a\n" + bytes(64)
    parts = (ctypes.c_char_p * 1)(arc)
    lens = (ctypes.c_size_t * 1)(len(arc))
    src = pna.DIFF_SOURCE_FN(lambda *a: 0)
    cb = pna.DIFF_FN(lambda *a: 0)
    summ = pna.DiffSummary()
    f = L.pna_gpu_diff_archive_host
    # Without a device no context can be made, so each case here also has a null ctx and returns at that check first; the other arguments'
    # checks, each on its own with a real context, are in tests/test_gpu_diff.py::test_argument_checks_with_a_context.
    assert f(None, parts, lens, 1, None, 0, src, cb, None, ctypes.byref(summ)) == PNA_E_INVAL                  # null ctx
    assert f(None, None, lens, 1, None, 0, src, cb, None, ctypes.byref(summ)) == PNA_E_INVAL                   # null parts
    assert f(None, parts, lens, 1, None, 0, ctypes.cast(None, pna.DIFF_SOURCE_FN), cb, None, None) == PNA_E_INVAL   # null source
    assert f(None, parts, lens, 1, None, 0, src, ctypes.cast(None, pna.DIFF_FN), None, None) == PNA_E_INVAL   # null cb
    assert f(None, parts, lens, 1, None, 5, src, cb, None, None) == PNA_E_INVAL                                # a length without a password
    assert L.pna_gpu_debug_diff_stats(None, None, None, None) == PNA_E_INVAL
