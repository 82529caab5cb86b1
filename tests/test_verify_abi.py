"""`pna verify` (pna_gpu_verify_archive_host): the public declaration, the exported symbol, and the argument checks that run before any device work."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PNA_E_INVAL = -2                                                        # include/pna_gpu.h


def test_header_declares_verify():
    h = open(os.path.join(ROOT, "include", "pna_gpu.h")).read()
    assert re.search(r"int\s+pna_gpu_verify_archive_host\s*\(", h)
    for name in ("PNA_VERIFY_FAST", "PNA_VERIFY_OK", "PNA_VERIFY_SKIPPED", "PNA_VERIFY_BAD_CRC", "PNA_VERIFY_BAD_STRUCTURE", "PNA_VERIFY_BAD_AUTH",
                 "PNA_VERIFY_BAD_DECRYPT", "PNA_VERIFY_BAD_STREAM", "PNA_VERIFY_UNSUPPORTED", "PNA_VERIFY_SIZE_HINT", "PNA_VERIFY_UNAUTHENTICATED",
                 "PNA_VERIFY_KIND_SOLID", "PNA_VERIFY_KIND_BROKEN", "pna_verify_summary", "pna_verify_fn"):
        assert name in h, name


def test_library_exports_verify(pna):
    lib = pna.load_library()
    assert "pna_gpu_verify_archive_host" in pna.EXPORTS
    getattr(lib, "pna_gpu_verify_archive_host")
    assert ctypes.sizeof(pna.VerifySummary) == 48


def test_verify_null_arguments(pna):
    L = pna.load_library()
    arc = b"\x89PNA\r\n\x1a\n" + bytes(64)
    parts = (ctypes.c_char_p * 1)(arc)
    lens = (ctypes.c_size_t * 1)(len(arc))
    cb = pna.VERIFY_FN(lambda *a: 0)
    summ = pna.VerifySummary()
    f = L.pna_gpu_verify_archive_host
    # Without a device no context can be made, so each case here also has a null ctx and returns at that check first; the other arguments'
    # checks, each on its own with a real context, are in tests/test_gpu_verify.py::test_argument_checks_with_a_context.
    assert f(None, parts, lens, 1, None, 0, 0, cb, None, ctypes.byref(summ)) == PNA_E_INVAL                 # null ctx
    assert f(None, None, lens, 1, None, 0, 0, cb, None, ctypes.byref(summ)) == PNA_E_INVAL                  # null parts
    assert f(None, parts, lens, 1, None, 0, 0, ctypes.cast(None, pna.VERIFY_FN), None, None) == PNA_E_INVAL  # null cb
    assert f(None, parts, lens, 1, None, 5, 0, cb, None, None) == PNA_E_INVAL                               # a length without a password
