"""The .xz decoder core (csrc/xz_core.h: container walk, LZMA2 chunk walk, range decoder, CRC arithmetic -- the code the device kernels run) on the CPU,
against liblzma: built with g++ alone by tests/xz_core/Makefile, once as a shared object that this module loads, once as a stand-alone program under
-fsanitize=address,undefined that decodes the same streams plus the damaged ones (the sanitizer build is never loaded into this process)."""
import ctypes
import lzma
import os
import subprocess
import tempfile

import pytest

import xz_cases as X

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(tempfile.gettempdir(), "pna_xz_core_%d" % os.getuid())


@pytest.fixture(scope="module")
def built():
    subprocess.run(["make", "-s", "-C", os.path.join(HERE, "xz_core"), "OUT=" + OUT, "lib", "san"], check=True)
    return OUT


@pytest.fixture(scope="module")
def core(built):
    lib = ctypes.CDLL(os.path.join(built, "libxz_host.so"))
    lib.xz_host_size.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_uint64)]
    lib.xz_host_decode.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t)]

    def decode(stream):
        """(status, bytes or None): 0 decoded, 1 corrupt, 2 unsupported"""
        size = ctypes.c_uint64()
        st = lib.xz_host_size(stream, len(stream), ctypes.byref(size))
        if st:
            return st, None
        buf, got = ctypes.create_string_buffer(max(size.value, 1)), ctypes.c_size_t()
        st = lib.xz_host_decode(stream, len(stream), buf, size.value, ctypes.byref(got))
        return st, (buf.raw[:got.value] if st == 0 else None)
    return decode


def damaged():
    mixed = [s for n, s, _ in X.streams() if n == "mixed"][0]
    text = [s for n, s, _ in X.streams() if n == "text5k_p6"][0]
    out = X.damage_cases(mixed)
    out += [("trailing", text + bytes(4)), ("two_streams", text + text), ("short", text[:20]), ("none", b"")]
    for at in range(12, 36):                                    # every byte of the block header, the chunk header and the range coder's start
        b = bytearray(text)
        b[at] ^= 0x81
        out.append(("text_flip@%d" % at, bytes(b)))
    return out


def test_every_stream_equals_liblzma(core):
    for name, stream, plain in X.streams():
        assert lzma.decompress(stream) == plain, name
        assert core(stream) == (0, plain), name


def test_out_of_scope_streams_are_unsupported(core):
    for name, stream in X.unsupported():
        assert len(lzma.decompress(stream)) == 5000
        assert core(stream) == (2, None), name


def test_what_liblzma_refuses_is_refused(core):
    """equal bytes where liblzma accepts, a refusal where it refuses -- except bytes behind the footer, refused here by design"""
    for name, stream in damaged():
        st, out = core(stream)
        if X.liblzma_refuses(stream):
            assert st != 0, name
        else:
            assert (st, out) == (0, lzma.decompress(stream)), name
    assert len(X.damage_cases(b"x" * 100)) == 14
    assert all(X.liblzma_refuses(s) for _, s in damaged()[:14])


def test_sanitizer_driver(built, tmp_path):
    """the stand-alone program under ASan + UBSan over the whole list and the damaged streams: block-sized buffers, so a read or write outside a block's
    compressed bytes or decoded range, or a model index past the launch's size, stops it"""
    lines = []
    for i, (name, stream, plain) in enumerate(X.streams()):
        a, b = tmp_path / ("s%d.xz" % i), tmp_path / ("s%d.raw" % i)
        a.write_bytes(stream)
        b.write_bytes(plain)
        lines.append("%s %s" % (a, b))
    for i, (name, stream) in enumerate(damaged() + X.unsupported()):
        if not X.liblzma_refuses(stream) and (name, stream) not in X.unsupported():
            continue
        a = tmp_path / ("d%d.xz" % i)
        a.write_bytes(stream)
        lines.append("%s -" % a)
    manifest = tmp_path / "manifest"
    manifest.write_text("\n".join(lines) + "\n")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([os.path.join(built, "xz_host_san"), str(manifest)], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "%d streams, 0 failures" % len(lines) in r.stdout
