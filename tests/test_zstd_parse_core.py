"""The zstd decoder's parse layer (csrc/zstd_parse_core.h: bit readers, FSE table builders, one parser per header -- the code the device kernels run) on
the CPU: tests/zstd_parse_core/zparse_host.cpp makes a small single-lane decoder of it, built with g++ alone by the Makefile beside it, once as a shared
object that this module loads, once as a stand-alone program under -fsanitize=address,undefined that decodes the same streams plus the damaged ones (the
sanitizer build is never loaded into this process).  The references are oracle/zstd_dec.c and the system libzstd (placement_cases.zstd_cpu_decode)."""
import ctypes
import os
import subprocess
import tempfile

import pytest

import placement_cases as P
import zstd_parse_cases as Z

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(tempfile.gettempdir(), "pna_zstd_parse_core_%d" % os.getuid())
NOT_ASSERTED = ("fcs_8_bytes", "nseq_3_bytes")        # a frame of 4 GiB; a block of 32 512 sequences and more: reported only
SLACK = 64                                            # what placement_cases' decoders allow a damaged stream beyond the plain text's size


@pytest.fixture(scope="module")
def built():
    subprocess.run(["make", "-s", "-C", os.path.join(HERE, "zstd_parse_core"), "OUT=" + OUT, "lib", "san"], check=True)
    return OUT


@pytest.fixture(scope="module")
def core(built):
    lib = ctypes.CDLL(os.path.join(built, "libzparse_host.so"))
    lib.zparse_host_decode.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ctypes.c_uint64)]
    lib.zparse_host_census_names.restype = ctypes.c_char_p
    names = lib.zparse_host_census_names().decode().rstrip(",").split(",")
    assert len(names) == lib.zparse_host_census_size()

    def decode(stream, cap, census=None):
        """(status, bytes or None): 0 decoded, 1 corrupt, 2 unsupported, 3 more than cap bytes; census: a dict the branch counts are added to"""
        buf, got, cen = ctypes.create_string_buffer(max(cap, 1)), ctypes.c_size_t(), (ctypes.c_uint64 * len(names))()
        st = lib.zparse_host_decode(stream, len(stream), buf, cap, ctypes.byref(got), cen)
        if census is not None:
            for k, v in zip(names, cen):
                census[k] = census.get(k, 0) + v
        return st, (buf.raw[:got.value] if st == 0 else None)
    decode.names = names
    return decode


def damaged():
    """[(name, stream, size of the undamaged plain text)]: the damage list on libzstd's level-3 stream of the 300 KiB text and on the direct-weights fixture"""
    out = []
    targets = [(n, s, d) for n, s, d in Z.fixtures() if n == "skew12x600_l3"]
    if P.have_libzstd():
        targets.insert(0, ("text300k_l3", Z.write(Z.plain("text300k"), "l3"), Z.plain("text300k")))
    for n, s, d in targets:
        out += [("%s %s" % (n, c), b, len(d)) for c, b in Z.damage_cases(s)]
    return out


def test_every_stream_decodes_to_its_plain_text(core):
    for name, stream, plain in Z.streams():
        assert P.zstd_cpu_decode(stream, len(plain)) == plain, name
        assert core(stream, len(plain)) == (0, plain), name


def test_census_every_header_branch_is_reached(core):
    """Every branch of the parsers is taken at least once by the committed streams alone (tests/golden/zstd_parse/), so that none is checked by no stream.
    Measured -- the fixtures alone / every stream of zstd_parse_cases.streams() with libzstd 1.4.8:
    frame 48/72, skippable 3/5, fcs bytes 0: 9/14, 1: 14/14, 2: 17/21, 4: 8/23, 8: 0/0, checksum 10/15, none 38/57, window byte 9/15, single segment 39/57,
    blocks raw 6/11, RLE 8/8, compressed 49/122, literals raw 24/24, RLE 1/1, Huffman 23/75, treeless 1/22, literals header raw or RLE 1 byte 11/11,
    2 bytes 5/5, 3 bytes 9/9, compressed 3 bytes 12/15, 4 bytes 7/29, 5 bytes 5/53, Huffman streams 1: 7/7, 4: 17/90, weights direct 17/17, FSE 6/58,
    sequence count 0: 1/1, 1 byte 31/32, 2 bytes 17/89, 3 bytes 0/0, modes (predefined, RLE, FSE, repeat) LL 26/26 3/3 16/78 3/14,
    OF 22/22 3/3 20/82 3/14, ML 23/23 1/1 21/83 3/14.
    The two branches no small stream reaches (an 8-byte content size: a frame of 4 GiB; a 3-byte sequence count: 32 512 sequences in a block) are
    printed with their counts and not asserted."""
    alone, every = {}, {}
    for name, stream, plain in Z.fixtures():
        assert core(stream, len(plain), alone) == (0, plain), name
    for name, stream, plain in Z.streams():
        assert core(stream, len(plain), every) == (0, plain), name
    for k in core.names:
        print("%-24s %6d %6d" % (k, alone[k], every[k]))
    assert [k for k in core.names if alone[k] < 1 and k not in NOT_ASSERTED] == []
    assert set(NOT_ASSERTED) <= set(core.names)


def test_damaged_streams_refused_or_equal_to_the_cpu_decoders(core):
    """a refusal where both CPU decoders refuse, their bytes where they decode"""
    cases = damaged()
    assert len(cases) >= 8 + 1 + 35 + 40 + 2
    for name, stream, n in cases:
        st, out = core(stream, n + SLACK)
        if P.zstd_cpu_refuses(stream, n):
            assert st != 0, name
        else:
            assert (st, out) == (0, P.zstd_cpu_decode(stream, n)), name


def test_sanitizer_driver(built, tmp_path):
    """the stand-alone program under ASan + UBSan over the whole list and the damaged streams: source and destination buffers of exactly the stream's and
    the content's size, every block copied to a buffer of its own size, so a read outside a block or a stream, a write outside the content, or a table
    index past its array stops it"""
    lines = []
    for i, (name, stream, plain) in enumerate(Z.streams()):
        a, b = tmp_path / ("s%d.zst" % i), tmp_path / ("s%d.raw" % i)
        a.write_bytes(stream)
        b.write_bytes(plain)
        lines.append("%s %s %d" % (a, b, len(plain)))
    for i, (name, stream, n) in enumerate(damaged()):
        a = tmp_path / ("d%d.zst" % i)
        a.write_bytes(stream)
        if P.zstd_cpu_refuses(stream, n):
            lines.append("%s - %d" % (a, n + SLACK))
        else:
            b = tmp_path / ("d%d.raw" % i)
            b.write_bytes(P.zstd_cpu_decode(stream, n))
            lines.append("%s %s %d" % (a, b, n + SLACK))
    manifest = tmp_path / "manifest"
    manifest.write_text("\n".join(lines) + "\n")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([os.path.join(built, "zparse_host_san"), str(manifest)], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "%d streams, 0 failures" % len(lines) in r.stdout
