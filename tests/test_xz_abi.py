"""PNA_ALGO_XZ in the public interface: the constant, the prototypes, the Python binding."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header() -> str:
    with open(os.path.join(ROOT, "include", "pna_gpu.h")) as f:
        return f.read()


def test_constant_and_prototypes():
    h = header()
    assert re.search(r"^#define\s+PNA_ALGO_XZ\s+4\b", h, re.M)
    flat = re.sub(r"\s+", " ", h)
    assert ("int pna_gpu_xz_decompress_open_device(pna_gpu_ctx *ctx, const void *d_src, uint64_t src_off, uint64_t src_len, void *d_dst, "
            "uint64_t dst_off, uint64_t dst_cap, uint64_t *raw_len, void *hip_stream);") in flat
    for rule in ("LZMA2 (id 0x21)", "SHA-256", "found from the end", "lc + lp <= 4", "4 GiB or more of decoded bytes"):
        assert rule in flat, rule


def test_python_binding(pna):
    assert pna.ALGO_XZ == 4 and pna.Compression.XZ == 4
    assert "pna_gpu_xz_decompress_open_device" in pna.EXPORTS
    lib = pna.load_library()
    assert lib.pna_gpu_xz_decompress_open_device.restype is not None
    assert callable(pna.Context.xz_open_device)


def test_kernels_are_in_the_library(pna):
    """the xz launch symbols are weak references in the host code: the library must define them, or xz silently stays unsupported"""
    import subprocess
    out = subprocess.run(["nm", "-D", "--defined-only", pna.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for sym in ("launch_xzscan", "launch_lzma2", "launch_xzcheck"):
        assert sym in out, sym
