"""portable-network-archive_amd -- MI355X-native per-entry compression path of PNA (host-side Python binding).

Thin ctypes layer over the C ABI of ``libpna_gpu.so`` (include/pna_gpu.h).  It mirrors the names of the reference's
seam -- ``Compression`` (lib/src/entry/options.rs:241-247), ``CompressionLevel`` defaults
(lib/src/compress/zstandard.rs:13, lib/src/compress/deflate.rs:33-38) and a ``CompressionWriter`` with
``write`` / ``flush`` / ``try_into_inner`` (lib/src/compress.rs:21-76) -- so tests read like the reference's own.

There is no CPU fallback: if the HIP extension is missing or no GPU is usable, construction raises.
(The package directory name contains a hyphen; import it with ``importlib.import_module("portable-network-archive_amd")``.)
"""
from __future__ import annotations

import collections
import ctypes
import os
from typing import Iterable, List, Optional, Sequence

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PNA_GPU_LIB") or os.path.join(_HERE, "libpna_gpu.so")

PNA_OK = 0
ALGO_STORE, ALGO_DEFLATE, ALGO_ZSTD = 0, 1, 2                   # ALGO_STORE (Compression::No): written on the device by the archive entry points -- Context.create_archive_device,
#   create_archive_chunked[_device], create_archive_encrypted, create_archive_with_metadata, create_archive_tree[_device] and the solid forms (store_stats tells which
#   form of k_store ran); create_archive(None or ctx, .., algo=ALGO_STORE) keeps the host loop; compress_batch*, compress_solid, writer, write_file and create_archive_multi refuse it
ALGO_XZ = 4                                                      # Compression::XZ: decoded everywhere; written by compress_batch* and the non-solid create_archive* on a context with set_option("xz_encode", 1)
LEVEL_DEFAULT = -1000
# error codes of include/pna_gpu.h
E_NODEVICE, E_INVAL, E_NOMEM, E_DSTSIZE, E_HIP, E_SINK, E_UNSUPPORTED = -1, -2, -3, -4, -5, -6, -7
F_HUF, F_FSE, F_LAZY, F_REP, F_DEFAULT = 1, 2, 4, 8, 0x80000000
F_FAR, F_ADOPT, F_INS2, F_STRONG = 0x10, 0x20, 0x40, 0x80
F_LZ_WAVEPARSE, F_LZ_FUSED = 0x4000, 0x8000                      # forms of the LZ stage (default: split, lane-per-region parse); same bytes
F_STD = F_HUF | F_FSE | F_LAZY | F_FAR | F_ADOPT | F_INS2          # what F_DEFAULT selects

SEG_SIZE = 1 << 20
PART_HEAD, PART_TAIL = 1, 2
BLK_SIZE = 1 << 17
SEQ_CAP = 22528


class Compression:
    """Compression::to_byte() values -- lib/src/entry/options.rs:241-247."""
    No = ALGO_STORE
    Deflate = ALGO_DEFLATE
    ZStandard = ALGO_ZSTD
    XZ = ALGO_XZ


class PnaGpuError(RuntimeError):
    def __init__(self, code: int, text: str):
        super().__init__(f"pna_gpu error {code}: {text}")
        self.code = code


class Timing(ctypes.Structure):
    _fields_ = [("ms_lz", ctypes.c_double), ("ms_stats", ctypes.c_double), ("ms_lit", ctypes.c_double),
                ("ms_seq", ctypes.c_double), ("ms_pack", ctypes.c_double), ("in_bytes", ctypes.c_uint64),
                ("out_bytes", ctypes.c_uint64), ("n_segments", ctypes.c_uint64), ("n_blocks", ctypes.c_uint64),
                ("ms_frame", ctypes.c_double), ("ms_cipher", ctypes.c_double), ("ms_lz_match", ctypes.c_double),
                ("lz_match_launches", ctypes.c_uint64), ("blk_log", ctypes.c_uint32), ("lz_units", ctypes.c_uint32)]


class DecodeForms(ctypes.Structure):
    """pna_gpu_decode_forms (include/pna_gpu.h): which forms of the decoders the latest decode call ran."""
    _fields_ = [(k, ctypes.c_uint64) for k in ("zstd_executor_frames", "zstd_workgroup_frames", "zstd_listed_entries", "inflate_lane_pieces",
                                                "inflate_lane_streams", "inflate_chunk_streams")]


ENC_NONE, ENC_AES, ENC_CAMELLIA = 0, 1, 2          # Encryption::to_byte(); ENC_CAMELLIA: written and read on a context with set_option("camellia", 1), E_UNSUPPORTED otherwise
MODE_CBC, MODE_CTR, MODE_GCM = 0, 1, 2             # CipherMode::to_byte()


class CipherStruct(ctypes.Structure):
    """pna_gpu_cipher (include/pna_gpu.h)."""
    _fields_ = [("encryption", ctypes.c_int), ("cipher_mode", ctypes.c_int), ("key", ctypes.c_uint8 * 32),
                ("phsf", ctypes.c_char_p), ("ivs", ctypes.c_void_p), ("gcm_segment_size", ctypes.c_uint32)]


class MetaStruct(ctypes.Structure):
    """pna_gpu_entry_meta (include/pna_gpu.h)."""
    _fields_ = [("extra", ctypes.POINTER(ctypes.c_void_p)), ("extra_len", ctypes.POINTER(ctypes.c_size_t)),
                ("facets", ctypes.POINTER(ctypes.c_void_p)), ("facets_len", ctypes.POINTER(ctypes.c_size_t))]


KIND_FILE, KIND_DIRECTORY, KIND_SYMLINK, KIND_HARDLINK = 0, 1, 2, 3      # DataKind::to_byte(): the kinds of the create_archive_tree* entry points


class KindsStruct(ctypes.Structure):
    """pna_gpu_entry_kinds (include/pna_gpu.h)."""
    _fields_ = [("kind", ctypes.POINTER(ctypes.c_uint8)), ("link", ctypes.POINTER(ctypes.c_void_p)), ("link_len", ctypes.POINTER(ctypes.c_size_t))]


def _kinds_struct(n: int, kinds, links):
    """(KindsStruct or None, what must stay alive): kinds None = all files; links None = the struct's link arrays stay NULL."""
    if kinds is None:
        return None, []
    ks = KindsStruct()
    a_kind = (ctypes.c_uint8 * max(n, 1))(*[int(k) for k in kinds])
    keep = [a_kind]
    ks.kind = ctypes.cast(a_kind, ctypes.POINTER(ctypes.c_uint8))
    if links is not None:
        bb = [bytes(b) if b is not None else b"" for b in links]
        arr = (ctypes.c_void_p * max(n, 1))(*[ctypes.cast(ctypes.c_char_p(b), ctypes.c_void_p) if b else None for b in bb])
        lens = (ctypes.c_size_t * max(n, 1))(*[len(b) for b in bb])
        keep += [bb, arr, lens]
        ks.link = ctypes.cast(arr, ctypes.POINTER(ctypes.c_void_p))
        ks.link_len = ctypes.cast(lens, ctypes.POINTER(ctypes.c_size_t))
    return ks, keep


def _meta_struct(n: int, extra, facets):
    """(MetaStruct or None, what must stay alive) from per-entry blobs of framed chunks (None: no such blobs)."""
    if extra is None and facets is None:
        return None, []
    ms = MetaStruct()
    keep = []
    for field, blobs in (("extra", extra), ("facets", facets)):
        if blobs is None:
            continue
        bb = [bytes(b) if b is not None else b"" for b in blobs]
        arr = (ctypes.c_void_p * max(n, 1))(*[ctypes.cast(ctypes.c_char_p(b), ctypes.c_void_p) if b else None for b in bb])
        lens = (ctypes.c_size_t * max(n, 1))(*[len(b) for b in bb])
        keep += [bb, arr, lens]
        setattr(ms, field, ctypes.cast(arr, ctypes.POINTER(ctypes.c_void_p)))
        setattr(ms, field + "_len", ctypes.cast(lens, ctypes.POINTER(ctypes.c_size_t)))
    return ms, keep


_TREE_BOUND_ARGS = [ctypes.c_int, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p]


class Cipher:
    """What WriteCipher carries (lib/src/entry/write.rs:54-57): algorithm, mode, the derived key, the PHSF string; plus the
    per-entry IVs (None = drawn by the library like random::random_vec)."""

    def __init__(self, key: bytes, phsf: str, mode: int = MODE_CTR, encryption: int = ENC_AES, ivs: Optional[bytes] = None,
                 gcm_segment_size: int = 0):
        assert len(key) == 32
        self.key, self.phsf, self.mode, self.encryption, self.ivs = bytes(key), phsf, mode, encryption, ivs
        self.gcm_segment_size = gcm_segment_size
        self._keep = None

    def struct(self, n: int) -> CipherStruct:
        c = CipherStruct()
        c.encryption, c.cipher_mode = self.encryption, self.mode
        c.key = (ctypes.c_uint8 * 32)(*self.key)
        c.phsf = self.phsf.encode()
        c.gcm_segment_size = self.gcm_segment_size
        if self.ivs is not None:
            assert len(self.ivs) >= (39 if self.mode == MODE_GCM else 16) * n
            self._keep = ctypes.create_string_buffer(bytes(self.ivs), max(len(self.ivs), 1))
            c.ivs = ctypes.cast(self._keep, ctypes.c_void_p)
        else:
            c.ivs = None
        return c


SINK_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t)
PART_SINK_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_size_t)
RAW_ENTRY_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_uint64, ctypes.c_uint64)
ENTRY_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t)
VERIFY_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_int, ctypes.c_int, ctypes.c_uint32,
                             ctypes.c_uint64, ctypes.c_char_p)

# pna_gpu_verify_archive_host (include/pna_gpu.h): flags, record statuses, record flags, record kinds
VERIFY_FAST = 1
VERIFY_OK, VERIFY_SKIPPED, VERIFY_BAD_CRC, VERIFY_BAD_STRUCTURE, VERIFY_BAD_AUTH, VERIFY_BAD_DECRYPT, VERIFY_BAD_STREAM, VERIFY_UNSUPPORTED = range(8)
VERIFY_SIZE_HINT, VERIFY_UNAUTHENTICATED = 1, 2
VERIFY_KIND_SOLID, VERIFY_KIND_BROKEN = -1, -2


class VerifySummary(ctypes.Structure):
    """pna_verify_summary (include/pna_gpu.h)."""
    _fields_ = [("total", ctypes.c_uint64), ("ok", ctypes.c_uint64), ("failed", ctypes.c_uint64), ("skipped", ctypes.c_uint64),
                ("unsupported", ctypes.c_uint64), ("unauthenticated_failure", ctypes.c_uint32), ("broken", ctypes.c_uint32)]

# pna_gpu_diff_archive_host (include/pna_gpu.h): what the host's side of an entry is, record statuses
DIFF_FS_MISSING, DIFF_FS_FILE, DIFF_FS_DIR, DIFF_FS_SYMLINK, DIFF_FS_OTHER, DIFF_FS_IGNORE = range(6)
(DIFF_SAME, DIFF_MISSING, DIFF_TYPE_MISMATCH, DIFF_SIZE_DIFFERS, DIFF_CONTENTS_DIFFER, DIFF_SYMLINK_DIFFERS, DIFF_NOT_COMPARED, DIFF_SKIPPED,
 DIFF_DAMAGED) = range(9)
DIFF_NO_OFFSET = (1 << 64) - 1                                  # first_diff of a record that has none
DIFF_TILE = 16384                                               # bytes one wave of k_diff compares (pna_dev.h DIFF_TILE)


class DiffFile(ctypes.Structure):
    """pna_diff_file (include/pna_gpu.h)."""
    _fields_ = [("fs_kind", ctypes.c_int), ("data", ctypes.c_void_p), ("len", ctypes.c_uint64)]


class DiffSummary(ctypes.Structure):
    """pna_diff_summary (include/pna_gpu.h)."""
    _fields_ = [("total", ctypes.c_uint64), ("same", ctypes.c_uint64), ("differ", ctypes.c_uint64), ("not_compared", ctypes.c_uint64),
                ("skipped", ctypes.c_uint64), ("damaged", ctypes.c_uint64), ("broken", ctypes.c_uint32), ("pad", ctypes.c_uint32)]


DIFF_SOURCE_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_int, ctypes.c_uint64, ctypes.POINTER(DiffFile))
DIFF_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_uint32,
                           ctypes.c_uint64, ctypes.c_uint64, ctypes.c_char_p)
DiffRecord = collections.namedtuple("DiffRecord", "name kind status verify_status flags size first_diff link_target")

# pna_gpu_extract_select_host (include/pna_gpu.h): destinations, record statuses, flags
EXTRACT_SKIP, EXTRACT_HOST, EXTRACT_DEVICE = range(3)
EXTRACT_OK, EXTRACT_TOO_SMALL = 0, 1
EXTRACT_CHECK_ALL = 1
EXTRACT_GAP_MAX = 65536                                         # records at most this far apart travel in one copy (PNA_EXTRACT_GAP_MAX)
EXTRACT_NO_SIZE = (1 << 64) - 1                                 # stored_size of an entry without fSIZ
PICK_TILE = 16384                                               # bytes one wave of k_pick copies (pna_dev.h PICK_TILE)


class ExtractDest(ctypes.Structure):
    """pna_extract_dest (include/pna_gpu.h)."""
    _fields_ = [("where", ctypes.c_int), ("d_dst", ctypes.c_void_p), ("cap", ctypes.c_uint64)]


class ExtractSummary(ctypes.Structure):
    """pna_extract_summary (include/pna_gpu.h)."""
    _fields_ = [("total", ctypes.c_uint64), ("selected", ctypes.c_uint64), ("to_host", ctypes.c_uint64), ("to_device", ctypes.c_uint64),
                ("too_small", ctypes.c_uint64)]


EXTRACT_SELECT_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_int, ctypes.c_uint64, ctypes.POINTER(ExtractDest))
EXTRACT_RECORD_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_uint64)

class KdfJob(ctypes.Structure):
    """pna_kdf_job (include/pna_gpu.h)."""
    _fields_ = [("kind", ctypes.c_int), ("t_cost", ctypes.c_uint32), ("m_cost_kib", ctypes.c_uint32), ("lanes", ctypes.c_uint32), ("rounds", ctypes.c_uint32),
                ("salt", ctypes.c_void_p), ("salt_len", ctypes.c_size_t)]


KDF_ARGON2D, KDF_ARGON2I, KDF_ARGON2ID_JOB, KDF_PBKDF2_SHA256_JOB = 0, 1, 2, 3      # pna_kdf_job.kind

_lib = None

EXPORTS = [
    "pna_gpu_init", "pna_gpu_set_option", "pna_gpu_shutdown", "pna_gpu_archive_chunked_bound", "pna_gpu_create_archive_chunked_device",
    "pna_gpu_create_archive_chunked_host", "pna_gpu_comm_unique_id", "pna_gpu_comm_init", "pna_gpu_comm_destroy", "pna_gpu_comm_last_error",
    "pna_gpu_host_alloc", "pna_gpu_host_free", "pna_gpu_gather_ordered", "pna_gpu_gather_ordered_start", "pna_gpu_gather_wait", "pna_gpu_gather_ticket", "pna_gpu_gather_wait_for", "pna_gather_verdict", "pna_gather_offsets", "pna_gpu_last_error", "pna_gpu_strerror", "pna_gpu_bound", "pna_gpu_clamp_level",
    "pna_gpu_compress_batch", "pna_gpu_compress_batch_device", "pna_gpu_stream_new", "pna_gpu_stream_write",
    "pna_gpu_stream_flush", "pna_gpu_stream_finish", "pna_gpu_stream_abort", "pna_gpu_compress_solid",
    "pna_gpu_last_timing", "pna_gpu_last_decode_forms", "pna_gpu_debug_block", "pna_gpu_debug_lz_stamps", "pna_bench_corpus_fill_device",
    "pna_gpu_archive_bound", "pna_gpu_create_archive_device", "pna_gpu_create_archive_host", "pna_gpu_debug_crc_schedule", "pna_gpu_debug_pinned_bytes",
    "pna_gpu_solid_archive_bound", "pna_gpu_solid_archive_enc_bound", "pna_gpu_create_solid_archive_device", "pna_gpu_create_solid_archive_host",
    "pna_gpu_create_archive_part_device", "pna_gpu_decompress_batch", "pna_gpu_decompress_batch_device",
    "pna_gpu_archive_enc_bound", "pna_gpu_create_archive_enc_device", "pna_gpu_cipher_apply_device", "pna_gpu_create_archive_enc_host",
    "pna_gpu_create_solid_archive_enc_device", "pna_gpu_create_solid_archive_enc_host", "pna_gpu_extract_archive_host", "pna_gpu_zstd_stream_frames_device",
    "pna_gpu_zstd_decompress_open_device", "pna_gpu_inflate_open_device", "pna_gpu_xz_decompress_open_device", "pna_gpu_open_size_device", "pna_gpu_create_archive_meta_device",
    "pna_gpu_create_archive_meta_host", "pna_gpu_stream_stats", "pna_bench_stream_threads",
    # include/pna_archive.h
    "pna_crc32", "pna_archive_new", "pna_archive_add_file", "pna_archive_add_dir", "pna_archive_add_solid",
    "pna_archive_inner_entry_bytes", "pna_archive_finalize", "pna_archive_abort", "pna_create_archive",
    "pna_kdf_pbkdf2_sha256", "pna_create_archive_encrypted", "pna_create_archive_encrypted_ex", "pna_create_archive_encrypted_with", "pna_kdf_derive", "pna_kdf_argon2", "pna_split_archive", "pna_join_parts",
    "pna_archive_seek_to_end", "pna_archive_list_entries",
    # streaming entries, parts, append (include/pna_gpu.h)
    "pna_gpu_create_archive_part_host", "pna_gpu_create_archive_multi_host", "pna_gpu_append_archive_host", "pna_gpu_stream_entry_begin", "pna_gpu_stream_entry_write",
    "pna_gpu_stream_entry_finish", "pna_gpu_stream_entry_abort",
    # pna verify (include/pna_gpu.h)
    "pna_gpu_verify_archive_host",
    # pna diff (include/pna_gpu.h)
    "pna_gpu_diff_archive_host", "pna_gpu_debug_diff_stats",
    # extract of chosen entries, to host or device (include/pna_gpu.h)
    "pna_gpu_extract_select_host", "pna_extract_plan_runs", "pna_gpu_debug_extract_stats", "pna_gpu_debug_pick_device",
    # key derivation on the device (include/pna_gpu.h)
    "pna_gpu_kdf_batch", "pna_phsf_parse", "pna_gpu_debug_kdf_stats", "pna_gpu_debug_store_stats",
    # entry kinds: directories, symbolic links, hard links in the create calls (include/pna_gpu.h, include/pna_archive.h)
    "pna_gpu_entry_kinds_check", "pna_gpu_archive_tree_bound", "pna_gpu_create_archive_tree_device", "pna_gpu_create_archive_tree_host",
    "pna_gpu_solid_archive_tree_bound", "pna_gpu_create_solid_archive_tree_device", "pna_gpu_create_solid_archive_tree_host", "pna_archive_entry_record_bytes",
]


def load_library() -> ctypes.CDLL:
    """dlopen libpna_gpu.so (built in-tree by __graft_entry__.build()).  Fails loudly when it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(there is no CPU fallback for the compression path)")
    try:  # share PyTorch's HIP runtime when torch is used in the same process
        import torch  # noqa: F401
    except Exception:  # pragma: no cover - torch is optional for the C ABI itself
        pass
    L = ctypes.CDLL(LIB_PATH)
    vp, sz, u32, u64p = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint64)
    L.pna_gpu_init.restype = ctypes.c_int
    L.pna_gpu_init.argtypes = [ctypes.POINTER(vp), ctypes.c_int, u32]
    L.pna_gpu_shutdown.restype = None
    L.pna_gpu_shutdown.argtypes = [vp]
    L.pna_gpu_last_error.restype = ctypes.c_char_p
    L.pna_gpu_last_error.argtypes = [vp]
    L.pna_gpu_strerror.restype = ctypes.c_char_p
    L.pna_gpu_strerror.argtypes = [ctypes.c_int]
    L.pna_gpu_bound.restype = sz
    L.pna_gpu_bound.argtypes = [ctypes.c_int, sz]
    L.pna_gpu_clamp_level.restype = ctypes.c_int
    L.pna_gpu_clamp_level.argtypes = [ctypes.c_int, ctypes.c_int]
    L.pna_gpu_compress_batch.restype = ctypes.c_int
    L.pna_gpu_compress_batch.argtypes = [vp, ctypes.c_int, ctypes.c_int, sz, ctypes.POINTER(vp), ctypes.POINTER(sz),
                                         ctypes.POINTER(vp), ctypes.POINTER(sz), ctypes.POINTER(sz)]
    L.pna_gpu_compress_batch_device.restype = ctypes.c_int
    L.pna_gpu_compress_batch_device.argtypes = [vp, ctypes.c_int, ctypes.c_int, sz, vp, u64p, u64p, vp, sz, u64p, vp]
    L.pna_gpu_archive_bound.restype = sz
    L.pna_gpu_archive_bound.argtypes = [ctypes.c_int, sz, ctypes.POINTER(ctypes.c_char_p), u64p]
    L.pna_gpu_create_archive_device.restype = ctypes.c_int
    L.pna_gpu_create_archive_device.argtypes = [vp, ctypes.c_int, ctypes.c_int, sz, ctypes.POINTER(ctypes.c_char_p), vp, u64p, u64p,
                                                vp, sz, u64p, u64p, vp]
    L.pna_gpu_create_archive_part_device.restype = ctypes.c_int
    L.pna_gpu_create_archive_part_device.argtypes = [vp, ctypes.c_int, ctypes.c_int, sz, ctypes.POINTER(ctypes.c_char_p), vp, u64p, u64p,
                                                     vp, sz, u64p, u64p, u32, vp]
    L.pna_gpu_archive_enc_bound.restype = sz
    L.pna_gpu_archive_enc_bound.argtypes = [ctypes.c_int, sz, ctypes.POINTER(ctypes.c_char_p), u64p, ctypes.POINTER(CipherStruct)]
    L.pna_gpu_create_archive_enc_device.restype = ctypes.c_int
    L.pna_gpu_create_archive_enc_device.argtypes = [vp, ctypes.c_int, ctypes.c_int, sz, ctypes.POINTER(ctypes.c_char_p), vp, u64p, u64p,
                                                    ctypes.POINTER(CipherStruct), vp, sz, u64p, u64p, u32, vp]
    L.pna_gpu_cipher_apply_device.restype = ctypes.c_int
    L.pna_gpu_cipher_apply_device.argtypes = [vp, ctypes.POINTER(CipherStruct), ctypes.c_int, sz, vp, u64p, u64p, vp]
    L.pna_gpu_decompress_batch.restype = ctypes.c_int
    L.pna_gpu_decompress_batch.argtypes = [vp, ctypes.c_int, sz, ctypes.POINTER(vp), ctypes.POINTER(sz), ctypes.POINTER(vp), ctypes.POINTER(sz)]
    L.pna_gpu_decompress_batch_device.restype = ctypes.c_int
    L.pna_gpu_decompress_batch_device.argtypes = [vp, ctypes.c_int, sz, vp, u64p, u64p, vp, u64p, u64p, vp]
    L.pna_gpu_solid_archive_bound.restype = sz
    L.pna_gpu_solid_archive_bound.argtypes = [ctypes.c_int, sz, ctypes.POINTER(ctypes.c_char_p), u64p]
    L.pna_gpu_solid_archive_enc_bound.restype = sz
    L.pna_gpu_solid_archive_enc_bound.argtypes = [ctypes.c_int, sz, ctypes.POINTER(ctypes.c_char_p), u64p, ctypes.POINTER(CipherStruct)]
    L.pna_gpu_create_solid_archive_device.restype = ctypes.c_int
    L.pna_gpu_create_solid_archive_device.argtypes = [vp, ctypes.c_int, ctypes.c_int, sz, ctypes.POINTER(ctypes.c_char_p), vp, u64p, u64p,
                                                      vp, sz, u64p, vp]
    L.pna_gpu_create_solid_archive_enc_device.restype = ctypes.c_int
    L.pna_gpu_create_solid_archive_enc_device.argtypes = [vp, ctypes.c_int, ctypes.c_int, sz, ctypes.POINTER(ctypes.c_char_p), vp, u64p, u64p,
                                                          ctypes.POINTER(CipherStruct), vp, sz, u64p, vp]
    L.pna_gpu_debug_crc_schedule.restype = ctypes.c_uint32
    L.pna_gpu_debug_crc_schedule.argtypes = [ctypes.c_char_p, sz]
    L.pna_gpu_stream_new.restype = ctypes.c_int
    L.pna_gpu_stream_new.argtypes = [vp, ctypes.c_int, ctypes.c_int, SINK_FN, vp, ctypes.POINTER(vp)]
    L.pna_gpu_stream_write.restype = ctypes.c_int
    L.pna_gpu_stream_write.argtypes = [vp, ctypes.c_char_p, sz]
    L.pna_gpu_stream_flush.restype = ctypes.c_int
    L.pna_gpu_stream_flush.argtypes = [vp]
    L.pna_gpu_stream_finish.restype = ctypes.c_int
    L.pna_gpu_stream_finish.argtypes = [vp]
    L.pna_gpu_stream_abort.restype = None
    L.pna_gpu_stream_abort.argtypes = [vp]
    L.pna_gpu_stream_stats.restype = ctypes.c_int
    L.pna_gpu_stream_stats.argtypes = [vp, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)]
    L.pna_bench_stream_threads.restype = ctypes.c_double
    L.pna_bench_stream_threads.argtypes = [vp, ctypes.c_int, ctypes.c_int, ctypes.c_uint, sz, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(sz),
                                           ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_int)]
    L.pna_gpu_compress_solid.restype = ctypes.c_int
    L.pna_gpu_compress_solid.argtypes = [vp, ctypes.c_int, ctypes.c_int, ctypes.c_char_p, sz, SINK_FN, vp]
    L.pna_gpu_last_timing.restype = ctypes.c_int
    L.pna_gpu_last_timing.argtypes = [vp, ctypes.POINTER(Timing)]
    L.pna_gpu_last_decode_forms.restype = ctypes.c_int
    L.pna_gpu_last_decode_forms.argtypes = [vp, ctypes.POINTER(DecodeForms)]
    L.pna_gpu_debug_block.restype = ctypes.c_int
    L.pna_gpu_debug_block.argtypes = [vp, u32, u64p, u32, ctypes.POINTER(u32), ctypes.c_char_p, u32, ctypes.POINTER(u32)]
    L.pna_gpu_debug_lz_stamps.restype = ctypes.c_int
    L.pna_gpu_debug_lz_stamps.argtypes = [vp, ctypes.POINTER(ctypes.c_ulonglong)]
    L.pna_bench_corpus_fill_device.restype = ctypes.c_int
    L.pna_bench_corpus_fill_device.argtypes = [vp, ctypes.c_int, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64,
                                               ctypes.c_uint64, vp, vp]
    L.pna_crc32.restype = ctypes.c_uint32
    L.pna_crc32.argtypes = [ctypes.c_uint32, ctypes.c_char_p, sz]
    L.pna_archive_new.restype = ctypes.c_int
    L.pna_archive_new.argtypes = [SINK_FN, vp, u32, ctypes.POINTER(vp)]
    L.pna_archive_add_file.restype = ctypes.c_int
    L.pna_archive_add_file.argtypes = [vp, ctypes.c_char_p, ctypes.c_int, ctypes.c_int64, ctypes.c_char_p, sz, u32]
    L.pna_archive_add_dir.restype = ctypes.c_int
    L.pna_archive_add_dir.argtypes = [vp, ctypes.c_char_p]
    L.pna_archive_add_solid.restype = ctypes.c_int
    L.pna_archive_add_solid.argtypes = [vp, ctypes.c_int, ctypes.POINTER(vp), ctypes.POINTER(sz), sz]
    L.pna_archive_inner_entry_bytes.restype = sz
    L.pna_archive_inner_entry_bytes.argtypes = [ctypes.c_char_p, ctypes.c_char_p, sz, vp, sz]
    L.pna_archive_finalize.restype = ctypes.c_int
    L.pna_archive_finalize.argtypes = [vp]
    L.pna_archive_abort.restype = None
    L.pna_archive_abort.argtypes = [vp]
    L.pna_create_archive.restype = ctypes.c_int
    L.pna_create_archive.argtypes = [vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, sz, ctypes.POINTER(ctypes.c_char_p),
                                     ctypes.POINTER(vp), ctypes.POINTER(sz), SINK_FN, vp]
    L.pna_gpu_create_archive_enc_host.restype = ctypes.c_int
    L.pna_gpu_create_archive_enc_host.argtypes = [vp, ctypes.c_int, ctypes.c_int, sz, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(vp),
                                                  ctypes.POINTER(sz), ctypes.POINTER(CipherStruct), SINK_FN, vp]
    L.pna_gpu_create_archive_meta_host.restype = ctypes.c_int
    L.pna_gpu_create_archive_meta_host.argtypes = [vp, ctypes.c_int, ctypes.c_int, sz, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(vp),
                                                   ctypes.POINTER(sz), ctypes.POINTER(CipherStruct), ctypes.POINTER(MetaStruct), SINK_FN, vp]
    L.pna_gpu_extract_archive_host.restype = ctypes.c_int
    L.pna_gpu_extract_archive_host.argtypes = [vp, ctypes.c_char_p, sz, ctypes.c_char_p, sz, ENTRY_FN, vp]
    L.pna_gpu_verify_archive_host.restype = ctypes.c_int
    L.pna_gpu_verify_archive_host.argtypes = [vp, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(sz), sz, ctypes.c_char_p, sz, ctypes.c_uint32,
                                              VERIFY_FN, vp, ctypes.POINTER(VerifySummary)]
    L.pna_gpu_diff_archive_host.restype = ctypes.c_int
    L.pna_gpu_diff_archive_host.argtypes = [vp, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(sz), sz, ctypes.c_char_p, sz, DIFF_SOURCE_FN, DIFF_FN, vp,
                                            ctypes.POINTER(DiffSummary)]
    L.pna_gpu_debug_diff_stats.restype = ctypes.c_int
    L.pna_gpu_debug_diff_stats.argtypes = [vp, u64p, u64p, ctypes.POINTER(ctypes.c_double)]
    L.pna_gpu_extract_select_host.restype = ctypes.c_int
    L.pna_gpu_extract_select_host.argtypes = [vp, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(sz), sz, ctypes.c_char_p, sz, ctypes.c_uint32,
                                              EXTRACT_SELECT_FN, EXTRACT_RECORD_FN, vp, ctypes.POINTER(ExtractSummary)]
    L.pna_extract_plan_runs.restype = ctypes.c_int
    L.pna_extract_plan_runs.argtypes = [u64p, u64p, ctypes.POINTER(ctypes.c_uint8), sz, ctypes.c_uint64, u64p, u64p, ctypes.POINTER(sz)]
    L.pna_gpu_kdf_batch.restype = ctypes.c_int
    L.pna_gpu_kdf_batch.argtypes = [vp, ctypes.c_char_p, sz, sz, ctypes.POINTER(KdfJob), ctypes.c_char_p, ctypes.POINTER(ctypes.c_int), vp]
    L.pna_phsf_parse.restype = ctypes.c_int
    L.pna_phsf_parse.argtypes = [ctypes.c_char_p, sz, ctypes.POINTER(KdfJob), ctypes.c_char_p, sz, ctypes.POINTER(sz)]
    L.pna_gpu_debug_kdf_stats.restype = ctypes.c_int
    L.pna_gpu_debug_kdf_stats.argtypes = [vp, u64p, u64p, u64p, ctypes.POINTER(ctypes.c_double)]
    L.pna_gpu_debug_store_stats.restype = ctypes.c_int
    L.pna_gpu_debug_store_stats.argtypes = [vp, u64p, u64p, u64p, ctypes.POINTER(ctypes.c_double)]
    L.pna_gpu_debug_extract_stats.restype = ctypes.c_int
    L.pna_gpu_debug_extract_stats.argtypes = [vp, u64p, u64p, u64p, u64p, ctypes.POINTER(ctypes.c_double)]
    L.pna_gpu_debug_pick_device.restype = ctypes.c_int
    L.pna_gpu_debug_pick_device.argtypes = [vp, sz, vp, u64p, ctypes.POINTER(vp), u64p, vp]
    L.pna_gpu_open_size_device.restype = ctypes.c_int
    L.pna_gpu_open_size_device.argtypes = [vp, ctypes.c_int, vp, ctypes.c_uint64, ctypes.c_uint64, u64p, ctypes.POINTER(ctypes.c_int), vp]
    L.pna_gpu_inflate_open_device.restype = ctypes.c_int
    L.pna_gpu_inflate_open_device.argtypes = [vp, vp, ctypes.c_uint64, ctypes.c_uint64, vp, ctypes.c_uint64, ctypes.c_uint64, u64p, vp]
    L.pna_gpu_xz_decompress_open_device.restype = ctypes.c_int
    L.pna_gpu_xz_decompress_open_device.argtypes = [vp, vp, ctypes.c_uint64, ctypes.c_uint64, vp, ctypes.c_uint64, ctypes.c_uint64, u64p, vp]
    L.pna_kdf_pbkdf2_sha256.restype = ctypes.c_int
    L.pna_kdf_pbkdf2_sha256.argtypes = [ctypes.c_char_p, sz, ctypes.c_char_p, sz, u32, ctypes.c_char_p, sz, ctypes.c_char_p, sz]
    L.pna_split_archive.restype = ctypes.c_int
    L.pna_split_archive.argtypes = [ctypes.c_char_p, sz, sz, PART_SINK_FN, vp, ctypes.POINTER(u32)]
    L.pna_join_parts.restype = ctypes.c_int
    L.pna_join_parts.argtypes = [ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(sz), sz, SINK_FN, vp]
    L.pna_kdf_argon2.restype = ctypes.c_int
    L.pna_kdf_argon2.argtypes = [ctypes.c_int, ctypes.c_char_p, sz, ctypes.c_char_p, sz, u32, u32, u32, ctypes.c_char_p, sz]
    L.pna_create_archive_encrypted.restype = ctypes.c_int
    L.pna_create_archive_encrypted.argtypes = [vp, ctypes.c_int, ctypes.c_int, sz, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(vp),
                                               ctypes.POINTER(sz), ctypes.c_char_p, sz, ctypes.c_int, u32, SINK_FN, vp]
    L.pna_create_archive_encrypted_ex.restype = ctypes.c_int
    L.pna_create_archive_encrypted_ex.argtypes = [vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, sz, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(vp),
                                                  ctypes.POINTER(sz), ctypes.c_char_p, sz, ctypes.c_int, ctypes.c_int, u32, SINK_FN, vp]
    L.pna_create_archive_encrypted_with.restype = ctypes.c_int
    L.pna_create_archive_encrypted_with.argtypes = [vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, sz, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(vp),
                                                    ctypes.POINTER(sz), ctypes.c_char_p, sz, ctypes.c_int, ctypes.c_int, ctypes.c_int, u32, SINK_FN, vp]
    L.pna_kdf_derive.restype = ctypes.c_int
    L.pna_kdf_derive.argtypes = [ctypes.c_int, ctypes.c_char_p, sz, ctypes.c_char_p, sz, u32, ctypes.c_char_p, ctypes.c_char_p, sz]
    L.pna_gpu_create_solid_archive_enc_host.restype = ctypes.c_int
    L.pna_gpu_create_solid_archive_enc_host.argtypes = [vp, ctypes.c_int, ctypes.c_int, sz, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(vp),
                                                        ctypes.POINTER(sz), ctypes.POINTER(CipherStruct), SINK_FN, vp]
    L.pna_archive_seek_to_end.restype = ctypes.c_int
    L.pna_archive_seek_to_end.argtypes = [ctypes.c_char_p, sz, u64p, ctypes.POINTER(ctypes.c_int)]
    L.pna_archive_list_entries.restype = ctypes.c_int
    L.pna_archive_list_entries.argtypes = [ctypes.c_char_p, sz, RAW_ENTRY_FN, vp]
    L.pna_gpu_create_archive_part_host.restype = ctypes.c_int
    L.pna_gpu_create_archive_part_host.argtypes = [vp, ctypes.c_int, ctypes.c_int, sz, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(vp),
                                                   ctypes.POINTER(sz), u32, SINK_FN, vp]
    L.pna_gpu_create_archive_multi_host.restype = ctypes.c_int
    L.pna_gpu_create_archive_multi_host.argtypes = [ctypes.POINTER(vp), sz, ctypes.c_int, ctypes.c_int, sz, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(vp),
                                                    ctypes.POINTER(sz), SINK_FN, vp]
    L.pna_gpu_append_archive_host.restype = ctypes.c_int
    L.pna_gpu_append_archive_host.argtypes = [vp, ctypes.c_int, ctypes.c_int, ctypes.c_char_p, sz, sz, ctypes.POINTER(ctypes.c_char_p),
                                              ctypes.POINTER(vp), ctypes.POINTER(sz), u64p, SINK_FN, vp]
    L.pna_gpu_stream_entry_begin.restype = ctypes.c_int
    L.pna_gpu_stream_entry_begin.argtypes = [vp, ctypes.c_int, ctypes.c_int, ctypes.c_char_p, ctypes.c_char_p, sz, u32, SINK_FN, vp, ctypes.POINTER(vp)]
    L.pna_gpu_stream_entry_write.restype = ctypes.c_int
    L.pna_gpu_stream_entry_write.argtypes = [vp, ctypes.c_char_p, sz]
    L.pna_gpu_stream_entry_finish.restype = ctypes.c_int
    L.pna_gpu_stream_entry_finish.argtypes = [vp]
    L.pna_gpu_stream_entry_abort.restype = None
    L.pna_gpu_stream_entry_abort.argtypes = [vp]
    _lib = L
    return L


def bound(algo: int, n: int) -> int:
    return load_library().pna_gpu_bound(algo, n)


def clamp_level(algo: int, level: int = LEVEL_DEFAULT) -> int:
    """From<CompressionLevel> mappings -- compress/zstandard.rs:43-57, compress/deflate.rs:89-101, compress/xz.rs:36-46."""
    return load_library().pna_gpu_clamp_level(algo, level)


class Context:
    """One GPU context (pna_gpu_init).  Raises PnaGpuError(PNA_E_NODEVICE) without a usable MI355X."""

    def __init__(self, device: int = 0, flags: int = F_DEFAULT):
        self._L = load_library()
        h = ctypes.c_void_p()
        rc = self._L.pna_gpu_init(ctypes.byref(h), device, flags)
        if rc != PNA_OK:
            raise PnaGpuError(rc, self._L.pna_gpu_strerror(rc).decode())
        self._h = h

    def close(self) -> None:
        if getattr(self, "_h", None):
            self._L.pna_gpu_shutdown(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc: int) -> None:
        if rc != PNA_OK:
            raise PnaGpuError(rc, self._L.pna_gpu_last_error(self._h).decode() or self._L.pna_gpu_strerror(rc).decode())

    # ---- batch of independent entries (host buffers)
    def compress_batch(self, entries: Sequence[bytes], algo: int = ALGO_ZSTD, level: int = LEVEL_DEFAULT) -> List[bytes]:
        n = len(entries)
        if n == 0:
            return []
        srcs = [e if isinstance(e, bytes) else bytes(e) for e in entries]       # passed by pointer, not copied
        caps = [self._L.pna_gpu_bound(algo, len(e)) for e in srcs]
        arena = bytearray(sum(caps) + 1)                                        # one output arena, entry i at offs[i]
        base = ctypes.addressof((ctypes.c_char * len(arena)).from_buffer(arena))
        offs, pos = [], 0
        for c in caps:
            offs.append(pos); pos += c
        vp, sz = ctypes.c_void_p, ctypes.c_size_t
        a_src = (vp * n)(*[ctypes.cast(ctypes.c_char_p(b), vp) for b in srcs])
        a_len = (sz * n)(*[len(e) for e in srcs])
        a_dst = (vp * n)(*[base + o for o in offs])
        a_cap = (sz * n)(*caps)
        a_out = (sz * n)()
        self._check(self._L.pna_gpu_compress_batch(self._h, algo, level, n, a_src, a_len, a_dst, a_cap, a_out))
        mv = memoryview(arena)
        return [bytes(mv[offs[i]:offs[i] + a_out[i]]) for i in range(n)]

    # ---- batch resident in HBM (raw device pointers; torch tensors via .data_ptr())
    def compress_batch_device(self, d_src: int, src_off: Sequence[int], src_len: Sequence[int], d_dst: int, dst_cap: int,
                              algo: int = ALGO_ZSTD, level: int = LEVEL_DEFAULT, stream: int = 0) -> List[int]:
        n = len(src_len)
        a_off = (ctypes.c_uint64 * (n + 1))(*src_off) if len(src_off) == n + 1 else (ctypes.c_uint64 * (n + 1))(*list(src_off), 0)
        a_len = (ctypes.c_uint64 * max(n, 1))(*src_len)
        a_out = (ctypes.c_uint64 * (n + 1))()
        self._check(self._L.pna_gpu_compress_batch_device(self._h, algo, level, n, ctypes.c_void_p(d_src), a_off, a_len,
                                                          ctypes.c_void_p(d_dst), dst_cap, a_out,
                                                          ctypes.c_void_p(stream) if stream else None))
        return list(a_out)

    def create_archive_device(self, names: Sequence[str], d_src: int, src_off: Sequence[int], src_len: Sequence[int], d_dst: int,
                              dst_cap: int, algo: int = ALGO_ZSTD, level: int = LEVEL_DEFAULT, stream: int = 0,
                              _cache: Optional[dict] = None, part: int = PART_HEAD | PART_TAIL, cipher: Optional[Cipher] = None,
                              want_offsets: bool = True):
        """Whole non-solid archive assembled in HBM (pna_gpu_create_archive_enc_device; `part` selects whether this shard
        carries the archive header / AEND; `cipher` adds the AES stage between compression and chunk CRC).
        Returns (archive_len, entry_off)."""
        n = len(src_len)
        if _cache is not None and "a" in _cache:
            a_names, a_off, a_len = _cache["a"]
        else:
            a_names = (ctypes.c_char_p * max(n, 1))(*[s.encode() for s in names])
            a_off = (ctypes.c_uint64 * (n + 1))(*(list(src_off)[:n] + [0]))
            a_len = (ctypes.c_uint64 * max(n, 1))(*src_len)
            if _cache is not None:
                _cache["a"] = (a_names, a_off, a_len)
        if _cache is not None and "out" in _cache:
            a_out = _cache["out"]
        else:
            a_out = (ctypes.c_uint64 * (n + 1))()
            if _cache is not None:
                _cache["out"] = a_out
        total = ctypes.c_uint64()
        if cipher is not None and _cache is not None:
            cs = _cache.get("cs") or _cache.setdefault("cs", cipher.struct(n))
        else:
            cs = cipher.struct(n) if cipher is not None else None
        self._check(self._L.pna_gpu_create_archive_enc_device(self._h, algo, level, n, a_names, ctypes.c_void_p(d_src), a_off, a_len,
                                                              ctypes.byref(cs) if cs is not None else None,
                                                              ctypes.c_void_p(d_dst), dst_cap, a_out, ctypes.byref(total), part,
                                                              ctypes.c_void_p(stream) if stream else None))
        return total.value, (list(a_out) if want_offsets else None)      # the list conversion costs milliseconds for 10^5 entries

    def open_size_device(self, d_src: int, src_off: int, src_len: int, algo: int = ALGO_ZSTD, stream: int = 0):
        """The decoded size of one zstd / zlib / xz / stored stream in device memory whose size is recorded nowhere (pna_gpu_open_size_device):
        (size, exact) -- exact False: a proven upper bound (zstd frames without a content size); an xz stream's size is the sum of its Index records, always exact."""
        size, exact = ctypes.c_uint64(), ctypes.c_int()
        self._check(self._L.pna_gpu_open_size_device(self._h, algo, ctypes.c_void_p(d_src), src_off, src_len, ctypes.byref(size), ctypes.byref(exact),
                                                     ctypes.c_void_p(stream) if stream else None))
        return size.value, bool(exact.value)

    def inflate_open_device(self, d_src: int, src_off: int, src_len: int, d_dst: int, dst_off: int, dst_cap: int, stream: int = 0) -> int:
        """One zlib stream in device memory whose size is recorded nowhere, decoded into dst_cap bytes of room (pna_gpu_inflate_open_device).
        Returns the decoded size."""
        raw = ctypes.c_uint64()
        self._check(self._L.pna_gpu_inflate_open_device(self._h, ctypes.c_void_p(d_src), src_off, src_len, ctypes.c_void_p(d_dst), dst_off, dst_cap,
                                                        ctypes.byref(raw), ctypes.c_void_p(stream) if stream else None))
        return raw.value

    def xz_open_device(self, d_src: int, src_off: int, src_len: int, d_dst: int, dst_off: int, dst_cap: int, stream: int = 0) -> int:
        """One .xz stream in device memory whose size is recorded nowhere, decoded into dst_cap bytes of room (pna_gpu_xz_decompress_open_device).
        Returns the decoded size."""
        raw = ctypes.c_uint64()
        self._check(self._L.pna_gpu_xz_decompress_open_device(self._h, ctypes.c_void_p(d_src), src_off, src_len, ctypes.c_void_p(d_dst), dst_off, dst_cap,
                                                              ctypes.byref(raw), ctypes.c_void_p(stream) if stream else None))
        return raw.value

    def cipher_apply_device(self, cipher: Cipher, d_buf: int, off: Sequence[int], length: Sequence[int], decrypt: bool = False,
                            stream: int = 0) -> None:
        """The cipher stage alone, in place, over byte ranges of a device buffer (range i uses cipher.ivs[16 i ..))."""
        n = len(length)
        cs = cipher.struct(n)
        mk = lambda xs: (ctypes.c_uint64 * max(n, 1))(*list(xs)[:n])
        self._check(self._L.pna_gpu_cipher_apply_device(self._h, ctypes.byref(cs), 1 if decrypt else 0, n, ctypes.c_void_p(d_buf),
                                                        mk(off), mk(length), ctypes.c_void_p(stream) if stream else None))

    def create_solid_archive_device(self, names: Sequence[str], d_src: int, src_off: Sequence[int], src_len: Sequence[int], d_dst: int,
                                    dst_cap: int, algo: int = ALGO_ZSTD, level: int = LEVEL_DEFAULT, stream: int = 0,
                                    _cache: Optional[dict] = None, cipher: Optional[Cipher] = None) -> int:
        """`pna create --solid` assembled in HBM (pna_gpu_create_solid_archive_enc_device; `cipher`: CTR with one IV, or GCM with one salt || nonce prefix).
        Returns the archive length."""
        n = len(src_len)
        if _cache is not None and "a" in _cache:
            a_names, a_off, a_len = _cache["a"]
        else:
            a_names = (ctypes.c_char_p * max(n, 1))(*[s.encode() for s in names])
            a_off = (ctypes.c_uint64 * (n + 1))(*(list(src_off)[:n] + [0]))
            a_len = (ctypes.c_uint64 * max(n, 1))(*src_len)
            if _cache is not None:
                _cache["a"] = (a_names, a_off, a_len)
        total = ctypes.c_uint64()
        cs = cipher.struct(1) if cipher is not None else None
        self._check(self._L.pna_gpu_create_solid_archive_enc_device(self._h, algo, level, n, a_names, ctypes.c_void_p(d_src), a_off, a_len,
                                                                    ctypes.byref(cs) if cs is not None else None,
                                                                    ctypes.c_void_p(d_dst), dst_cap, ctypes.byref(total),
                                                                    ctypes.c_void_p(stream) if stream else None))
        return total.value

    def create_solid_archive_enc_host(self, names: Sequence[str], entries: Sequence[bytes], algo: int = ALGO_ZSTD, level: int = LEVEL_DEFAULT,
                                      cipher: Optional[Cipher] = None) -> bytes:
        """`pna create --solid` from host memory with the caller's key and IV (pna_gpu_create_solid_archive_enc_host): streamed in windows of
        solid_win_mib MiB; CTR with one IV, GCM with one salt || nonce prefix; the bytes of create_solid_archive_device with the same cipher.
        cipher None: create_archive(..., solid=True)."""
        n = len(entries)
        out = bytearray()

        def _sink(_u, buf, k):
            out.extend((ctypes.c_char * k).from_address(buf))
            return 0
        cb = SINK_FN(_sink)
        bufs = [e if isinstance(e, (bytes, memoryview)) else bytes(e) for e in entries]
        ptrs = []
        for b in bufs:                                                  # bytes, or a writable / numpy-backed memoryview (no copy of large entries)
            if isinstance(b, bytes):
                ptrs.append(ctypes.cast(ctypes.c_char_p(b), ctypes.c_void_p))
            else:
                ptrs.append(ctypes.c_void_p(ctypes.addressof(ctypes.c_char.from_buffer(b)) if len(b) else 0))
        a_names = (ctypes.c_char_p * max(n, 1))(*[s.encode() for s in names])
        a_src = (ctypes.c_void_p * max(n, 1))(*ptrs)
        a_len = (ctypes.c_size_t * max(n, 1))(*[len(e) for e in bufs])
        cs = cipher.struct(1) if cipher is not None else None
        self._check(self._L.pna_gpu_create_solid_archive_enc_host(self._h, algo, level, n, a_names, a_src, a_len,
                                                                  ctypes.byref(cs) if cs is not None else None, cb, None))
        return bytes(out)

    def decompress_batch(self, payloads: Sequence[bytes], raw_sizes: Sequence[int], algo: int = ALGO_ZSTD) -> List[bytes]:
        """decompress_reader for a batch of entries: payload i (concatenated FDAT bodies) -> raw_sizes[i] bytes (algo: ALGO_ZSTD, ALGO_DEFLATE, ALGO_XZ)."""
        n = len(payloads)
        keep = [p if isinstance(p, bytes) else bytes(p) for p in payloads]
        outs = [ctypes.create_string_buffer(max(r, 1)) for r in raw_sizes]
        a_src = (ctypes.c_void_p * max(n, 1))(*[ctypes.cast(ctypes.c_char_p(b), ctypes.c_void_p) for b in keep])
        a_sl = (ctypes.c_size_t * max(n, 1))(*[len(b) for b in keep])
        a_dst = (ctypes.c_void_p * max(n, 1))(*[ctypes.cast(o, ctypes.c_void_p) for o in outs])
        a_rl = (ctypes.c_size_t * max(n, 1))(*raw_sizes)
        self._check(self._L.pna_gpu_decompress_batch(self._h, algo, n, a_src, a_sl, a_dst, a_rl))
        return [o.raw[:r] for o, r in zip(outs, raw_sizes)]

    def decompress_batch_device(self, d_src: int, src_off: Sequence[int], src_len: Sequence[int], d_dst: int, dst_off: Sequence[int],
                                raw_len: Sequence[int], algo: int = ALGO_ZSTD, stream: int = 0) -> None:
        n = len(src_len)
        mk = lambda xs: (ctypes.c_uint64 * max(n, 1))(*list(xs)[:n])
        self._check(self._L.pna_gpu_decompress_batch_device(self._h, algo, n, ctypes.c_void_p(d_src), mk(src_off), mk(src_len),
                                                            ctypes.c_void_p(d_dst), mk(dst_off), mk(raw_len),
                                                            ctypes.c_void_p(stream) if stream else None))

    def create_archive_chunked_device(self, names: Sequence[str], d_src: int, src_off: Sequence[int], src_len: Sequence[int], d_dst: int, dst_cap: int,
                                      max_chunk_size: int, algo: int = ALGO_ZSTD, level: int = LEVEL_DEFAULT, cipher: Optional[Cipher] = None,
                                      part: int = PART_HEAD | PART_TAIL):
        """pna_gpu_create_archive_chunked_device: the archive in HBM with FDAT chunks of at most max_chunk_size bytes.  Returns (archive_len, entry_off)."""
        n = len(src_len)
        a_names = (ctypes.c_char_p * max(n, 1))(*[s.encode() for s in names])
        a_off = (ctypes.c_uint64 * (n + 1))(*(list(src_off)[:n] + [0]))
        a_len = (ctypes.c_uint64 * max(n, 1))(*src_len)
        a_out = (ctypes.c_uint64 * (n + 1))()
        total = ctypes.c_uint64()
        cs = cipher.struct(n) if cipher is not None else None
        f = self._L.pna_gpu_create_archive_chunked_device
        f.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                      ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p]
        self._check(f(self._h, algo, level, n, a_names, ctypes.c_void_p(d_src), a_off, a_len, ctypes.byref(cs) if cs is not None else None, None,
                      max_chunk_size, ctypes.c_void_p(d_dst), dst_cap, a_out, ctypes.byref(total), part, None))
        return total.value, list(a_out)

    def create_archive_tree_device(self, names: Sequence[str], d_src: int, src_off: Sequence[int], src_len: Sequence[int], d_dst: int, dst_cap: int,
                                   kinds=None, links=None, algo: int = ALGO_ZSTD, level: int = LEVEL_DEFAULT, cipher: Optional[Cipher] = None,
                                   facets=None, extra=None, max_chunk_size: int = 0, solid: bool = False, part: int = PART_HEAD | PART_TAIL):
        """pna_gpu_create_archive_tree_device / pna_gpu_create_solid_archive_tree_device: the archive in HBM with directories (KIND_DIRECTORY), symbolic
        links and hard links (KIND_SYMLINK, KIND_HARDLINK: links[i] = the target's bytes) between the files, in the order given.  An entry that is not a
        file has src_len[i] == 0.  Returns (archive_len, entry_off); entry_off is None for a solid archive."""
        n = len(src_len)
        a_names = (ctypes.c_char_p * max(n, 1))(*[s.encode() for s in names])
        a_off = (ctypes.c_uint64 * (n + 1))(*(list(src_off)[:n] + [0]))
        a_len = (ctypes.c_uint64 * max(n, 1))(*src_len)
        a_out = (ctypes.c_uint64 * (n + 1))()
        total = ctypes.c_uint64()
        cs = cipher.struct(1 if solid else n) if cipher is not None else None
        ks, _keep_k = _kinds_struct(n, kinds, links)
        ms, _keep_m = _meta_struct(n, extra, facets)
        vp = ctypes.c_void_p
        ref = lambda x: ctypes.byref(x) if x is not None else None
        if solid:
            f = self._L.pna_gpu_create_solid_archive_tree_device
            f.argtypes = [vp, ctypes.c_int, ctypes.c_int, ctypes.c_size_t, vp, vp, vp, vp, vp, vp, ctypes.c_uint32, vp, vp, ctypes.c_size_t, vp, vp]
            self._check(f(self._h, algo, level, n, a_names, vp(d_src), a_off, a_len, ref(cs), ref(ms), max_chunk_size, ref(ks), vp(d_dst), dst_cap, ctypes.byref(total), None))
            return total.value, None
        f = self._L.pna_gpu_create_archive_tree_device
        f.argtypes = [vp, ctypes.c_int, ctypes.c_int, ctypes.c_size_t, vp, vp, vp, vp, vp, vp, ctypes.c_uint32, vp, vp, ctypes.c_size_t, vp, vp, ctypes.c_uint32, vp]
        self._check(f(self._h, algo, level, n, a_names, vp(d_src), a_off, a_len, ref(cs), ref(ms), max_chunk_size, ref(ks), vp(d_dst), dst_cap, a_out,
                      ctypes.byref(total), part, None))
        return total.value, list(a_out)

    def set_option(self, name: str, value: int) -> None:
        """pna_gpu_set_option: tuning knobs of the context (include/pna_gpu.h lists them)."""
        self._L.pna_gpu_set_option.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_long]
        self._check(self._L.pna_gpu_set_option(self._h, name.encode(), value))

    def options(self, **kw):
        """Context manager: set options for the duration of a block, then put the given previous values back (tests: `with ctx.options(sub_mib=(128, 1024))`
        -- value, value to restore)."""
        ctx = self

        class _O:
            def __enter__(self_):
                for k, (v, _) in kw.items():
                    ctx.set_option(k, v)

            def __exit__(self_, *a):
                for k, (_, r) in kw.items():
                    ctx.set_option(k, r)
        return _O()

    def timing(self) -> Timing:
        t = Timing()
        self._check(self._L.pna_gpu_last_timing(self._h, ctypes.byref(t)))
        return t

    def decode_forms(self) -> DecodeForms:
        f = DecodeForms()
        self._check(self._L.pna_gpu_last_decode_forms(self._h, ctypes.byref(f)))
        return f

    def debug_block(self, block: int):
        """LZ-stage output of one block of the last device batch: (list of (ll, ml, off), literal bytes)."""
        seqs = (ctypes.c_uint64 * SEQ_CAP)()
        lits = ctypes.create_string_buffer(BLK_SIZE)
        ns, nl = ctypes.c_uint32(), ctypes.c_uint32()
        self._check(self._L.pna_gpu_debug_block(self._h, block, seqs, SEQ_CAP, ctypes.byref(ns), lits, BLK_SIZE, ctypes.byref(nl)))
        out = [((s >> 38) & 0x3FFFF, (s >> 20) & 0x3FFFF, s & 0xFFFFF) for s in seqs[:ns.value]]
        return out, lits.raw[:nl.value]

    def lz_stamps(self):
        a = (ctypes.c_ulonglong * 8)()
        self._check(self._L.pna_gpu_debug_lz_stamps(self._h, a))
        return list(a)

    def corpus_fill_device(self, kind: int, first_file: int, n_files: int, file_len: int, stride: int, d_dst: int) -> None:
        self._check(self._L.pna_bench_corpus_fill_device(self._h, kind, first_file, n_files, file_len, stride,
                                                         ctypes.c_void_p(d_dst), None))

    # ---- streaming facade
    def writer(self, sink, algo: int = ALGO_ZSTD, level: int = LEVEL_DEFAULT) -> "CompressionWriter":
        """One writer per entry; writers of one context may be driven from many threads at once (their finishes are batched)."""
        return CompressionWriter(self, sink, algo, level)

    def stream_stats(self):
        """(device batches, entries, largest batch) run so far on behalf of CompressionWriter.try_into_inner()."""
        b, e, m = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
        self._check(self._L.pna_gpu_stream_stats(self._h, ctypes.byref(b), ctypes.byref(e), ctypes.byref(m)))
        return b.value, e.value, m.value

    def bench_stream_threads(self, entries: Sequence[bytes], threads: int, algo: int = ALGO_ZSTD, level: int = LEVEL_DEFAULT):
        """The reference's one-entry-per-task fan-out on `threads` native host threads over the streaming facade; (seconds, compressed bytes)."""
        n = len(entries)
        keep = [ctypes.create_string_buffer(e, len(e)) for e in entries]
        src = (ctypes.c_void_p * max(n, 1))(*[ctypes.cast(k, ctypes.c_void_p) for k in keep])
        sl = (ctypes.c_size_t * max(n, 1))(*[len(e) for e in entries])
        out, rc = ctypes.c_uint64(), ctypes.c_int()
        secs = self._L.pna_bench_stream_threads(self._h, algo, level, threads, n, src, sl, ctypes.byref(out), ctypes.byref(rc))
        self._check(rc.value)
        return secs, out.value

    def compress_solid(self, data: bytes, algo: int = ALGO_ZSTD, level: int = LEVEL_DEFAULT) -> List[bytes]:
        """SolidArchive payload: returns the pieces pushed to the sink (one SDAT chunk each in the reference)."""
        pieces: List[bytes] = []

        def _sink(_u, buf, n):
            pieces.append(ctypes.string_at(buf, n))
            return 0
        cb = SINK_FN(_sink)
        self._check(self._L.pna_gpu_compress_solid(self._h, algo, level, bytes(data), len(data), cb, None))
        return pieces


class CompressionWriter:
    """Shape of CompressionWriter<W> -- lib/src/compress.rs:21-76: write(), flush(), try_into_inner() (= finish)."""

    def __init__(self, ctx: Context, sink, algo: int, level: int):
        self._ctx, self._sink_obj = ctx, sink

        def _sink(_u, buf, n):
            try:
                sink.write(ctypes.string_at(buf, n))
                return 0
            except Exception:
                return 1
        self._cb = SINK_FN(_sink)
        h = ctypes.c_void_p()
        ctx._check(ctx._L.pna_gpu_stream_new(ctx._h, algo, level, self._cb, None, ctypes.byref(h)))
        self._h = h

    def write(self, data: bytes) -> int:
        self._ctx._check(self._ctx._L.pna_gpu_stream_write(self._h, bytes(data), len(data)))
        return len(data)

    def flush(self) -> None:
        self._ctx._check(self._ctx._L.pna_gpu_stream_flush(self._h))

    def try_into_inner(self):
        h, self._h = self._h, None
        self._ctx._check(self._ctx._L.pna_gpu_stream_finish(h))
        return self._sink_obj


class Archive:
    """Archive<W> writer -- lib/src/archive/write.rs: write_header (constructor), add_entry, finalize.

    The sink is any object with .write(bytes).  Payloads handed to add_file() are already-compressed streams."""

    def __init__(self, sink, archive_number: int = 0):
        self._L = load_library()
        self._sink_obj = sink

        def _sink(_u, buf, n):
            try:
                sink.write(ctypes.string_at(buf, n))
                return 0
            except Exception:
                return 1
        self._cb = SINK_FN(_sink)
        h = ctypes.c_void_p()
        rc = self._L.pna_archive_new(self._cb, None, archive_number, ctypes.byref(h))
        if rc:
            raise PnaGpuError(rc, self._L.pna_gpu_strerror(rc).decode())
        self._h = h

    def _check(self, rc):
        if rc:
            raise PnaGpuError(rc, self._L.pna_gpu_strerror(rc).decode())

    def add_file(self, name: str, compression: int, raw_size: Optional[int], payload: bytes, max_chunk_size: int = 0):
        self._check(self._L.pna_archive_add_file(self._h, name.encode(), compression, -1 if raw_size is None else raw_size,
                                                 bytes(payload), len(payload), max_chunk_size))

    def add_dir(self, name: str):
        self._check(self._L.pna_archive_add_dir(self._h, name.encode()))

    def add_solid(self, compression: int, pieces: Sequence[bytes]):
        n = len(pieces)
        bufs = [ctypes.create_string_buffer(bytes(p), max(len(p), 1)) for p in pieces]
        pp = (ctypes.c_void_p * max(n, 1))(*[ctypes.cast(b, ctypes.c_void_p) for b in bufs])
        pl = (ctypes.c_size_t * max(n, 1))(*[len(p) for p in pieces])
        self._check(self._L.pna_archive_add_solid(self._h, compression, pp, pl, n))

    def finalize(self):
        h, self._h = self._h, None
        self._check(self._L.pna_archive_finalize(h))
        return self._sink_obj


def inner_entry_bytes(name: str, data: bytes) -> bytes:
    """One STORE entry serialised as chunk bytes (what SolidArchive::add_entry feeds the compressor)."""
    L = load_library()
    need = L.pna_archive_inner_entry_bytes(name.encode(), bytes(data), len(data), None, 0)
    buf = ctypes.create_string_buffer(need)
    got = L.pna_archive_inner_entry_bytes(name.encode(), bytes(data), len(data), buf, need)
    return buf.raw[:got]


def archive_bound(algo: int, names: Sequence[str], src_len: Sequence[int]) -> int:
    n = len(src_len)
    a_names = (ctypes.c_char_p * max(n, 1))(*[s.encode() for s in names])
    a_len = (ctypes.c_uint64 * max(n, 1))(*src_len)
    return load_library().pna_gpu_archive_bound(algo, n, a_names, a_len)


def archive_enc_bound(algo: int, names: Sequence[str], src_len: Sequence[int], cipher: Optional[Cipher]) -> int:
    n = len(src_len)
    a_names = (ctypes.c_char_p * max(n, 1))(*[s.encode() for s in names])
    a_len = (ctypes.c_uint64 * max(n, 1))(*src_len)
    cs = cipher.struct(0) if cipher is not None and cipher.ivs is None else (cipher.struct(n) if cipher is not None else None)
    return load_library().pna_gpu_archive_enc_bound(algo, n, a_names, a_len, ctypes.byref(cs) if cs is not None else None)


def archive_chunked_bound(algo: int, names: Sequence[str], src_len: Sequence[int], max_chunk_size: int, cipher: Optional[Cipher] = None) -> int:
    n = len(src_len)
    a_names = (ctypes.c_char_p * max(n, 1))(*[s.encode() for s in names])
    a_len = (ctypes.c_uint64 * max(n, 1))(*src_len)
    cs = cipher.struct(0) if cipher is not None and cipher.ivs is None else (cipher.struct(n) if cipher is not None else None)
    L = load_library()
    L.pna_gpu_archive_chunked_bound.restype = ctypes.c_size_t
    L.pna_gpu_archive_chunked_bound.argtypes = [ctypes.c_int, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32]
    return L.pna_gpu_archive_chunked_bound(algo, n, a_names, a_len, ctypes.byref(cs) if cs is not None else None, max_chunk_size)


def create_archive_chunked(ctx: "Context", names: Sequence[str], entries: Sequence[bytes], max_chunk_size: int, algo: int = ALGO_ZSTD,
                           level: int = LEVEL_DEFAULT, cipher: Optional[Cipher] = None, part: int = PART_HEAD | PART_TAIL) -> bytes:
    """pna_gpu_create_archive_chunked_host: the bounded host pipeline with FlattenWriter::max_chunk_size (lib/src/util/io.rs:60-77)."""
    L = load_library()
    n = len(entries)
    out = bytearray()

    def _sink(_u, buf, k):
        out.extend((ctypes.c_char * k).from_address(buf))
        return 0
    cb = SINK_FN(_sink)
    bufs = [e if isinstance(e, bytes) else bytes(e) for e in entries]
    a_names = (ctypes.c_char_p * max(n, 1))(*[s.encode() for s in names])
    a_src = (ctypes.c_void_p * max(n, 1))(*[ctypes.cast(ctypes.c_char_p(b), ctypes.c_void_p) for b in bufs])
    a_len = (ctypes.c_size_t * max(n, 1))(*[len(e) for e in entries])
    cs = cipher.struct(n) if cipher is not None else None
    L.pna_gpu_create_archive_chunked_host.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                                      ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, SINK_FN, ctypes.c_void_p]
    rc = L.pna_gpu_create_archive_chunked_host(ctx._h, algo, level, n, a_names, a_src, a_len, ctypes.byref(cs) if cs is not None else None, None,
                                               max_chunk_size, part, cb, None)
    if rc:
        raise PnaGpuError(rc, L.pna_gpu_last_error(ctx._h).decode() or L.pna_gpu_strerror(rc).decode())
    return bytes(out)


def gather_verdict(sizes: Sequence[int], caps: Sequence[int], root: int = 0):
    """pna_gather_verdict: what every rank decides from the all-gathered (size, capacity) pairs -- (rc, offsets); rc = PNA_E_DSTSIZE when the parts
    do not fit the root's capacity (the same answer on every rank, so an overflow is an error everywhere and never a hang)."""
    n = len(sizes)
    pairs = (ctypes.c_uint64 * (2 * n))(*[v for sc in zip(sizes, caps) for v in sc])
    o = (ctypes.c_uint64 * (n + 1))()
    L = load_library()
    L.pna_gather_verdict.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    rc = L.pna_gather_verdict(pairs, n, root, None, o)
    return rc, list(o)


def gather_offsets(sizes: Sequence[int]) -> List[int]:
    """pna_gather_offsets: where every rank's part starts in the gathered stream (+ the total)."""
    n = len(sizes)
    a = (ctypes.c_uint64 * max(n, 1))(*sizes)
    o = (ctypes.c_uint64 * (n + 1))()
    rc = load_library().pna_gather_offsets(a, n, o)
    if rc:
        raise PnaGpuError(rc, "pna_gather_offsets")
    return list(o)


class Comm:
    """pna_gpu_comm: the RCCL communicator of the ordered gather (one process per GPU).  `Comm.unique_id()` on rank 0, the 128 bytes to all ranks."""

    @staticmethod
    def unique_id() -> bytes:
        buf = ctypes.create_string_buffer(128)
        rc = load_library().pna_gpu_comm_unique_id(buf)
        if rc:
            raise PnaGpuError(rc, "pna_gpu_comm_unique_id (is RCCL installed?)")
        return buf.raw

    def __init__(self, device: int, uid: bytes, nranks: int, rank: int):
        self._L = load_library()
        self._L.pna_gpu_comm_last_error.restype = ctypes.c_char_p
        self._L.pna_gpu_comm_last_error.argtypes = [ctypes.c_void_p]
        h = ctypes.c_void_p()
        rc = self._L.pna_gpu_comm_init(device, bytes(uid), nranks, rank, ctypes.byref(h))
        if rc:
            raise PnaGpuError(rc, "pna_gpu_comm_init")
        self._h, self.nranks, self.rank = h, nranks, rank

    def gather_ordered(self, d_local: int, local_len: int, d_out: int = 0, out_cap: int = 0, root: int = 0, stream: int = 0):
        """Returns (sizes of all ranks' parts, total); on `root` the parts lie in d_out in rank order."""
        sizes = (ctypes.c_uint64 * self.nranks)()
        total = ctypes.c_uint64()
        f = self._L.pna_gpu_gather_ordered
        f.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
        rc = f(self._h, ctypes.c_void_p(d_local), local_len, root, ctypes.c_void_p(d_out), out_cap, sizes, ctypes.byref(total), ctypes.c_void_p(stream) if stream else None)
        if rc:
            raise PnaGpuError(rc, self._L.pna_gpu_comm_last_error(self._h).decode())
        return list(sizes), total.value

    def gather_ordered_start(self, d_local: int, local_len: int, d_out: int = 0, out_cap: int = 0, root: int = 0, stream: int = 0):
        """Posts the gather behind the work queued on `stream` and returns (sizes, total) as soon as the size exchange is through; the transfers run on the
        communicator's own stream until gather_wait().  PnaGpuError(PNA_E_DSTSIZE) is raised on EVERY rank when the parts do not fit the root's d_out."""
        sizes = (ctypes.c_uint64 * self.nranks)()
        total = ctypes.c_uint64()
        f = self._L.pna_gpu_gather_ordered_start
        f.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
        rc = f(self._h, ctypes.c_void_p(d_local), local_len, root, ctypes.c_void_p(d_out), out_cap, sizes, ctypes.byref(total), ctypes.c_void_p(stream) if stream else None)
        if rc:
            raise PnaGpuError(rc, self._L.pna_gpu_comm_last_error(self._h).decode())
        return list(sizes), total.value

    def ticket(self) -> int:
        """The latest posted gather's ticket (= how many this communicator has posted)."""
        self._L.pna_gpu_gather_ticket.argtypes = [ctypes.c_void_p]
        self._L.pna_gpu_gather_ticket.restype = ctypes.c_uint64
        return int(self._L.pna_gpu_gather_ticket(self._h))

    def gather_wait(self, ticket: int = 0):
        """Blocks until the gathers up to `ticket` are done (0: all posted ones)."""
        self._L.pna_gpu_gather_wait_for.argtypes = [ctypes.c_void_p, ctypes.c_uint64]
        rc = self._L.pna_gpu_gather_wait_for(self._h, ticket)
        if rc:
            raise PnaGpuError(rc, self._L.pna_gpu_comm_last_error(self._h).decode())

    def close(self):
        if getattr(self, "_h", None):
            self._L.pna_gpu_comm_destroy.argtypes = [ctypes.c_void_p]
            self._L.pna_gpu_comm_destroy(self._h)
            self._h = None


def solid_archive_bound(algo: int, names: Sequence[str], src_len: Sequence[int]) -> int:
    n = len(src_len)
    a_names = (ctypes.c_char_p * max(n, 1))(*[s.encode() for s in names])
    a_len = (ctypes.c_uint64 * max(n, 1))(*src_len)
    return load_library().pna_gpu_solid_archive_bound(algo, n, a_names, a_len)


def solid_archive_enc_bound(algo: int, names: Sequence[str], src_len: Sequence[int], cipher: Optional[Cipher]) -> int:
    n = len(src_len)
    a_names = (ctypes.c_char_p * max(n, 1))(*[s.encode() for s in names])
    a_len = (ctypes.c_uint64 * max(n, 1))(*src_len)
    cs = cipher.struct(1) if cipher is not None else None
    return load_library().pna_gpu_solid_archive_enc_bound(algo, n, a_names, a_len, ctypes.byref(cs) if cs is not None else None)


def crc_schedule(payload: bytes) -> int:
    """crc32(b"FDAT" + payload) computed by the host walk through k_frame's lane schedule (table self-check)."""
    return load_library().pna_gpu_debug_crc_schedule(payload, len(payload))


def crc32(data: bytes, crc: int = 0) -> int:
    return load_library().pna_crc32(crc, bytes(data), len(data))


class HostSlot:
    """pna_gpu_host_alloc: a page-locked buffer the host reads its files into (read_exact into the slot instead of fs::read into a Vec,
    cli/src/command/core.rs:889-913); entries that lie in one go to the device straight from there -- no staging copy.  `view` is a writable
    memoryview of the buffer, `ptr` its address."""

    def __init__(self, ctx: "Context", nbytes: int):
        self._ctx, self.nbytes = ctx, nbytes
        p = ctypes.c_void_p()
        L = ctx._L
        L.pna_gpu_host_alloc.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_void_p)]
        ctx._check(L.pna_gpu_host_alloc(ctx._h, nbytes, ctypes.byref(p)))
        self.ptr = p.value
        self.view = memoryview((ctypes.c_ubyte * nbytes).from_address(self.ptr)).cast("B")

    def free(self):
        if self.ptr:
            self.view.release()
            self._ctx._L.pna_gpu_host_free.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
            self._ctx._check(self._ctx._L.pna_gpu_host_free(self._ctx._h, ctypes.c_void_p(self.ptr)))
            self.ptr = 0


def create_archive_from_slot(ctx: "Context", names: Sequence[str], slot: HostSlot, offsets: Sequence[int], lengths: Sequence[int], algo: int = ALGO_ZSTD,
                             level: int = LEVEL_DEFAULT) -> bytes:
    """pna_gpu_create_archive_host over entries that lie in a HostSlot (entry i = slot bytes [offsets[i], offsets[i] + lengths[i])): the zero-staging path."""
    L = load_library()
    n = len(lengths)
    out = bytearray()

    def _sink(_u, buf, k):
        out.extend((ctypes.c_char * k).from_address(buf))
        return 0
    cb = SINK_FN(_sink)
    a_names = (ctypes.c_char_p * max(n, 1))(*[s.encode() for s in names])
    a_src = (ctypes.c_void_p * max(n, 1))(*[slot.ptr + o for o in offsets])
    a_len = (ctypes.c_size_t * max(n, 1))(*lengths)
    ctx._check(L.pna_gpu_create_archive_host(ctx._h, algo, level, n, a_names, a_src, a_len, cb, None))
    return bytes(out)


def create_archive(ctx: Optional[Context], names: Sequence[str], entries: Sequence[bytes], algo: int = ALGO_ZSTD,
                   level: int = LEVEL_DEFAULT, solid: bool = False) -> bytes:
    """`pna create` (cli/src/command/create.rs:575-635): entry-parallel compression on the GPU, ordered write."""
    L = load_library()
    n = len(entries)
    out = bytearray()

    def _sink(_u, buf, k):
        out.extend((ctypes.c_char * k).from_address(buf))      # one copy out of the (page-locked) staging buffer
        return 0
    cb = SINK_FN(_sink)
    bufs = [e if isinstance(e, bytes) else bytes(e) for e in entries]      # kept alive; passed by pointer, not copied
    a_names = (ctypes.c_char_p * max(n, 1))(*[s.encode() for s in names])
    a_src = (ctypes.c_void_p * max(n, 1))(*[ctypes.cast(ctypes.c_char_p(b), ctypes.c_void_p) for b in bufs])
    a_len = (ctypes.c_size_t * max(n, 1))(*[len(e) for e in entries])
    rc = L.pna_create_archive(ctx._h if ctx is not None else None, algo, level, 1 if solid else 0, n, a_names, a_src, a_len, cb, None)
    if rc:
        msg = L.pna_gpu_last_error(ctx._h).decode() if ctx is not None else ""
        raise PnaGpuError(rc, msg or L.pna_gpu_strerror(rc).decode())
    return bytes(out)


def kdf_pbkdf2_sha256(password: bytes, salt: bytes, rounds: int, key_len: int = 32):
    """hash::pbkdf2_with_salt on the C++ host (include/pna_archive.h): returns (key, PHSF string)."""
    key = ctypes.create_string_buffer(key_len)
    phsf = ctypes.create_string_buffer(256)
    rc = load_library().pna_kdf_pbkdf2_sha256(bytes(password), len(password), bytes(salt), len(salt), rounds, key, key_len, phsf, 256)
    if rc:
        raise PnaGpuError(rc, load_library().pna_gpu_strerror(rc).decode())
    return key.raw, phsf.value.decode()


KDFS = {"argon2id": 0, "pbkdf2": 1}      # include/pna_archive.h PNA_KDF_*


def kdf_derive(kdf: str, password: bytes, salt: bytes, rounds: int = 0):
    """The password hash of create_archive_encrypted(kdf=...) over a given salt (pna_kdf_derive): returns (key, PHSF string)."""
    if kdf not in KDFS:
        raise ValueError("kdf must be one of %s" % sorted(KDFS))
    key = ctypes.create_string_buffer(32)
    phsf = ctypes.create_string_buffer(256)
    rc = load_library().pna_kdf_derive(KDFS[kdf], bytes(password), len(password), bytes(salt), len(salt), rounds, key, phsf, 256)
    if rc:
        raise PnaGpuError(rc, load_library().pna_gpu_strerror(rc).decode())
    return key.raw, phsf.value.decode()


def create_archive_encrypted(ctx: Context, names: Sequence[str], entries: Sequence[bytes], password: bytes, algo: int = ALGO_ZSTD,
                             level: int = LEVEL_DEFAULT, mode: int = MODE_CTR, rounds: int = 0, cipher: Optional[Cipher] = None,
                             solid: bool = False, kdf: str = "pbkdf2", encryption: int = ENC_AES) -> bytes:
    """`pna create [--solid] --aes [ctr|cbc|gcm] [--argon2 | --pbkdf2]`: key derivation on the host, compression + cipher + framing on the device.
    encryption: ENC_AES (default) or ENC_CAMELLIA (`--camellia`; on a context with set_option("camellia", 1), PNA_E_UNSUPPORTED otherwise); with
    `cipher` it is the cipher's own that counts.
    kdf: "pbkdf2" (PBKDF2-SHA256, `rounds`, 0 = 600 000) or "argon2id" (m=19456, t=2, p=1, the reference's default).  solid: one cipher stream
    over the solid stream, CTR or GCM (pna_gpu_create_solid_archive_enc_host).  With `cipher` the caller supplies key / PHSF / IVs itself
    (pna_gpu_create_archive_enc_host, or the solid form: one IV / one salt || nonce prefix)."""
    if kdf not in KDFS:
        raise ValueError("kdf must be one of %s" % sorted(KDFS))
    L = load_library()
    n = len(entries)
    out = bytearray()

    def _sink(_u, buf, k):
        out.extend((ctypes.c_char * k).from_address(buf))
        return 0
    cb = SINK_FN(_sink)
    bufs = [e if isinstance(e, bytes) else bytes(e) for e in entries]
    a_names = (ctypes.c_char_p * max(n, 1))(*[s.encode() for s in names])
    a_src = (ctypes.c_void_p * max(n, 1))(*[ctypes.cast(ctypes.c_char_p(b), ctypes.c_void_p) for b in bufs])
    a_len = (ctypes.c_size_t * max(n, 1))(*[len(e) for e in entries])
    if cipher is not None and solid:
        cs = cipher.struct(1)
        rc = L.pna_gpu_create_solid_archive_enc_host(ctx._h, algo, level, n, a_names, a_src, a_len, ctypes.byref(cs), cb, None)
    elif cipher is not None:
        cs = cipher.struct(n)
        rc = L.pna_gpu_create_archive_enc_host(ctx._h, algo, level, n, a_names, a_src, a_len, ctypes.byref(cs), cb, None)
    elif encryption != ENC_AES:
        rc = L.pna_create_archive_encrypted_with(ctx._h, algo, level, 1 if solid else 0, n, a_names, a_src, a_len, bytes(password), len(password),
                                                 encryption, mode, KDFS[kdf], rounds, cb, None)
    elif solid or kdf != "pbkdf2":
        rc = L.pna_create_archive_encrypted_ex(ctx._h, algo, level, 1 if solid else 0, n, a_names, a_src, a_len, bytes(password), len(password),
                                               mode, KDFS[kdf], rounds, cb, None)
    else:
        rc = L.pna_create_archive_encrypted(ctx._h, algo, level, n, a_names, a_src, a_len, bytes(password), len(password), mode, rounds, cb, None)
    if rc:
        raise PnaGpuError(rc, L.pna_gpu_last_error(ctx._h).decode() or L.pna_gpu_strerror(rc).decode())
    return bytes(out)


def extract_archive(ctx: Context, archive: bytes, password: Optional[bytes] = None):
    """`pna extract` for a non-solid archive (pna_gpu_extract_archive_host): returns [(name, kind, data)] in archive order; chunk CRCs
    are verified (data chunks on the device), entries and solid streams are decrypted (AES -- with option "camellia" also Camellia -- in CTR / CBC /
    GCM STREAM) and decoded on the device."""
    out = []

    def _cb(_u, idx, name, kind, data, n):
        out.append((name.decode("utf-8"), kind, ctypes.string_at(data, n) if n else b""))
        return 0
    cb = ENTRY_FN(_cb)
    buf = archive if isinstance(archive, bytes) else bytes(archive)
    rc = ctx._L.pna_gpu_extract_archive_host(ctx._h, buf, len(buf), password, len(password) if password else 0, cb, None)
    ctx._check(rc)
    return out


def verify_archive(ctx: Context, archive_or_parts, password: Optional[bytes] = None, fast: bool = False):
    """`pna experimental verify` (pna_gpu_verify_archive_host): every entry checked on the device, the walk going on after damage.
    `archive_or_parts`: one archive image, or the parts of a split archive in order.  Returns (records, summary): records are
    (name or None, kind, status, flags, size, detail) in archive order (VERIFY_* constants), summary a dict of pna_verify_summary's
    fields plus "rc" -- E_INVAL with summary["broken"] == 1 when the archive's structure broke off (the records before the break are
    kept); any other error raises PnaGpuError."""
    parts = [archive_or_parts] if isinstance(archive_or_parts, (bytes, bytearray, memoryview)) else list(archive_or_parts)
    keep = [p if isinstance(p, bytes) else bytes(p) for p in parts]
    n = len(keep)
    arr = (ctypes.c_char_p * max(n, 1))(*keep)
    lens = (ctypes.c_size_t * max(n, 1))(*[len(p) for p in keep])
    recs = []

    def _cb(_u, idx, name, kind, status, flags, size, detail):
        recs.append((name.decode("utf-8") if name is not None else None, kind, status, flags, size, detail.decode() if detail else ""))
        return 0
    cb = VERIFY_FN(_cb)
    summ = VerifySummary()
    rc = ctx._L.pna_gpu_verify_archive_host(ctx._h, arr, lens, n, password, len(password) if password else 0,
                                            VERIFY_FAST if fast else 0, cb, None, ctypes.byref(summ))
    if rc != PNA_OK and not (rc == E_INVAL and summ.broken):
        ctx._check(rc)
    out = {f: getattr(summ, f) for f, _ in VerifySummary._fields_}
    out["rc"] = rc
    return recs, out


def diff_archive(ctx: Context, archive_or_parts, source, password: Optional[bytes] = None):
    """`pna experimental diff` (pna_gpu_diff_archive_host): the archive's entries against the host's files, compared on the device.
    `source`: a mapping path -> bytes (a path that is absent is a missing file), or a callable (index, path, kind, stored_size) -> (fs_kind, data)
    (DIFF_FS_* constants; data: bytes-like, or None; a (address, length) pair names memory the caller keeps alive until the entry's record, e.g. inside a
    Context.host_alloc buffer, which is copied without staging).  Returns (records, summary): records are DiffRecord tuples in archive order (DIFF_*
    statuses; first_diff is None where the record has none), summary a dict of pna_diff_summary's fields plus "rc" as in verify_archive."""
    parts = [archive_or_parts] if isinstance(archive_or_parts, (bytes, bytearray, memoryview)) else list(archive_or_parts)
    keep = [p if isinstance(p, bytes) else bytes(p) for p in parts]
    n = len(keep)
    arr = (ctypes.c_char_p * max(n, 1))(*keep)
    lens = (ctypes.c_size_t * max(n, 1))(*[len(p) for p in keep])
    recs, held, err = [], {}, []

    def _src(_u, idx, name, kind, stored, out):
        try:
            path = name.decode("utf-8")
            if callable(source):
                fs_kind, data = source(idx, path, kind, None if stored == DIFF_NO_OFFSET else stored)
            else:
                data = source.get(path)
                fs_kind = DIFF_FS_MISSING if data is None else DIFF_FS_FILE
            out[0].fs_kind, out[0].data, out[0].len = fs_kind, None, 0
            if data is not None and fs_kind in (DIFF_FS_FILE, DIFF_FS_SYMLINK):
                if isinstance(data, tuple):
                    out[0].data, out[0].len = data
                elif len(data):
                    if not isinstance(data, bytes):
                        try:
                            data = (ctypes.c_char * len(data)).from_buffer(data)        # (a writable buffer: bytearray, numpy array, mmap -- no copy)
                        except TypeError:
                            data = bytes(data)
                    held[idx] = data                            # alive until the entry's record
                    out[0].data = ctypes.cast(ctypes.c_char_p(data), ctypes.c_void_p).value if isinstance(data, bytes) else ctypes.addressof(data)
                    out[0].len = len(data)
            return 0
        except Exception as e:  # noqa: BLE001 - reported through the call's return code
            err.append(e)
            return 1

    def _cb(_u, idx, name, kind, status, vstatus, flags, size, first, link):
        held.pop(idx, None)
        recs.append(DiffRecord(name.decode("utf-8") if name is not None else None, kind, status, vstatus, flags, size,
                               None if first == DIFF_NO_OFFSET else first, link))
        return 0
    src_cb, cb = DIFF_SOURCE_FN(_src), DIFF_FN(_cb)
    summ = DiffSummary()
    rc = ctx._L.pna_gpu_diff_archive_host(ctx._h, arr, lens, n, password, len(password) if password else 0, src_cb, cb, None, ctypes.byref(summ))
    if err:
        raise err[0]
    if rc != PNA_OK and not (rc == E_INVAL and summ.broken):
        ctx._check(rc)
    out = {f: getattr(summ, f) for f, _ in DiffSummary._fields_ if f != "pad"}
    out["rc"] = rc
    return recs, out


def diff_stats(ctx: Context):
    """(streams handed to the decoders, bytes compared by k_diff, k_diff's HIP-event milliseconds) of the context's latest diff_archive call."""
    a, b, ms = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_double()
    ctx._check(ctx._L.pna_gpu_debug_diff_stats(ctx._h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(ms)))
    return a.value, b.value, ms.value


def extract_plan_runs(rec_off: Sequence[int], rec_len: Sequence[int], wanted: Sequence[int], gap_max: int = EXTRACT_GAP_MAX):
    """pna_extract_plan_runs: the H2D copies [(offset, length)] that carry the wanted records (host code, no device)."""
    n = len(rec_off)
    ro, rl = (ctypes.c_uint64 * max(n, 1))(*rec_off), (ctypes.c_uint64 * max(n, 1))(*rec_len)
    w = (ctypes.c_uint8 * max(n, 1))(*[1 if x else 0 for x in wanted])
    uo, ul, k = (ctypes.c_uint64 * max(n, 1))(), (ctypes.c_uint64 * max(n, 1))(), ctypes.c_size_t()
    rc = load_library().pna_extract_plan_runs(ro, rl, w, n, gap_max, uo, ul, ctypes.byref(k))
    if rc:
        raise PnaGpuError(rc, load_library().pna_gpu_strerror(rc).decode())
    return [(uo[i], ul[i]) for i in range(k.value)]


def extract_select(ctx: Context, archive_or_parts, select, password: Optional[bytes] = None, check_all: bool = False):
    """`pna extract archive.pna path...` (pna_gpu_extract_select_host): the entries `select` chooses, to host memory or to device memory of the caller's.
    `archive_or_parts`: one archive image, or the parts of a split archive in order.  select(index, name, kind, stored_size) -- stored_size None for an
    entry without fSIZ -- returns None (skip), "host", or a contiguous torch.uint8 CUDA tensor (device; cap = numel).  Returns (records, summary): a
    record is (index, name, kind, status, data, length) for a selected entry, in archive order; data is bytes for host records, the caller's tensor
    for device records (None when status is EXTRACT_TOO_SMALL: length then is the size needed); summary a dict of pna_extract_summary's fields."""
    parts = [archive_or_parts] if isinstance(archive_or_parts, (bytes, bytearray, memoryview)) else list(archive_or_parts)
    keep = [p if isinstance(p, bytes) else bytes(p) for p in parts]
    n = len(keep)
    arr = (ctypes.c_char_p * max(n, 1))(*keep)
    lens = (ctypes.c_size_t * max(n, 1))(*[len(p) for p in keep])
    recs, held, err = [], {}, []

    def _sel(_u, idx, name, kind, stored, out):
        try:
            d = select(idx, name.decode("utf-8"), kind, None if stored == EXTRACT_NO_SIZE else stored)
            if d is None:
                out[0].where = EXTRACT_SKIP
            elif isinstance(d, str):
                if d != "host":
                    raise ValueError("select returns None, \"host\" or a torch.uint8 CUDA tensor")
                out[0].where = EXTRACT_HOST
            else:
                import torch
                if not (isinstance(d, torch.Tensor) and d.is_cuda and d.dtype == torch.uint8 and d.is_contiguous()):
                    raise ValueError("select returns None, \"host\" or a contiguous torch.uint8 CUDA tensor")
                held[idx] = d
                out[0].where, out[0].d_dst, out[0].cap = EXTRACT_DEVICE, (d.data_ptr() if d.numel() else None), d.numel()
            return 0
        except Exception as e:  # noqa: BLE001 - reported through the call's return code
            err.append(e)
            return 1

    def _cb(_u, idx, name, kind, status, data, length):
        t = held.pop(idx, None)
        if t is not None:
            recs.append((idx, name.decode("utf-8"), kind, status, None if status == EXTRACT_TOO_SMALL else t, length))
        else:
            recs.append((idx, name.decode("utf-8"), kind, status, ctypes.string_at(data, length) if length else b"", length))
        return 0
    sel_cb, cb = EXTRACT_SELECT_FN(_sel), EXTRACT_RECORD_FN(_cb)
    summ = ExtractSummary()
    try:
        import torch
        if torch.cuda.is_available():
            torch.cuda.synchronize()                            # (the destinations' earlier work on torch's streams is done before the library's stream writes them)
    except ImportError:  # pragma: no cover - torch is optional unless tensors are handed in
        pass
    rc = ctx._L.pna_gpu_extract_select_host(ctx._h, arr, lens, n, password, len(password) if password else 0, EXTRACT_CHECK_ALL if check_all else 0,
                                            sel_cb, cb, None, ctypes.byref(summ))
    if rc != PNA_OK:                                            # (a `select` that raised: E_SINK, its exception as the cause)
        raise PnaGpuError(rc, ctx._L.pna_gpu_last_error(ctx._h).decode() or ctx._L.pna_gpu_strerror(rc).decode()) from (err[0] if err else None)
    return recs, {f: getattr(summ, f) for f, _ in ExtractSummary._fields_}


def extract_to_device(ctx: Context, archive_or_parts, names=None, password: Optional[bytes] = None):
    """The named file entries (all of them when `names` is None) decoded into device memory: {name: torch.uint8 tensor}.  A first call selects nothing
    and collects the fSIZ values; one tensor is allocated from them, entries at 256-byte strides, and extract_select fills it.  Entries without
    fSIZ are offered an empty destination there and report their size (EXTRACT_TOO_SMALL): they, and any entry whose fSIZ was too small, go through a
    second call with the sizes reported."""
    import torch
    want = None if names is None else set(names)
    sizes = {}                                                  # index -> bytes offered

    def _list(idx, name, kind, stored):
        if kind == 0 and (want is None or name in want):
            sizes[idx] = stored or 0
        return None
    extract_select(ctx, archive_or_parts, _list, password)
    out = {}
    for _ in range(2):
        offs, at = {}, 0
        for idx, n in sizes.items():
            offs[idx] = at
            at += (n + 255) & ~255
        buf = torch.empty(max(at, 1), dtype=torch.uint8, device="cuda")
        recs, _s = extract_select(ctx, archive_or_parts,
                                  lambda idx, name, kind, stored: buf[offs[idx]:offs[idx] + sizes[idx]] if idx in offs else None, password)
        sizes = {}
        for idx, name, kind, status, data, length in recs:
            if status == EXTRACT_TOO_SMALL:
                sizes[idx] = length
            else:
                out[name] = data
        if not sizes:
            return out
    raise PnaGpuError(E_INVAL, "extract_to_device: an entry decoded to another size than the call before reported")


def extract_stats(ctx: Context):
    """(bytes of H2D archive copies, streams taken through the decode stage, key derivations, bytes k_pick moved, k_pick's HIP-event milliseconds) of the
    context's latest extract_select call."""
    a, b, k, p, ms = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_double()
    ctx._check(ctx._L.pna_gpu_debug_extract_stats(ctx._h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(k), ctypes.byref(p), ctypes.byref(ms)))
    return a.value, b.value, k.value, p.value, ms.value


def pick_device(ctx: Context, src, src_off: Sequence[int], dsts: Sequence[int], lens: Sequence[int], stream: int = 0) -> None:
    """k_pick alone (pna_gpu_debug_pick_device): bytes [src_off[i], src_off[i] + lens[i]) of the CUDA tensor `src` to device address dsts[i]."""
    n = len(src_off)
    so, ln = (ctypes.c_uint64 * max(n, 1))(*src_off), (ctypes.c_uint64 * max(n, 1))(*lens)
    dd = (ctypes.c_void_p * max(n, 1))(*dsts)
    ctx._check(ctx._L.pna_gpu_debug_pick_device(ctx._h, n, src.data_ptr(), so, dd, ln, stream or None))


def kdf_batch(ctx: Context, password: bytes, jobs, stream: int = 0, with_status: bool = True):
    """pna_gpu_kdf_batch: one password, many salts and parameter sets -> (keys, statuses).  A job is a dict -- {"kind": KDF_ARGON2D / KDF_ARGON2I /
    KDF_ARGON2ID_JOB, "t_cost", "m_cost_kib", "lanes", "salt"} or {"kind": KDF_PBKDF2_SHA256_JOB, "rounds", "salt"} -- or a tuple (kind, t_cost,
    m_cost_kib, lanes, rounds, salt).  Argon2's fill and PBKDF2's chain run on the device for every job the device takes (kdf_stats tells).
    with_status = False passes status = NULL: the first job whose parameters are refused fails the call."""
    n = len(jobs)
    arr, salts = (KdfJob * max(n, 1))(), []
    for i, j in enumerate(jobs):
        if isinstance(j, dict):
            j = (j["kind"], j.get("t_cost", 0), j.get("m_cost_kib", 0), j.get("lanes", 0), j.get("rounds", 0), j["salt"])
        kind, t, m, p, rounds, salt = j
        buf = ctypes.create_string_buffer(bytes(salt), max(len(salt), 1))
        salts.append(buf)
        arr[i] = KdfJob(kind, t, m, p, rounds, ctypes.cast(buf, ctypes.c_void_p), len(salt))
    keys = ctypes.create_string_buffer(32 * max(n, 1))
    st = (ctypes.c_int * max(n, 1))()
    ctx._check(ctx._L.pna_gpu_kdf_batch(ctx._h, bytes(password), len(password), n, arr, keys, st if with_status else None, stream or None))
    return [keys.raw[32 * i:32 * i + 32] for i in range(n)], list(st)[:n]


def phsf_parse(phsf) -> dict:
    """pna_phsf_parse: a PHSF string as a kdf_batch job (a dict).  PnaGpuError: E_INVAL (malformed) or E_UNSUPPORTED (another hash, a cost beyond the caps)."""
    raw = phsf.encode() if isinstance(phsf, str) else bytes(phsf)
    j, salt, n = KdfJob(), ctypes.create_string_buffer(max(len(raw), 1)), ctypes.c_size_t()
    rc = load_library().pna_phsf_parse(raw, len(raw), ctypes.byref(j), salt, len(raw), ctypes.byref(n))
    if rc:
        raise PnaGpuError(rc, load_library().pna_gpu_strerror(rc).decode())
    return {"kind": j.kind, "t_cost": j.t_cost, "m_cost_kib": j.m_cost_kib, "lanes": j.lanes, "rounds": j.rounds, "salt": salt.raw[:n.value]}


def kdf_stats(ctx: Context):
    """(jobs the kernels derived, jobs the host functions derived, rounds of the Argon2 block memory, the kernels' HIP-event milliseconds) of the context's
    latest kdf_batch -- or, after a read-side driver's call under option kdf_device, the sums over that call's batches."""
    d, h, r, ms = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_double()
    ctx._check(ctx._L.pna_gpu_debug_kdf_stats(ctx._h, ctypes.byref(d), ctypes.byref(h), ctypes.byref(r), ctypes.byref(ms)))
    return d.value, h.value, r.value, ms.value


def store_stats(ctx: Context):
    """(pieces through the fused k_store, pieces through its copy-only form, data chunks folded by k_store_fold, k_store's HIP-event milliseconds) of the
    context's latest create call with ALGO_STORE, solid or not (pna_gpu_debug_store_stats), summed over the call's sub-batches: stored payloads without a
    cipher take the fused form, those under a cipher the copy-only one (their CRC is k_frame's, over the ciphertext); the inner payloads of a stored solid
    stream always take the fused form (the cipher runs over the stream afterwards)."""
    f, c, n, ms = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_double()
    ctx._check(ctx._L.pna_gpu_debug_store_stats(ctx._h, ctypes.byref(f), ctypes.byref(c), ctypes.byref(n), ctypes.byref(ms)))
    return f.value, c.value, n.value, ms.value


def kdf_argon2(kind: int, password: bytes, salt: bytes, t_cost: int, m_cost_kib: int, lanes: int, key_len: int = 32) -> bytes:
    """hash::argon2_with_salt on the C++ host (include/pna_archive.h); kind 0 = Argon2d, 1 = Argon2i, 2 = Argon2id."""
    key = ctypes.create_string_buffer(key_len)
    rc = load_library().pna_kdf_argon2(kind, bytes(password), len(password), bytes(salt), len(salt), t_cost, m_cost_kib, lanes, key, key_len)
    if rc:
        raise PnaGpuError(rc, load_library().pna_gpu_strerror(rc).decode())
    return key.raw


def split_archive(archive: bytes, max_part_bytes: int) -> List[bytes]:
    """`pna create --split` (pna_split_archive): one archive image -> the bytes of every part."""
    parts: List[bytearray] = []

    def _sink(_u, idx, buf, n):
        while len(parts) <= idx:
            parts.append(bytearray())
        parts[idx] += ctypes.string_at(buf, n)
        return 0
    cb = PART_SINK_FN(_sink)
    cnt = ctypes.c_uint32()
    rc = load_library().pna_split_archive(bytes(archive), len(archive), max_part_bytes, cb, None, ctypes.byref(cnt))
    if rc:
        raise PnaGpuError(rc, load_library().pna_gpu_strerror(rc).decode())
    assert cnt.value == len(parts)
    return [bytes(p) for p in parts]


def join_parts(parts: Sequence[bytes]) -> bytes:
    """Parts of a multipart archive, in order -> one archive image (pna_join_parts)."""
    out = bytearray()

    def _sink(_u, buf, n):
        out.extend(ctypes.string_at(buf, n))
        return 0
    cb = SINK_FN(_sink)
    n = len(parts)
    keep = [bytes(p) for p in parts]
    a = (ctypes.c_char_p * max(n, 1))(*keep)
    l = (ctypes.c_size_t * max(n, 1))(*[len(p) for p in keep])
    rc = load_library().pna_join_parts(a, l, n, cb, None)
    if rc:
        raise PnaGpuError(rc, load_library().pna_gpu_strerror(rc).decode())
    return bytes(out)


def create_archive_with_metadata(ctx: Context, names: Sequence[str], entries: Sequence[bytes], facets: Optional[Sequence[bytes]] = None,
                                 extra: Optional[Sequence[bytes]] = None, algo: int = ALGO_ZSTD, level: int = LEVEL_DEFAULT,
                                 cipher: Optional[Cipher] = None) -> bytes:
    """`pna create --keep-timestamp --keep-permission ...` (pna_gpu_create_archive_meta_host): facets[i] / extra[i] are chunks the
    caller has already framed (length | type | data | crc); they land around fSIZ exactly where NormalEntry::write_chunks_to puts them."""
    L = load_library()
    n = len(entries)
    out = bytearray()

    def _sink(_u, buf, k):
        out.extend((ctypes.c_char * k).from_address(buf))
        return 0
    cb = SINK_FN(_sink)
    bufs = [e if isinstance(e, bytes) else bytes(e) for e in entries]
    a_names = (ctypes.c_char_p * max(n, 1))(*[s.encode() for s in names])
    a_src = (ctypes.c_void_p * max(n, 1))(*[ctypes.cast(ctypes.c_char_p(b), ctypes.c_void_p) for b in bufs])
    a_len = (ctypes.c_size_t * max(n, 1))(*[len(e) for e in entries])
    ms = MetaStruct()
    keep = []
    for field, blobs in (("extra", extra), ("facets", facets)):
        if blobs is None:
            continue
        bb = [bytes(b) for b in blobs]
        keep.append(bb)
        arr = (ctypes.c_void_p * max(n, 1))(*[ctypes.cast(ctypes.c_char_p(b), ctypes.c_void_p) if b else None for b in bb])
        lens = (ctypes.c_size_t * max(n, 1))(*[len(b) for b in bb])
        keep += [arr, lens]
        setattr(ms, field, ctypes.cast(arr, ctypes.POINTER(ctypes.c_void_p)))
        setattr(ms, field + "_len", ctypes.cast(lens, ctypes.POINTER(ctypes.c_size_t)))
    cs = cipher.struct(n) if cipher is not None else None
    rc = L.pna_gpu_create_archive_meta_host(ctx._h, algo, level, n, a_names, a_src, a_len, ctypes.byref(cs) if cs is not None else None,
                                            ctypes.byref(ms), cb, None)
    if rc:
        raise PnaGpuError(rc, L.pna_gpu_last_error(ctx._h).decode() or L.pna_gpu_strerror(rc).decode())
    return bytes(out)


def write_file(ctx: Context, sink, name: str, writes: Sequence[bytes], algo: int = ALGO_ZSTD, level: int = LEVEL_DEFAULT,
               meta: bytes = b"", max_chunk_size: int = 0) -> None:
    """Archive::write_file (lib/src/archive/write.rs:276-299 -> write_stream_entry, :730-777): an entry whose data arrives in `writes`;
    the record carries no fSIZ and one FDAT chunk per encoder burst.  `sink(bytes)` receives the entry's chunk bytes; `meta` = already
    framed extra + metadata chunks."""
    L = load_library()

    def _sink(_u, buf, n):
        sink(ctypes.string_at(buf, n))
        return 0
    cb = SINK_FN(_sink)
    w = ctypes.c_void_p()
    ctx._check(L.pna_gpu_stream_entry_begin(ctx._h, algo, level, name.encode(), meta, len(meta), max_chunk_size, cb, None, ctypes.byref(w)))
    for d in writes:
        rc = L.pna_gpu_stream_entry_write(w, bytes(d), len(d))
        if rc:
            L.pna_gpu_stream_entry_abort(w)
            ctx._check(rc)
    ctx._check(L.pna_gpu_stream_entry_finish(w))


def seek_to_end(archive: bytes):
    """Archive::seek_to_end (lib/src/archive/read.rs:412-424): (offset of the AEND chunk, has_next_archive)."""
    off, nxt = ctypes.c_uint64(), ctypes.c_int()
    rc = load_library().pna_archive_seek_to_end(bytes(archive), len(archive), ctypes.byref(off), ctypes.byref(nxt))
    if rc:
        raise PnaGpuError(rc, load_library().pna_gpu_strerror(rc).decode())
    return off.value, bool(nxt.value)


def list_entries(archive: bytes):
    """Top-level records of an archive image: [(name bytes, kind (-1 = solid), offset, length)] (pna_archive_list_entries)."""
    out = []

    def _cb(_u, idx, name, name_len, kind, off, ln):
        out.append((ctypes.string_at(name, name_len) if name_len else b"", kind, off, ln))
        return 0
    cb = RAW_ENTRY_FN(_cb)
    rc = load_library().pna_archive_list_entries(bytes(archive), len(archive), cb, None)
    if rc:
        raise PnaGpuError(rc, load_library().pna_gpu_strerror(rc).decode())
    return out


def append_archive(ctx: Context, archive: bytes, names: Sequence[str], entries: Sequence[bytes], algo: int = ALGO_ZSTD,
                   level: int = LEVEL_DEFAULT) -> bytes:
    """`pna append` (cli/src/command/append.rs:504-560): the archive with the new entries behind the old ones."""
    L = load_library()
    n = len(entries)
    out = bytearray()

    def _sink(_u, buf, k):
        out.extend(ctypes.string_at(buf, k))
        return 0
    cb = SINK_FN(_sink)
    keep = [bytes(e) for e in entries]
    a_names = (ctypes.c_char_p * max(n, 1))(*[s.encode() for s in names])
    a_src = (ctypes.c_void_p * max(n, 1))(*[ctypes.cast(ctypes.c_char_p(b), ctypes.c_void_p) for b in keep])
    a_len = (ctypes.c_size_t * max(n, 1))(*[len(b) for b in keep])
    at = ctypes.c_uint64()
    ctx._check(L.pna_gpu_append_archive_host(ctx._h, algo, level, bytes(archive), len(archive), n, a_names, a_src, a_len, ctypes.byref(at), cb, None))
    return bytes(archive[:at.value]) + bytes(out)


def create_archive_multi(ctxs: Sequence[Context], names: Sequence[str], entries: Sequence[bytes], algo: int = ALGO_ZSTD,
                         level: int = LEVEL_DEFAULT) -> bytes:
    """`pna create` from ONE process over several contexts / GPUs (pna_gpu_create_archive_multi_host): contiguous index ranges per
    context, parts written in index order."""
    L = load_library()
    n = len(entries)
    out = bytearray()

    def _sink(_u, buf, k):
        out.extend(ctypes.string_at(buf, k))
        return 0
    cb = SINK_FN(_sink)
    keep = [bytes(e) for e in entries]
    a_ctx = (ctypes.c_void_p * len(ctxs))(*[c._h for c in ctxs])
    a_names = (ctypes.c_char_p * max(n, 1))(*[s.encode() for s in names])
    a_src = (ctypes.c_void_p * max(n, 1))(*[ctypes.cast(ctypes.c_char_p(b), ctypes.c_void_p) for b in keep])
    a_len = (ctypes.c_size_t * max(n, 1))(*[len(b) for b in keep])
    rc = L.pna_gpu_create_archive_multi_host(a_ctx, len(ctxs), algo, level, n, a_names, a_src, a_len, cb, None)
    if rc:
        raise PnaGpuError(rc, L.pna_gpu_last_error(ctxs[0]._h).decode() or L.pna_gpu_strerror(rc).decode())
    return bytes(out)


def entry_record_bytes(kind: int, name: str, target: bytes = b"", extra: bytes = b"", facets: bytes = b"", max_chunk_size: int = 0) -> bytes:
    """pna_archive_entry_record_bytes: the whole record of a directory (KIND_DIRECTORY), symbolic link or hard link as raw chunk bytes --
    FHED | extra | facets | FDAT(target)* | FEND.  Raises ValueError for what the library refuses (a file's kind, a link without a target)."""
    L = load_library()
    f = L.pna_archive_entry_record_bytes
    f.restype = ctypes.c_size_t
    f.argtypes = [ctypes.c_int, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t,
                  ctypes.c_uint32, ctypes.c_void_p, ctypes.c_size_t]
    args = (kind, name.encode(), bytes(extra) or None, len(extra), bytes(facets) or None, len(facets), bytes(target) or None, len(target), max_chunk_size)
    need = f(*args, None, 0)
    if need == 0:
        raise ValueError("not a record this library writes: kind %d, target of %d bytes" % (kind, len(target)))
    buf = ctypes.create_string_buffer(need)
    got = f(*args, buf, need)
    return buf.raw[:got]


def entry_kinds_check(src_len: Sequence[int], kinds, links) -> int:
    """pna_gpu_entry_kinds_check: PNA_OK, or E_INVAL for an unknown kind, a non-file with source bytes, a link without a target.  Needs no device."""
    n = len(src_len)
    ks, _keep = _kinds_struct(n, kinds, links)
    a_len = (ctypes.c_uint64 * max(n, 1))(*src_len)
    f = load_library().pna_gpu_entry_kinds_check
    f.restype = ctypes.c_int
    f.argtypes = [ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p]
    return f(n, a_len, ctypes.byref(ks) if ks is not None else None)


def _tree_bound(fn_name: str, algo: int, names, src_len, kinds, links, cipher, facets, extra, max_chunk_size: int) -> int:
    n = len(src_len)
    a_names = (ctypes.c_char_p * max(n, 1))(*[s.encode() for s in names])
    a_len = (ctypes.c_uint64 * max(n, 1))(*src_len)
    cs = cipher.struct(0) if cipher is not None else None
    ks, _keep_k = _kinds_struct(n, kinds, links)
    ms, _keep_m = _meta_struct(n, extra, facets)
    f = getattr(load_library(), fn_name)
    f.restype = ctypes.c_size_t
    f.argtypes = _TREE_BOUND_ARGS
    ref = lambda x: ctypes.byref(x) if x is not None else None
    return f(algo, n, a_names, a_len, ref(cs), ref(ms), max_chunk_size, ref(ks))


def archive_tree_bound(algo: int, names: Sequence[str], src_len: Sequence[int], kinds=None, links=None, cipher: Optional[Cipher] = None,
                       facets=None, extra=None, max_chunk_size: int = 0) -> int:
    """pna_gpu_archive_tree_bound: the destination capacity of Context.create_archive_tree_device."""
    return _tree_bound("pna_gpu_archive_tree_bound", algo, names, src_len, kinds, links, cipher, facets, extra, max_chunk_size)


def solid_archive_tree_bound(algo: int, names: Sequence[str], src_len: Sequence[int], kinds=None, links=None, cipher: Optional[Cipher] = None,
                             facets=None, extra=None, max_chunk_size: int = 0) -> int:
    """pna_gpu_solid_archive_tree_bound: ... of Context.create_archive_tree_device(solid=True)."""
    return _tree_bound("pna_gpu_solid_archive_tree_bound", algo, names, src_len, kinds, links, cipher, facets, extra, max_chunk_size)


def create_archive_tree(ctx: Context, names: Sequence[str], entries: Sequence[bytes], kinds=None, links=None, algo: int = ALGO_ZSTD,
                        level: int = LEVEL_DEFAULT, cipher: Optional[Cipher] = None, facets=None, extra=None, max_chunk_size: int = 0,
                        solid: bool = False, part: int = PART_HEAD | PART_TAIL) -> bytes:
    """`pna create some/tree` in one call (pna_gpu_create_archive_tree_host; solid: pna_gpu_create_solid_archive_tree_host): create_entry's four arms
    (cli/src/command/core.rs:915-977) as kinds[i] -- KIND_FILE: entries[i] is the file; KIND_DIRECTORY: a record without data; KIND_SYMLINK /
    KIND_HARDLINK: links[i] is the target (stored, never encrypted).  entries[i] of an entry that is not a file must be empty.  facets / extra: framed
    chunks per entry, as in create_archive_with_metadata.  kinds None: create_archive_chunked's bytes."""
    L = load_library()
    n = len(entries)
    out = bytearray()

    def _sink(_u, buf, k):
        out.extend((ctypes.c_char * k).from_address(buf))
        return 0
    cb = SINK_FN(_sink)
    bufs = [e if isinstance(e, bytes) else bytes(e) for e in entries]
    a_names = (ctypes.c_char_p * max(n, 1))(*[s.encode() for s in names])
    a_src = (ctypes.c_void_p * max(n, 1))(*[ctypes.cast(ctypes.c_char_p(b), ctypes.c_void_p) for b in bufs])
    a_len = (ctypes.c_size_t * max(n, 1))(*[len(e) for e in bufs])
    cs = cipher.struct(1 if solid else n) if cipher is not None else None
    ks, _keep_k = _kinds_struct(n, kinds, links)
    ms, _keep_m = _meta_struct(n, extra, facets)
    vp = ctypes.c_void_p
    ref = lambda x: ctypes.byref(x) if x is not None else None
    if solid:
        f = L.pna_gpu_create_solid_archive_tree_host
        f.argtypes = [vp, ctypes.c_int, ctypes.c_int, ctypes.c_size_t, vp, vp, vp, vp, vp, ctypes.c_uint32, vp, SINK_FN, vp]
        rc = f(ctx._h, algo, level, n, a_names, a_src, a_len, ref(cs), ref(ms), max_chunk_size, ref(ks), cb, None)
    else:
        f = L.pna_gpu_create_archive_tree_host
        f.argtypes = [vp, ctypes.c_int, ctypes.c_int, ctypes.c_size_t, vp, vp, vp, vp, vp, ctypes.c_uint32, vp, ctypes.c_uint32, SINK_FN, vp]
        rc = f(ctx._h, algo, level, n, a_names, a_src, a_len, ref(cs), ref(ms), max_chunk_size, ref(ks), part, cb, None)
    if rc:
        raise PnaGpuError(rc, L.pna_gpu_last_error(ctx._h).decode() or L.pna_gpu_strerror(rc).decode())
    return bytes(out)
