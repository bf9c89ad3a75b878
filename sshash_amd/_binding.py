"""ctypes binding of include/sshash_amd.h. Host-side mirror of the reference's dictionary interface."""
from __future__ import annotations

import ctypes as C
import os
import sys
from dataclasses import dataclass
from typing import Callable, Iterable, Optional, Sequence, Union

import numpy as np

INVALID_U64 = 0xFFFFFFFFFFFFFFFF  # reference include/constants.hpp:5
SEGMENTS_OFF = 0xFFFFFFFFFFFFFFFF  # SSHASH_SEGMENTS_OFF: Dictionary.set_read_segments(SEGMENTS_OFF) never cuts a read into segments

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_NAME = "libsshash_amd.so"


def library_path() -> str:
    # SSHASH_AMD_LIBRARY: another build of the same HIP library (tools/debug builds variants of it side by side)
    return os.environ.get("SSHASH_AMD_LIBRARY") or os.path.join(_HERE, _LIB_NAME)


class SSHashError(RuntimeError):
    """Raised for every non-OK sshash_status; ``.status`` holds the code (include/sshash_amd.h)."""

    def __init__(self, status: int, message: str):
        super().__init__(f"[sshash status {status}] {message}")
        self.status = status


class _BuildConfig(C.Structure):
    _fields_ = [
        ("k", C.c_uint32),
        ("m", C.c_uint32),
        ("seed", C.c_uint64),
        ("canonical", C.c_uint32),
        ("num_threads", C.c_uint32),
        ("lambda_", C.c_double),
        ("verbose", C.c_uint32),
        ("weighted", C.c_uint32),
        ("num_shards", C.c_uint32),
        ("shard_id", C.c_uint32),
    ]


class _Info(C.Structure):
    _fields_ = [
        ("version", C.c_uint8 * 3),
        ("canonical", C.c_uint8),
        ("k", C.c_uint32),
        ("m", C.c_uint32),
        ("words_per_kmer", C.c_uint32),
        ("num_kmers", C.c_uint64),
        ("num_strings", C.c_uint64),
        ("num_bases", C.c_uint64),
        ("num_minimizers", C.c_uint64),
        ("num_bits", C.c_uint64),
        ("skew_partitions", C.c_uint32),
        ("weighted", C.c_uint32),
        ("num_shards", C.c_uint32),
        ("shard_id", C.c_uint32),
    ]


class _Results(C.Structure):
    _fields_ = [
        ("kmer_id", C.c_void_p),
        ("kmer_id_in_string", C.c_void_p),
        ("kmer_offset", C.c_void_p),
        ("string_id", C.c_void_p),
        ("string_begin", C.c_void_p),
        ("string_end", C.c_void_p),
        ("kmer_orientation", C.c_void_p),
        ("minimizer_found", C.c_void_p),
    ]


EXCHANGE_COUNTS = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64))
EXCHANGE_DATA = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64), C.c_void_p, C.POINTER(C.c_uint64), C.c_uint32, C.c_void_p)


class _Exchange(C.Structure):  # sshash_exchange
    _fields_ = [("ctx", C.c_void_p), ("counts", EXCHANGE_COUNTS), ("data", EXCHANGE_DATA)]


class _Report(C.Structure):
    _fields_ = [
        ("num_kmers", C.c_uint64),
        ("num_positive_kmers", C.c_uint64),
        ("num_negative_kmers", C.c_uint64),
        ("num_invalid_kmers", C.c_uint64),
        ("num_searches", C.c_uint64),
        ("num_extensions", C.c_uint64),
    ]


# sshash_streaming_run (include/sshash_amd.h): one maximal run of a read -- a search and the extensions behind it
RUN_DTYPE = np.dtype([("kmer_id", "<u8"), ("string_id", "<u8"), ("kmer_id_in_string", "<u8"), ("read_pos", "<u4"), ("num_kmers", "<u4")])
RUN_BACKWARD = 0x80000000  # bit 31 of num_kmers: orientation -1


class _Run(C.Structure):  # (the same record for ctypes: its size and offsets are checked against RUN_DTYPE by the tests)
    _fields_ = [("kmer_id", C.c_uint64), ("string_id", C.c_uint64), ("kmer_id_in_string", C.c_uint64), ("read_pos", C.c_uint32),
                ("num_kmers", C.c_uint32)]


# sshash_string_link (include/sshash_amd.h): one link of the dictionary's graph, from a string's end to a neighbour k-mer
LINK_DTYPE = np.dtype([("from_string", "<u8"), ("to_string", "<u8"), ("to_kmer_id", "<u8"), ("flags", "<u4"), ("reserved", "<u4")])


_lib: Optional[C.CDLL] = None


# sshash_per_read_fn: (ctx, first_read, n, rows) -> 0 to go on
_PerReadFn = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p)
_ReadRunsFn = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p)  # sshash_read_runs_fn: (ctx, first_read, n, run_offsets, runs)
# sshash_read_sum (include/sshash_amd.h): a read's row of streaming_sums
READ_SUM_DTYPE = np.dtype([("sum", "<u8"), ("positive_kmers", "<u8")])
# sshash_read_class: a read's row of streaming_classes, finished by class_best
READ_CLASS_DTYPE = np.dtype([("best_class", "<u4"), ("best", "<u4"), ("second", "<u4"), ("total", "<u4")])
MAX_CLASSES = 4096  # SSHASH_MAX_CLASSES
NO_CLASS = 0xFFFFFFFF  # SSHASH_NO_CLASS: best_class of a row of zeros


# The C ABI as ctypes sees it: name -> (restype, argtypes), one entry per function of include/sshash_amd.h (tests/test_capi.py holds
# the names against the header). _load() binds every one of them.
_P = C.c_void_p
_SIGNATURES = {
    "sshash_last_error": (C.c_char_p, []),
    "sshash_build_info": (C.c_char_p, []),
    "sshash_build_config_default": (None, [C.POINTER(_BuildConfig)]),
    "sshash_build_from_fasta": (C.c_int, [C.c_char_p, C.POINTER(_BuildConfig), C.POINTER(_P)]),
    "sshash_build_from_packed": (C.c_int, [_P, _P, C.c_uint64, C.POINTER(_BuildConfig), C.POINTER(_P)]),
    "sshash_save": (C.c_int, [_P, C.c_char_p]),
    "sshash_load": (C.c_int, [C.c_char_p, C.POINTER(_P)]),
    "sshash_free": (None, [_P]),
    "sshash_get_info": (C.c_int, [_P, C.POINTER(_Info)]),
    "sshash_bucket_stats": (C.c_int, [_P, C.POINTER(C.c_uint64 * 64)]),
    "sshash_device_count": (C.c_int, []),
    "sshash_to_device": (C.c_int, [_P, C.c_int]),
    "sshash_to_device_table_shard": (C.c_int, [_P, C.c_int, C.c_uint32, C.c_uint32]),
    "sshash_device_bytes": (C.c_int, [_P, C.c_int, C.POINTER(C.c_uint64)]),
    "sshash_device_stats": (C.c_int, [_P, C.c_int, C.POINTER(C.c_uint64 * 16)]),
    "sshash_device_table_histogram": (C.c_int, [_P, C.c_int, C.POINTER(C.c_uint64 * 32)]),
    "sshash_device_table_export": (C.c_int, [_P, C.c_int, C.POINTER(C.c_uint64 * 8), C.c_void_p, C.c_uint64]),
    "sshash_sharded_lookup_device": (C.c_int, [_P, C.c_int, C.c_uint32, C.c_int, _P, C.c_uint64, C.c_int, _P, C.POINTER(_Exchange), _P]),
    "sshash_sharded_lookup_rccl": (C.c_int, [_P, C.c_int, _P, C.c_int, _P, C.c_uint64, C.c_int, _P, _P]),
    "sshash_streaming_lookup_device": (C.c_int, [_P, C.c_int, _P, _P, C.c_uint64, C.c_uint64, C.POINTER(_Results), _P, _P]),
    "sshash_streaming_lookup": (C.c_int, [_P, _P, _P, C.c_uint64, C.POINTER(_Results), C.POINTER(_Report)]),
    "sshash_lookup_packed_device": (C.c_int, [_P, C.c_int, _P, C.c_uint64, C.c_int, C.POINTER(_Results), _P]),
    "sshash_lookup_ascii_device": (C.c_int, [_P, C.c_int, _P, C.c_uint64, C.c_int, C.POINTER(_Results), _P]),
    "sshash_lookup_packed": (C.c_int, [_P, _P, C.c_uint64, C.c_int, C.POINTER(_Results)]),
    "sshash_lookup_ascii": (C.c_int, [_P, _P, C.c_uint64, C.c_int, C.POINTER(_Results)]),
    "sshash_neighbours_packed_device": (C.c_int, [_P, C.c_int, _P, C.c_uint64, C.c_int, C.POINTER(_Results), _P]),
    "sshash_neighbours_packed": (C.c_int, [_P, _P, C.c_uint64, C.c_int, C.POINTER(_Results)]),
    "sshash_string_neighbours": (C.c_int, [_P, _P, C.c_uint64, C.c_int, C.POINTER(_Results)]),
    "sshash_string_neighbours_device": (C.c_int, [_P, C.c_int, _P, C.c_uint64, C.c_uint64, C.c_int, C.POINTER(_Results), _P]),
    "sshash_string_links_device": (C.c_int, [_P, C.c_int, C.c_uint64, C.c_uint64, C.c_int, _P, _P, C.c_uint64, _P]),
    "sshash_string_links": (C.c_int, [_P, C.c_uint64, C.c_uint64, C.c_int, _P, _P, C.c_uint64]),
    "sshash_kmer_adjacency_device": (C.c_int, [_P, C.c_int, C.c_uint64, C.c_uint64, C.c_int, _P, _P]),
    "sshash_kmer_adjacency": (C.c_int, [_P, C.c_uint64, C.c_uint64, C.c_int, _P]),
    "sshash_string_size": (C.c_int, [_P, _P, C.c_uint64, _P]),
    "sshash_string_offsets": (C.c_int, [_P, _P, C.c_uint64, _P, _P]),
    "sshash_is_member_packed_device": (C.c_int, [_P, C.c_int, _P, C.c_uint64, C.c_int, _P, _P]),
    "sshash_is_member_packed": (C.c_int, [_P, _P, C.c_uint64, C.c_int, _P]),
    "sshash_is_member_ascii": (C.c_int, [_P, _P, C.c_uint64, C.c_int, _P]),
    "sshash_weight": (C.c_int, [_P, _P, C.c_uint64, _P]),
    "sshash_weight_device": (C.c_int, [_P, C.c_int, _P, C.c_uint64, _P, _P]),
    "sshash_access": (C.c_int, [_P, C.c_uint64, _P]),
    "sshash_access_packed": (C.c_int, [_P, _P, C.c_uint64, _P]),
    "sshash_access_packed_device": (C.c_int, [_P, C.c_int, _P, C.c_uint64, _P, _P]),
    "sshash_streaming_query_from_file": (C.c_int, [_P, C.c_char_p, C.c_int, C.POINTER(_Report)]),
    "sshash_streaming_query": (C.c_int, [_P, _P, _P, C.c_uint64, C.POINTER(_Report)]),
    "sshash_streaming_query_device": (C.c_int, [_P, C.c_int, _P, _P, C.c_uint64, C.c_uint64, _P, _P]),
    "sshash_streaming_query_per_read_device": (C.c_int, [_P, C.c_int, _P, _P, C.c_uint64, C.c_uint64, _P, _P, _P]),
    "sshash_streaming_query_per_read": (C.c_int, [_P, _P, _P, C.c_uint64, _P, C.POINTER(_Report)]),
    "sshash_streaming_query_from_file_per_read": (C.c_int, [_P, C.c_char_p, C.c_int, _PerReadFn, _P, C.POINTER(_Report)]),
    "sshash_streaming_runs_device": (C.c_int, [_P, C.c_int, _P, _P, C.c_uint64, C.c_uint64, _P, _P, C.c_uint64, _P, _P]),
    "sshash_streaming_runs": (C.c_int, [_P, _P, _P, C.c_uint64, _P, _P, C.c_uint64, C.POINTER(_Report)]),
    "sshash_streaming_runs_from_file": (C.c_int, [_P, C.c_char_p, C.c_int, _ReadRunsFn, _P, C.POINTER(_Report)]),
    "sshash_cover_words": (C.c_int, [_P, C.POINTER(C.c_uint64)]),
    "sshash_streaming_cover_device": (C.c_int, [_P, C.c_int, _P, _P, C.c_uint64, C.c_uint64, _P, _P, _P]),
    "sshash_streaming_cover": (C.c_int, [_P, _P, _P, C.c_uint64, _P, C.POINTER(_Report)]),
    "sshash_streaming_cover_from_file": (C.c_int, [_P, C.c_char_p, C.c_int, _P, C.POINTER(_Report)]),
    "sshash_cover_string_counts_device": (C.c_int, [_P, C.c_int, _P, _P, _P, _P]),
    "sshash_cover_string_counts": (C.c_int, [_P, _P, _P, C.POINTER(C.c_uint64)]),
    "sshash_streaming_depth_device": (C.c_int, [_P, C.c_int, _P, _P, C.c_uint64, C.c_uint64, _P, _P, _P]),
    "sshash_depth_finish_device": (C.c_int, [_P, C.c_int, _P, _P, _P]),
    "sshash_set_read_segments": (C.c_int, [_P, C.c_uint64, C.c_int]),
    "sshash_get_read_segments": (C.c_int, [_P, C.POINTER(C.c_uint64), C.POINTER(C.c_int), C.POINTER(C.c_uint64)]),
    "sshash_streaming_depth": (C.c_int, [_P, _P, _P, C.c_uint64, _P, C.POINTER(_Report)]),
    "sshash_streaming_depth_from_file": (C.c_int, [_P, C.c_char_p, C.c_int, _P, C.POINTER(_Report)]),
    "sshash_depth_string_sums_device": (C.c_int, [_P, C.c_int, _P, _P, _P, _P]),
    "sshash_depth_string_sums": (C.c_int, [_P, _P, _P, C.POINTER(C.c_uint64)]),
    "sshash_value_prefix_device": (C.c_int, [_P, C.c_int, _P, C.c_uint32, _P, _P]),
    "sshash_streaming_sums_device": (C.c_int, [_P, C.c_int, _P, _P, C.c_uint64, C.c_uint64, _P, _P, _P, _P]),
    "sshash_streaming_sums": (C.c_int, [_P, _P, _P, C.c_uint64, _P, C.c_uint32, _P, C.POINTER(_Report)]),
    "sshash_streaming_sums_from_file": (C.c_int, [_P, C.c_char_p, C.c_int, _P, C.c_uint32, _PerReadFn, _P, C.POINTER(_Report)]),
    "sshash_streaming_classes_device": (C.c_int, [_P, C.c_int, _P, _P, C.c_uint64, C.c_uint64, _P, C.c_uint32, _P, _P, _P]),
    "sshash_streaming_classes": (C.c_int, [_P, _P, _P, C.c_uint64, _P, C.c_uint32, _P, C.POINTER(_Report)]),
    "sshash_streaming_classes_from_file": (C.c_int, [_P, C.c_char_p, C.c_int, _P, C.c_uint32, _PerReadFn, _P, C.POINTER(_Report)]),
    "sshash_class_best_device": (C.c_int, [_P, C.c_int, _P, C.c_uint64, C.c_uint32, _P, _P]),
    "sshash_class_best": (C.c_int, [_P, C.c_uint64, C.c_uint32, _P]),
    "sshash_class_totals_device": (C.c_int, [_P, C.c_int, _P, C.c_uint64, C.c_uint32, _P, _P]),
    "sshash_class_totals": (C.c_int, [_P, C.c_uint64, C.c_uint32, _P]),
    "sshash_streaming_best_run_device": (C.c_int, [_P, C.c_int, _P, _P, C.c_uint64, C.c_uint64, _P, _P, _P]),
    "sshash_streaming_best_run": (C.c_int, [_P, _P, _P, C.c_uint64, _P, C.POINTER(_Report)]),
    "sshash_streaming_best_run_from_file": (C.c_int, [_P, C.c_char_p, C.c_int, _PerReadFn, _P, C.POINTER(_Report)]),
    "sshash_runs_best_device": (C.c_int, [_P, C.c_int, _P, _P, C.c_uint64, _P, _P]),
    "sshash_runs_best": (C.c_int, [_P, _P, C.c_uint64, _P]),
    "sshash_route_packed_device": (C.c_int, [_P, C.c_int, _P, C.c_uint64, C.c_uint32, _P, _P, _P]),
    "sshash_route_bucket_device": (C.c_int, [_P, C.c_int, _P, C.c_uint64, C.c_uint32, C.c_int, _P, _P, _P, _P]),
    "sshash_route_bucket_by_key_device": (C.c_int, [_P, C.c_int, _P, C.c_uint64, C.c_uint32, _P, _P, _P, _P]),
    "sshash_route_combine_device": (C.c_int, [_P, C.c_int, _P, _P, C.c_uint64, _P, _P]),
    "sshash_iterate_packed": (C.c_int, [_P, C.c_uint64, C.c_uint64, _P]),
    "sshash_iterate_packed_device": (C.c_int, [_P, C.c_int, C.c_uint64, C.c_uint64, _P, _P]),
    "sshash_check_device": (C.c_int, [_P, C.c_int, C.POINTER(C.c_uint64 * 8)]),
}
C_ABI_SYMBOLS = tuple(_SIGNATURES)


def _preload_hip_runtime() -> None:
    """One HIP runtime per process. PyTorch-ROCm wheels bundle their own libamdhip64.so (same SONAME
    as the system one); if libsshash_amd.so pulled in /opt/rocm's copy first, a later `import torch`
    would load a second runtime and fail with "No HIP GPUs are available" -- and streams / events /
    synchronisation would not be shared between the two. So when torch is installed, its bundled
    runtime is loaded first and libsshash_amd.so binds to it (SONAME match); without torch the
    system ROCm runtime is used."""
    if "torch" in sys.modules:
        return  # torch already loaded its runtime; ours will resolve to it
    try:
        import importlib.util

        spec = importlib.util.find_spec("torch")
        if spec is None or not spec.origin:
            return
        cand = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
        if os.path.exists(cand):
            C.CDLL(cand, mode=C.RTLD_GLOBAL)
    except Exception:
        pass


def _load() -> C.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    path = library_path()
    if not os.path.exists(path):
        raise ImportError(
            f"{path} is missing: the HIP extension has not been built. Run "
            "`python -c 'import __graft_entry__ as g; g.build()'` (or `make -C sshash_amd/csrc`). "
            "There is no pure-Python / CPU fallback for the lookup path."
        )
    _preload_hip_runtime()
    lib = C.CDLL(path)
    for name, (res, args) in _SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError here == ABI symbol missing: fail loudly
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def _check(status: int) -> None:
    if status != 0:
        raise SSHashError(status, _load().sshash_last_error().decode("utf-8", "replace"))


def build_info() -> dict:
    """sshash_build_info(): {"isa_guard": "guarded" | "plain", "arch": "gfx950"}"""
    return dict(kv.split("=", 1) for kv in _load().sshash_build_info().decode().split(";") if "=" in kv)


def device_count() -> int:
    return int(_load().sshash_device_count())


@dataclass
class LookupResult:
    """Struct-of-arrays form of lookup_result (reference include/util.hpp:38-62)."""

    kmer_id: np.ndarray
    kmer_id_in_string: Optional[np.ndarray] = None
    kmer_offset: Optional[np.ndarray] = None
    kmer_orientation: Optional[np.ndarray] = None
    string_id: Optional[np.ndarray] = None
    string_begin: Optional[np.ndarray] = None
    string_end: Optional[np.ndarray] = None
    minimizer_found: Optional[np.ndarray] = None


@dataclass
class StreamingQueryReport:
    """streaming_query_report (reference include/util.hpp:21-36)."""

    num_kmers: int = 0
    num_positive_kmers: int = 0
    num_negative_kmers: int = 0
    num_invalid_kmers: int = 0
    num_searches: int = 0
    num_extensions: int = 0


def encode_kmers(kmers: Sequence[Union[str, bytes]], k: int) -> np.ndarray:
    """ASCII k-mers -> contiguous (n, k) uint8 array as the *_ascii entry points expect."""
    buf = bytearray()
    for s in kmers:
        b = s.encode("ascii") if isinstance(s, str) else bytes(s)
        if len(b) < k:
            raise ValueError(f"k-mer shorter than k={k}: {s!r}")
        buf += b[:k]
    return np.frombuffer(bytes(buf), dtype=np.uint8).reshape(len(kmers), k)


KmerBatch = Union[np.ndarray, Sequence[str], Sequence[bytes], str, bytes]


def _reads_arrays(reads: Sequence[Union[str, bytes]]):
    """Reads in memory as the streaming calls want them -> (bases, offsets, n): the reads back to back as uint8 (one spare byte when
    there is none), the n + 1 uint64 offsets of their first bases, and their number."""
    chunks = [s.encode("ascii", "replace") if isinstance(s, str) else bytes(s) for s in reads]
    offsets = np.zeros(len(chunks) + 1, dtype=np.uint64)
    if chunks:
        offsets[1:] = np.cumsum([len(c) for c in chunks], dtype=np.uint64)
    return np.frombuffer(b"".join(chunks) or b"\0", dtype=np.uint8), offsets, len(chunks)


def _owned(pointer, ctype, shape) -> np.ndarray:
    """A copy of the C array at `pointer` (the library's rows live only as long as the callback that receives them)."""
    return np.ctypeslib.as_array(C.cast(pointer, C.POINTER(ctype)), shape=shape).copy()


def _u32_per_id(array, n: int, noun: str, per: str) -> np.ndarray:
    """`array` as n contiguous uint32, one per k-mer id or string id; refused where a cast would change a value."""
    array = np.asarray(array)
    if array.ndim != 1 or array.size != n or array.dtype.kind not in "ui":
        raise ValueError(f"{noun}: {n} unsigned integers, one per {per}")
    if array.dtype != np.uint32:
        if array.size and (int(array.min()) < 0 or int(array.max()) >> 32):
            raise ValueError(f"{noun}: every one of them within 32 bits")
        array = array.astype(np.uint32)
    return np.ascontiguousarray(array)


def _accumulator(array, n: int, dtype, noun: str, size: str) -> np.ndarray:
    """The caller's array that a call ORs or adds into (None: a zeroed one): n contiguous words of `dtype`, used in place."""
    if array is None:
        return np.zeros(n, dtype=dtype)
    if not (isinstance(array, np.ndarray) and array.dtype == dtype and array.ndim == 1 and array.size == n and array.flags.c_contiguous):
        raise ValueError(f"{noun}: a contiguous {np.dtype(dtype).name} array of {size} = {n} words")
    return array


class Dictionary:
    """Handle on one SSHash dictionary (host index + optional HBM replicas)."""

    def __init__(self, handle: int):
        self._h = C.c_void_p(handle)
        info = _Info()
        _check(_load().sshash_get_info(self._h, C.byref(info)))
        self._info = info

    # ---- construction / persistence ------------------------------------------------------
    @staticmethod
    def _config(k, m, seed, canonical, num_threads, lambda_, verbose, num_shards=1, shard_id=0) -> _BuildConfig:
        cfg = _BuildConfig()
        _load().sshash_build_config_default(C.byref(cfg))
        cfg.num_shards, cfg.shard_id = int(num_shards), int(shard_id)
        cfg.k, cfg.m, cfg.seed = int(k), int(m), int(seed)
        cfg.canonical = 1 if canonical else 0
        cfg.num_threads = int(num_threads)
        cfg.lambda_ = float(lambda_)
        cfg.verbose = 1 if verbose else 0
        return cfg

    @classmethod
    def build(cls, input_filename: str, k: int = 31, m: int = 20, seed: int = 1, canonical: bool = False,
              num_threads: int = 0, lambda_: float = 5.0, verbose: bool = False, num_shards: int = 1,
              shard_id: int = 0, weighted: bool = False) -> "Dictionary":
        """dictionary::build(input_filename, build_configuration) -- reference include/dictionary.hpp:28.
        num_shards > 1: build only the part of the sparse-and-skew index owned by `shard_id`.
        weighted: the FASTA headers carry the k-mer abundances (build_configuration::weighted)."""
        cfg = cls._config(k, m, seed, canonical, num_threads, lambda_, verbose, num_shards, shard_id)
        cfg.weighted = 1 if weighted else 0
        h = C.c_void_p()
        _check(_load().sshash_build_from_fasta(os.fsencode(input_filename), C.byref(cfg), C.byref(h)))
        return cls(h.value)

    @classmethod
    def build_from_packed(cls, words: np.ndarray, endpoints: np.ndarray, k: int = 31, m: int = 20, seed: int = 1,
                          canonical: bool = False, num_threads: int = 0, lambda_: float = 5.0,
                          verbose: bool = False, num_shards: int = 1, shard_id: int = 0) -> "Dictionary":
        words = np.ascontiguousarray(words, dtype=np.uint64)
        endpoints = np.ascontiguousarray(endpoints, dtype=np.uint64)
        need = (2 * int(endpoints[-1]) + 63) // 64
        if words.size < need:
            raise ValueError("packed words shorter than endpoints[-1] bases")
        cfg = cls._config(k, m, seed, canonical, num_threads, lambda_, verbose, num_shards, shard_id)
        h = C.c_void_p()
        _check(_load().sshash_build_from_packed(words.ctypes.data, endpoints.ctypes.data, endpoints.size - 1,
                                                C.byref(cfg), C.byref(h)))
        return cls(h.value)

    @classmethod
    def load(cls, index_filename: str) -> "Dictionary":
        h = C.c_void_p()
        _check(_load().sshash_load(os.fsencode(index_filename), C.byref(h)))
        return cls(h.value)

    def save(self, index_filename: str) -> None:
        _check(_load().sshash_save(self._h, os.fsencode(index_filename)))

    def close(self) -> None:
        if self._h:
            _load().sshash_free(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- accessors (reference include/dictionary.hpp:31-38) --------------------------------
    def k(self) -> int: return int(self._info.k)
    def m(self) -> int: return int(self._info.m)
    def canonical(self) -> bool: return bool(self._info.canonical)
    def num_kmers(self) -> int: return int(self._info.num_kmers)
    def num_strings(self) -> int: return int(self._info.num_strings)
    def num_bases(self) -> int: return int(self._info.num_bases)
    def num_minimizers(self) -> int: return int(self._info.num_minimizers)
    def num_bits(self) -> int: return int(self._info.num_bits)
    def words_per_kmer(self) -> int: return int(self._info.words_per_kmer)
    def vnum(self): return tuple(self._info.version)
    def num_shards(self) -> int: return int(self._info.num_shards)
    def shard_id(self) -> int: return int(self._info.shard_id)
    def weighted(self) -> bool: return bool(self._info.weighted)

    # ---- device residency -----------------------------------------------------------------
    def to_device(self, device: int = 0, table_shards: int = 1, table_shard_id: int = 0) -> "Dictionary":
        """Upload to `device`. table_shards > 1: the replica's super-k-mer table holds only its share of the keys
        (see sharded.py)."""
        if table_shards > 1:
            _check(_load().sshash_to_device_table_shard(self._h, int(device), int(table_shards), int(table_shard_id)))
            return self
        _check(_load().sshash_to_device(self._h, int(device)))
        return self

    def device_bytes(self, device: int = 0) -> int:
        out = C.c_uint64()
        _check(_load().sshash_device_bytes(self._h, int(device), C.byref(out)))
        return int(out.value)

    def bucket_stats(self) -> dict:
        """The statistics `sshash build --verbose` prints for the sparse and skew index (sshash_bucket_stats)."""
        out = (C.c_uint64 * 64)()
        _check(_load().sshash_bucket_stats(self._h, C.byref(out)))
        v = [int(x) for x in out]
        return {"num_minimizers": v[0], "num_minimizer_positions": v[1], "num_buckets_larger_than_1_not_in_skew_index": v[2],
                "num_minimizer_positions_of_buckets_larger_than_1": v[3], "num_buckets_in_skew_index": v[4],
                "num_minimizer_positions_of_buckets_in_skew_index": v[5], "num_kmers_in_skew_index": v[6], "max_bucket_size": v[7],
                "num_kmers_in_skew_partition": v[8:8 + v[35]], "buckets_with_n_positions": v[16:32], "num_kmers": v[32],
                "num_strings": v[33], "num_bases": v[34], "max_string_length": v[36]}

    def device_stats(self, device: int = 0) -> dict:
        out = (C.c_uint64 * 16)()
        _check(_load().sshash_device_stats(self._h, int(device), C.byref(out)))
        reasons = {0: None, 1: "disabled", 2: "minimizer shard", 3: "more than 2^39 bases", 4: "too many items for one build pass",
                   5: "not enough free HBM"}
        return {"bytes": int(out[0]), "directory_sectors": int(out[1]), "directory_overflow_sectors": int(out[2]),
                "directory_keys": int(out[3]), "sk_slots": int(out[4]), "sk_keys": int(out[5]), "sk_inline_keys": int(out[6]),
                "sk_deferred_keys": int(out[7]), "sk_slots_used": int(out[8]), "sk_heavy_keys": int(out[9]),
                "sk_heavy_kmers": int(out[10]), "sk_absent_reason": reasons.get(int(out[11]), str(int(out[11]))),
                "sk_bytes": int(out[12]), "sk_key_length": int(out[13]), "sk_load_factor": round(int(out[8]) / int(out[4]), 4) if int(out[4]) else 0.0}

    def device_table_histogram(self, device: int = 0) -> dict:
        """Keys of the super-k-mer table by number of occurrences (sshash_device_table_histogram)."""
        out = (C.c_uint64 * 32)()
        _check(_load().sshash_device_table_histogram(self._h, int(device), C.byref(out)))
        v = [int(x) for x in out]
        bins = ["1", "2", "3", "4", "5-8", "9-16", "17-64", "65-1024", ">1024"]
        return {"keys_by_occurrences": dict(zip(bins, v[0:9])), "super_kmers_by_occurrences_of_their_key": dict(zip(bins, v[9:18])),
                "super_kmers": v[18], "slots_asked_for": v[19]}

    def device_table(self, device: int = 0):
        """-> (info, words): the replica's super-k-mer table copied to the host as uint32 words, the keys' region first
        (sshash_device_table_export). A test and diagnosis call, sized for small replicas."""
        names = ("bytes", "key_buckets", "kmer_buckets", "key_bucket_bytes", "kmer_bucket_bytes", "key_length", "table_shards", "table_shard_id")
        raw = (C.c_uint64 * 8)()
        _check(_load().sshash_device_table_export(self._h, int(device), C.byref(raw), None, 0))
        words = np.zeros(int(raw[0]) // 4, dtype=np.uint32)
        if words.size:
            _check(_load().sshash_device_table_export(self._h, int(device), C.byref(raw), words.ctypes.data_as(C.c_void_p), words.nbytes))
        return dict(zip(names, (int(x) for x in raw))), words

    def _as_batch(self, kmers: KmerBatch):
        """-> (is_ascii, contiguous ndarray, n)"""
        if isinstance(kmers, (str, bytes)):
            kmers = [kmers]
        if isinstance(kmers, np.ndarray) and kmers.dtype == np.uint64:
            a = np.ascontiguousarray(kmers)
            w = self.words_per_kmer()
            if a.size % w:
                raise ValueError("packed k-mer array length is not a multiple of words_per_kmer")
            return False, a, a.size // w
        if isinstance(kmers, np.ndarray) and kmers.dtype == np.uint8:
            a = np.ascontiguousarray(kmers)
            if a.size % self.k():
                raise ValueError("ASCII k-mer buffer length is not a multiple of k")
            return True, a, a.size // self.k()
        a = encode_kmers(list(kmers), self.k())
        return True, np.ascontiguousarray(a), a.shape[0]

    def lookup(self, kmers: KmerBatch, check_reverse_complement: bool = True, full: bool = False,
               out: Optional[np.ndarray] = None) -> LookupResult:
        """Batched dictionary::lookup (reference src/dictionary.cpp:58-78). Host buffers in/out. `out`: a uint64 array
        of n entries to receive the ids (e.g. page-locked memory: with input and output both page-locked the library
        copies from and to them directly instead of staging through its own pinned lanes)."""
        is_ascii, a, n = self._as_batch(kmers)
        if out is not None and (out.dtype != np.uint64 or out.size != n or not out.flags["C_CONTIGUOUS"]):
            raise ValueError("out must be a contiguous uint64 array with one entry per k-mer")
        res = LookupResult(kmer_id=out if out is not None else np.empty(n, dtype=np.uint64))
        r = _Results()
        r.kmer_id = res.kmer_id.ctypes.data
        if full:
            for name in ("kmer_id_in_string", "kmer_offset", "string_id", "string_begin", "string_end"):
                arr = np.empty(n, dtype=np.uint64)
                setattr(res, name, arr)
                setattr(r, name, arr.ctypes.data)
            res.kmer_orientation = np.empty(n, dtype=np.int8)
            res.minimizer_found = np.empty(n, dtype=np.uint8)
            r.kmer_orientation = res.kmer_orientation.ctypes.data
            r.minimizer_found = res.minimizer_found.ctypes.data
        fn = _load().sshash_lookup_ascii if is_ascii else _load().sshash_lookup_packed
        _check(fn(self._h, a.ctypes.data, n, 1 if check_reverse_complement else 0, C.byref(r)))
        return res

    def is_member(self, kmers: KmerBatch, check_reverse_complement: bool = True) -> np.ndarray:
        """Batched dictionary::is_member (reference src/dictionary.cpp:80-88)."""
        is_ascii, a, n = self._as_batch(kmers)
        out = np.empty(n, dtype=np.uint8)
        fn = _load().sshash_is_member_ascii if is_ascii else _load().sshash_is_member_packed
        _check(fn(self._h, a.ctypes.data, n, 1 if check_reverse_complement else 0, out.ctypes.data))
        return out.astype(bool)

    def lookup_device(self, device: int, d_kmers: int, n: int, d_kmer_id: int, check_reverse_complement: bool = True,
                      stream: int = 0, ascii_input: bool = False, **optional_outputs: int) -> None:
        """Device-pointer entry point: all pointers are raw HBM addresses (e.g. torch ``.data_ptr()``)."""
        r = _Results()
        r.kmer_id = d_kmer_id
        for name, ptr in optional_outputs.items():
            setattr(r, name, ptr)
        fn = _load().sshash_lookup_ascii_device if ascii_input else _load().sshash_lookup_packed_device
        _check(fn(self._h, int(device), C.c_void_p(d_kmers), int(n), 1 if check_reverse_complement else 0, C.byref(r),
                  C.c_void_p(stream)))

    def neighbours(self, kmers: np.ndarray, check_reverse_complement: bool = True, full: bool = False) -> LookupResult:
        """Batched dictionary::kmer_neighbours (reference src/dictionary.cpp:111-126,176-187) over packed k-mers:
        every array of the result has 8 entries per query -- forward neighbours with A,C,T,G appended (index = 2-bit
        code of the character, the reference's alphabet order), then backward neighbours with A,C,T,G prepended."""
        a = np.ascontiguousarray(kmers, dtype=np.uint64)
        n = a.size // self.words_per_kmer()
        res = LookupResult(kmer_id=np.empty(8 * n, dtype=np.uint64))
        r = _Results()
        r.kmer_id = res.kmer_id.ctypes.data
        if full:
            for name in ("kmer_id_in_string", "kmer_offset", "string_id", "string_begin", "string_end"):
                arr = np.empty(8 * n, dtype=np.uint64)
                setattr(res, name, arr)
                setattr(r, name, arr.ctypes.data)
            res.kmer_orientation = np.empty(8 * n, dtype=np.int8)
            res.minimizer_found = np.empty(8 * n, dtype=np.uint8)
            r.kmer_orientation = res.kmer_orientation.ctypes.data
            r.minimizer_found = res.minimizer_found.ctypes.data
        _check(_load().sshash_neighbours_packed(self._h, a.ctypes.data, n, 1 if check_reverse_complement else 0, C.byref(r)))
        return res

    def string_size(self, string_ids: Iterable[int]) -> np.ndarray:
        """dictionary::string_size (reference src/dictionary.cpp:102-109): k-mers per string."""
        sids = np.ascontiguousarray(np.asarray(string_ids, dtype=np.uint64))
        out = np.empty(sids.size, dtype=np.uint64)
        _check(_load().sshash_string_size(self._h, sids.ctypes.data, sids.size, out.ctypes.data))
        return out

    def string_offsets(self, string_ids: Iterable[int]):
        """dictionary::string_offsets (reference include/dictionary.hpp:105-108): [begin, end) of each string, in bases."""
        sids = np.ascontiguousarray(np.asarray(string_ids, dtype=np.uint64))
        begin, end = np.empty(sids.size, dtype=np.uint64), np.empty(sids.size, dtype=np.uint64)
        _check(_load().sshash_string_offsets(self._h, sids.ctypes.data, sids.size, begin.ctypes.data, end.ctypes.data))
        return begin, end

    def string_neighbours(self, string_ids: Iterable[int], check_reverse_complement: bool = True) -> np.ndarray:
        """Batched dictionary::string_neighbours (reference src/dictionary.cpp:189-201): ids, 8 per string."""
        sids = np.ascontiguousarray(np.asarray(string_ids, dtype=np.uint64))
        ids = np.empty(8 * sids.size, dtype=np.uint64)
        r = _Results()
        r.kmer_id = ids.ctypes.data
        _check(_load().sshash_string_neighbours(self._h, sids.ctypes.data, sids.size, 1 if check_reverse_complement else 0, C.byref(r)))
        return ids

    def string_neighbours_device(self, device: int, d_string_ids: int, n: int, d_kmer_id: int, check_reverse_complement: bool = True,
                                 stream: int = 0, first_string: int = 0, **optional_outputs: int) -> None:
        """string_neighbours on the GPU: d_string_ids holds n uint64 string ids, or is 0 for the strings first_string + i; d_kmer_id (and
        every optional output) has room for 8*n entries. An id past the last string gives eight not-found entries. Asynchronous."""
        r = _Results()
        r.kmer_id = d_kmer_id
        for name, ptr in optional_outputs.items():
            setattr(r, name, ptr)
        _check(_load().sshash_string_neighbours_device(self._h, int(device), C.c_void_p(d_string_ids), int(first_string), int(n),
                                                       1 if check_reverse_complement else 0, C.byref(r), C.c_void_p(stream)))

    # ---- the dictionary as a graph (include/sshash_amd.h: sshash_string_link, sshash_kmer_adjacency) ----------------------------
    def string_links(self, begin: int = 0, end: Optional[int] = None, check_reverse_complement: bool = True):
        """The links of the strings [begin, end) (default: all) -> (link_offsets, links): one LINK_DTYPE record per neighbour of a
        string's end k-mers that the dictionary holds, the records of string begin + i at links[link_offsets[i]:link_offsets[i + 1]]
        in increasing flags & 7. A counting call, then the exact one, on the first resident replica. links_gfa() reads the flags."""
        end = self.num_strings() if end is None else int(end)
        begin = int(begin)
        if begin < 0 or end < 0:
            raise SSHashError(1, "string_links: string ids are non-negative")
        rc = 1 if check_reverse_complement else 0
        link_offsets = np.zeros(max(end - begin, 0) + 1, dtype=np.uint64)
        _check(_load().sshash_string_links(self._h, begin, end, rc, link_offsets.ctypes.data, None, 0))
        links = np.zeros(int(link_offsets[-1]), dtype=LINK_DTYPE)
        if links.size:
            _check(_load().sshash_string_links(self._h, begin, end, rc, link_offsets.ctypes.data, links.ctypes.data, links.size))
        return link_offsets, links

    def string_links_device(self, device: int, begin: int, end: int, d_link_offsets: int, d_links: int = 0, links_capacity: int = 0,
                            check_reverse_complement: bool = True, stream: int = 0) -> None:
        """Device buffers, asynchronous: d_link_offsets receives end - begin + 1 uint64 (exact whatever the capacity), d_links the
        records below links_capacity (0 with capacity 0: the counting call)."""
        _check(_load().sshash_string_links_device(self._h, int(device), int(begin), int(end), 1 if check_reverse_complement else 0,
                                                  C.c_void_p(d_link_offsets), C.c_void_p(d_links), int(links_capacity), C.c_void_p(stream)))

    def kmer_adjacency(self, begin: int = 0, end: Optional[int] = None, check_reverse_complement: bool = True) -> np.ndarray:
        """Which of its eight neighbours every k-mer of the ids [begin, end) (default: all) has in the dictionary -> uint8 masks: bit c
        the forward neighbour "ACTG"[c], bit 4 + c the backward one. On the first resident replica. adjacency_degrees() counts them."""
        end = self.num_kmers() if end is None else int(end)
        begin = int(begin)
        if begin < 0 or end < 0:
            raise SSHashError(1, "iterate: ids are non-negative")
        masks = np.zeros(max(end - begin, 0), dtype=np.uint8)
        _check(_load().sshash_kmer_adjacency(self._h, begin, end, 1 if check_reverse_complement else 0, masks.ctypes.data if masks.size else None))
        return masks

    def kmer_adjacency_device(self, device: int, begin: int, end: int, d_masks: int, check_reverse_complement: bool = True,
                              stream: int = 0) -> None:
        """The same into the device buffer d_masks (end - begin bytes), asynchronous on `stream`."""
        _check(_load().sshash_kmer_adjacency_device(self._h, int(device), int(begin), int(end), 1 if check_reverse_complement else 0,
                                                    C.c_void_p(d_masks), C.c_void_p(stream)))

    def neighbours_device(self, device: int, d_kmers: int, n: int, d_kmer_id: int, check_reverse_complement: bool = True,
                          stream: int = 0, **optional_outputs: int) -> None:
        """Device-pointer form: d_kmer_id (and every optional output) has room for 8*n entries."""
        r = _Results()
        r.kmer_id = d_kmer_id
        for name, ptr in optional_outputs.items():
            setattr(r, name, ptr)
        _check(_load().sshash_neighbours_packed_device(self._h, int(device), C.c_void_p(d_kmers), int(n),
                                                       1 if check_reverse_complement else 0, C.byref(r), C.c_void_p(stream)))

    def is_member_device(self, device: int, d_kmers: int, n: int, d_out: int, check_reverse_complement: bool = True,
                         stream: int = 0) -> None:
        _check(_load().sshash_is_member_packed_device(self._h, int(device), C.c_void_p(d_kmers), int(n),
                                                      1 if check_reverse_complement else 0, C.c_void_p(d_out),
                                                      C.c_void_p(stream)))

    # ---- access (host) ----------------------------------------------------------------------
    def access(self, kmer_id: int) -> str:
        buf = C.create_string_buffer(self.k())
        _check(_load().sshash_access(self._h, int(kmer_id), buf))
        return buf.raw.decode("ascii")

    def access_packed(self, kmer_ids: Iterable[int]) -> np.ndarray:
        ids = np.ascontiguousarray(np.asarray(kmer_ids, dtype=np.uint64))
        out = np.empty(ids.size * self.words_per_kmer(), dtype=np.uint64)
        _check(_load().sshash_access_packed(self._h, ids.ctypes.data, ids.size, out.ctypes.data))
        return out

    # ---- iteration: dictionary::begin / at_kmer_id / at_string_id (reference include/dictionary.hpp:84-121) -------------------
    def kmers(self, begin: int = 0, end: Optional[int] = None) -> np.ndarray:
        """The k-mers of the ids [begin, end) in id order (default: the whole dictionary), decoded on the host: flat uint64,
        words_per_kmer() words per k-mer, like access_packed."""
        end = self.num_kmers() if end is None else int(end)
        begin = int(begin)
        if begin < 0 or end < 0:
            raise SSHashError(1, "iterate: ids are non-negative")
        out = np.empty(max(end - begin, 0) * self.words_per_kmer(), dtype=np.uint64)
        _check(_load().sshash_iterate_packed(self._h, begin, end, out.ctypes.data if out.size else None))
        return out

    def string_kmers(self, string_id: int) -> np.ndarray:
        """dictionary::at_string_id: the k-mers of string `string_id`, through string_offsets."""
        sid = int(string_id)
        b, e = self.string_offsets([sid])
        km1 = self.k() - 1
        return self.kmers(int(b[0]) - sid * km1, int(e[0]) - (sid + 1) * km1)

    def kmers_device(self, device: int, begin: int, end: int, d_out: int, stream: int = 0) -> None:
        """The same on the GPU into the device buffer d_out ((end - begin) * words_per_kmer() uint64), asynchronous on `stream`."""
        _check(_load().sshash_iterate_packed_device(self._h, int(device), int(begin), int(end), C.c_void_p(d_out),
                                                    C.c_void_p(stream)))

    def check(self, device: int = 0) -> dict:
        """The reference's `sshash check` on the replica of `device`: every k-mer, taken by the iterator, looked up forward and
        reverse-complemented and asked is_member. Counts of failures; first_failure is the smallest failing id or INVALID_U64."""
        out = (C.c_uint64 * 8)()
        _check(_load().sshash_check_device(self._h, int(device), C.byref(out)))
        names = ("kmers", "forward_not_found", "forward_other_id", "reverse_complement_wrong", "not_member", "first_failure")
        return {name: int(out[i]) for i, name in enumerate(names)}

    # ---- weights ---------------------------------------------------------------------------------
    def weight(self, kmer_ids: Iterable[int]) -> np.ndarray:
        """Batched dictionary::weight (reference src/dictionary.cpp:96-100, include/weights.hpp:147-152), host side."""
        ids = np.ascontiguousarray(np.asarray(kmer_ids, dtype=np.uint64))
        out = np.empty(ids.size, dtype=np.uint64)
        _check(_load().sshash_weight(self._h, ids.ctypes.data, ids.size, out.ctypes.data))
        return out

    def weight_device(self, device: int, d_kmer_ids: int, n: int, d_out: int, stream: int = 0) -> None:
        _check(_load().sshash_weight_device(self._h, int(device), C.c_void_p(d_kmer_ids), int(n), C.c_void_p(d_out),
                                            C.c_void_p(stream)))

    def route_bucket_device(self, device: int, d_kmers: int, n: int, num_shards: int, d_cursors: int, d_send: int = 0,
                            d_slots: int = 0, check_reverse_complement: bool = True, stream: int = 0) -> None:
        """Count (d_send == 0) or scatter the messages of a routed batch; see include/sshash_amd.h."""
        _check(_load().sshash_route_bucket_device(self._h, int(device), C.c_void_p(d_kmers), int(n), int(num_shards),
                                                  1 if check_reverse_complement else 0, C.c_void_p(d_cursors),
                                                  C.c_void_p(d_send or None), C.c_void_p(d_slots or None), C.c_void_p(stream)))

    def route_bucket_by_key_device(self, device: int, d_kmers: int, n: int, num_shards: int, d_cursors: int, d_send: int = 0,
                                   d_slots: int = 0, stream: int = 0) -> None:
        """The same for table shards: one message per query, to the owner of its table key."""
        _check(_load().sshash_route_bucket_by_key_device(self._h, int(device), C.c_void_p(d_kmers), int(n), int(num_shards),
                                                         C.c_void_p(d_cursors), C.c_void_p(d_send or None),
                                                         C.c_void_p(d_slots or None), C.c_void_p(stream)))

    def route_combine_device(self, device: int, d_replies: int, d_slots: int, m: int, d_out: int, stream: int = 0) -> None:
        _check(_load().sshash_route_combine_device(self._h, int(device), C.c_void_p(d_replies), C.c_void_p(d_slots), int(m),
                                                   C.c_void_p(d_out), C.c_void_p(stream)))

    def sharded_lookup_device(self, device: int, num_ranks: int, by_table_key: bool, d_kmers: int, n: int, d_kmer_id: int,
                              counts_fn, data_fn, check_reverse_complement: bool = True, stream: int = 0) -> None:
        """sshash_sharded_lookup_device: route -> exchange -> lookup -> return -> combine in one call; the exchange is
        `counts_fn(send: list[int]) -> list[int]` and `data_fn(send_ptr, send_counts, recv_ptr, recv_counts, elem_bytes,
        stream) -> None` (device pointers)."""
        errors = []

        def counts(_ctx, send, recv):
            try:
                got = counts_fn([int(send[p]) for p in range(num_ranks)])
                for p in range(num_ranks):
                    recv[p] = int(got[p])
                return 0
            except Exception as e:  # noqa: BLE001 -- must not unwind through the C frames
                errors.append(e)
                return 1

        def data(_ctx, send, send_counts, recv, recv_counts, elem_bytes, hip_stream):
            try:
                data_fn(int(send or 0), [int(send_counts[p]) for p in range(num_ranks)], int(recv or 0),
                        [int(recv_counts[p]) for p in range(num_ranks)], int(elem_bytes), int(hip_stream or 0))
                return 0
            except Exception as e:  # noqa: BLE001
                errors.append(e)
                return 1

        x = _Exchange(None, EXCHANGE_COUNTS(counts), EXCHANGE_DATA(data))
        status = _load().sshash_sharded_lookup_device(self._h, int(device), int(num_ranks), 1 if by_table_key else 0, C.c_void_p(d_kmers),
                                                      int(n), 1 if check_reverse_complement else 0, C.c_void_p(d_kmer_id), C.byref(x),
                                                      C.c_void_p(stream))
        if errors:
            raise errors[0]
        _check(status)

    def route_device(self, device: int, d_kmers: int, n: int, num_shards: int, d_owner_fwd: int, d_owner_rc: int,
                     stream: int = 0) -> None:
        """Owner shard of each query's forward / reverse-complement minimizer (uint32 device arrays)."""
        _check(_load().sshash_route_packed_device(self._h, int(device), C.c_void_p(d_kmers), int(n), int(num_shards),
                                                  C.c_void_p(d_owner_fwd), C.c_void_p(d_owner_rc), C.c_void_p(stream)))

    def access_packed_device(self, device: int, d_ids: int, n: int, d_out: int, stream: int = 0) -> None:
        _check(_load().sshash_access_packed_device(self._h, int(device), C.c_void_p(d_ids), int(n), C.c_void_p(d_out),
                                                   C.c_void_p(stream)))

    # ---- streaming query ----------------------------------------------------------------------
    @staticmethod
    def _report(r: _Report) -> StreamingQueryReport:
        return StreamingQueryReport(r.num_kmers, r.num_positive_kmers, r.num_negative_kmers, r.num_invalid_kmers,
                                    r.num_searches, r.num_extensions)

    def streaming_query_from_file(self, filename: str, multiline: bool = False,
                                  per_read: Optional[Callable[[int, np.ndarray], Optional[int]]] = None) -> StreamingQueryReport:
        """dictionary::streaming_query_from_file (reference include/dictionary.hpp:81-82, src/query.cpp:118-175).

        per_read: called as per_read(first_read, rows) for one batch of the file after the other, in file order; rows is an (n, 6)
        uint64 array (the columns of StreamingQueryReport), row i for record first_read + i of the file -- every record has a row,
        those shorter than k included. A return value other than None / 0 stops the query (SSHashError, status 1); an exception
        raised by the callable stops it too and is raised again here."""
        if per_read is None:  # (the C ABI's own total: the only file call with the parallel FASTQ reader)
            r = _Report()
            _check(_load().sshash_streaming_query_from_file(self._h, os.fsencode(filename), 1 if multiline else 0, C.byref(r)))
            return self._report(r)
        return self._rows_from_file(
            lambda fn, r: _load().sshash_streaming_query_from_file_per_read(self._h, os.fsencode(filename), 1 if multiline else 0, fn, None, r),
            lambda rows, n: _owned(rows, C.c_uint64, (n, 6)), per_read, None)

    def _rows_from_file(self, call, block_of, per_read, empty):
        """The file calls that return a row per record. `call(fn, report)` is the bound C call with everything but the callback and the
        report filled in; `block_of(pointer, n)` makes the owned numpy block of one batch's rows. per_read(first_read, block) gets one
        batch after the other -> StreamingQueryReport; per_read=None: the blocks are kept -> (all of them, or `empty`;
        StreamingQueryReport). An exception of the callable is parked while the C frames return and raised again here."""
        r = _Report()
        raised, kept = [], []

        def hand_over(_ctx, first_read, n, rows):
            try:
                block = block_of(rows, int(n))
                if per_read is None:
                    kept.append(block)
                    return 0
                stop = per_read(int(first_read), block)
                return int(stop) if stop else 0
            except BaseException as e:  # (must not travel through the C frames)
                raised.append(e)
                return -1

        status = call(_PerReadFn(hand_over), C.byref(r))
        if raised:
            raise raised[0]
        _check(status)
        if per_read is None:
            return (np.concatenate(kept) if kept else empty), self._report(r)
        return self._report(r)

    def streaming_query(self, reads: Sequence[Union[str, bytes]]) -> StreamingQueryReport:
        """One streaming_query per read (reset between reads), reads given in memory."""
        bases, offsets, n = _reads_arrays(reads)
        r = _Report()
        _check(_load().sshash_streaming_query(self._h, bases.ctypes.data, offsets.ctypes.data, n, C.byref(r)))
        return self._report(r)

    def streaming_query_per_read(self, reads: Sequence[Union[str, bytes]]):
        """The streaming query's report for every read on its own -> (rows, StreamingQueryReport): rows is an (n, 6) uint64 array,
        row r = (num_kmers, num_positive_kmers, num_negative_kmers, num_invalid_kmers, num_searches, num_extensions) of read r (six
        zeros for a read shorter than k); the report is the batch's, the column sums of the rows."""
        bases, offsets, n = _reads_arrays(reads)
        rows = np.zeros((n, 6), dtype=np.uint64)
        r = _Report()
        _check(_load().sshash_streaming_query_per_read(self._h, bases.ctypes.data, offsets.ctypes.data, n,
                                                       rows.ctypes.data if n else None, C.byref(r)))
        return rows, self._report(r)

    def streaming_query_per_read_device(self, device: int, d_bases: int, d_read_offsets: int, num_reads: int, d_rows: int,
                                        d_report: int = 0, stream: int = 0, total_bases: int = 0) -> None:
        """Device buffers: d_rows receives num_reads rows of six uint64 (overwritten), d_report (0: none) six counters (accumulated
        into). `total_bases` as for streaming_query_device."""
        _check(_load().sshash_streaming_query_per_read_device(self._h, int(device), C.c_void_p(d_bases), C.c_void_p(d_read_offsets),
                                                              int(num_reads), int(total_bases), C.c_void_p(d_rows),
                                                              C.c_void_p(d_report), C.c_void_p(stream)))

    def streaming_runs(self, reads: Sequence[Union[str, bytes]]):
        """WHERE the reads hit -> (run_offsets, runs, StreamingQueryReport): the maximal runs of the streaming query (a run = a search and
        the extensions behind it; sshash_streaming_runs in include/sshash_amd.h). run_offsets: len(reads) + 1 uint64, CSR; runs: a
        RUN_DTYPE array, the records of read r at runs[run_offsets[r]:run_offsets[r + 1]] in increasing read_pos. expand_runs() gives
        the per-k-mer results back."""
        bases, offsets, n = _reads_arrays(reads)
        run_offsets = np.zeros(n + 1, dtype=np.uint64)
        capacity = 2 * n + 64  # a first guess; run_offsets says whether it was enough
        while True:
            runs = np.zeros(capacity, dtype=RUN_DTYPE)
            r = _Report()
            _check(_load().sshash_streaming_runs(self._h, bases.ctypes.data, offsets.ctypes.data, n, run_offsets.ctypes.data,
                                                 runs.ctypes.data, capacity, C.byref(r)))
            total = int(run_offsets[-1])
            if total <= capacity:
                return run_offsets, runs[:total], self._report(r)
            capacity = total

    def streaming_runs_device(self, device: int, d_bases: int, d_read_offsets: int, num_reads: int, d_run_offsets: int, d_runs: int,
                              runs_capacity: int, d_report: int = 0, stream: int = 0, total_bases: int = 0) -> None:
        """Device buffers: d_run_offsets receives num_reads + 1 uint64 (overwritten, exact whatever the capacity), d_runs the records
        below runs_capacity (0 with capacity 0: the counting call), d_report (0: none) six counters (accumulated into).
        `total_bases` as for streaming_query_device."""
        _check(_load().sshash_streaming_runs_device(self._h, int(device), C.c_void_p(d_bases), C.c_void_p(d_read_offsets), int(num_reads),
                                                    int(total_bases), C.c_void_p(d_run_offsets), C.c_void_p(d_runs), int(runs_capacity),
                                                    C.c_void_p(d_report), C.c_void_p(stream)))

    def streaming_runs_from_file(self, filename: str, multiline: bool = False,
                                 per_batch: Optional[Callable[[int, np.ndarray, np.ndarray], Optional[int]]] = None):
        """A query file answered like streaming_runs -- contigs of a multiline FASTA onto the unitigs, without loading the file first.
        per_batch(first_read, run_offsets, runs) is called for one batch of the file after the other, in file order: run_offsets has
        n + 1 uint64, [0] = 0, LOCAL to the batch -- the runs of record first_read + i of the file are runs[run_offsets[i]:
        run_offsets[i + 1]], a RUN_DTYPE array; every record has an entry, one shorter than k an empty range. A return value other
        than None / 0 stops the query (SSHashError), an exception raised by the callable stops it too and is raised again here.
        per_batch=None: -> (run_offsets, runs, StreamingQueryReport) of the whole file, stitched; otherwise -> StreamingQueryReport."""
        r = _Report()
        raised, kept = [], []

        def hand_over(_ctx, first_read, n, run_offsets, runs):
            try:
                offsets = _owned(run_offsets, C.c_uint64, (int(n) + 1,))
                total = int(offsets[-1])
                block = _owned(runs, C.c_uint8, (total * RUN_DTYPE.itemsize,)).view(RUN_DTYPE) if total else np.zeros(0, dtype=RUN_DTYPE)
                if per_batch is None:
                    kept.append((offsets, block))
                    return 0
                stop = per_batch(int(first_read), offsets, block)
                return int(stop) if stop else 0
            except BaseException as e:  # (must not travel through the C frames)
                raised.append(e)
                return -1

        status = _load().sshash_streaming_runs_from_file(self._h, os.fsencode(filename), 1 if multiline else 0, _ReadRunsFn(hand_over), None,
                                                         C.byref(r))
        if raised:
            raise raised[0]
        _check(status)
        if per_batch is not None:
            return self._report(r)
        stitched, base = [np.zeros(1, dtype=np.uint64)], 0
        for offsets, _ in kept:
            stitched.append(offsets[1:] + np.uint64(base))
            base += int(offsets[-1])
        runs = np.concatenate([block for _, block in kept]) if kept else np.zeros(0, dtype=RUN_DTYPE)
        return np.concatenate(stitched), runs, self._report(r)

    # ---- streaming cover: which k-mers of the dictionary a read set holds ---------------------------
    def cover_words(self) -> int:
        """Words of a cover bitmap: ceil(num_kmers / 64); k-mer id i is bit i & 63 of word i >> 6."""
        words = C.c_uint64(0)
        _check(_load().sshash_cover_words(self._h, C.byref(words)))
        return int(words.value)

    def _cover_array(self, cover) -> np.ndarray:
        return _accumulator(cover, self.cover_words(), np.uint64, "cover", "cover_words()")

    def streaming_cover(self, reads: Sequence[Union[str, bytes]], cover: Optional[np.ndarray] = None):
        """WHICH k-mers of the dictionary the reads hold -> (cover, StreamingQueryReport): the ids of all positive k-mers of the reads
        (the kmer_id values streaming_lookup returns, INVALID_U64 aside) as a bitmap of cover_words() uint64; `cover` (None: a zeroed one)
        is ORed into, in place, and returned. cover_to_ids() lists the ids."""
        bases, offsets, n = _reads_arrays(reads)
        cover = self._cover_array(cover)
        r = _Report()
        _check(_load().sshash_streaming_cover(self._h, bases.ctypes.data, offsets.ctypes.data, n, cover.ctypes.data, C.byref(r)))
        return cover, self._report(r)

    def streaming_cover_device(self, device: int, d_bases: int, d_read_offsets: int, num_reads: int, d_cover: int, d_report: int = 0,
                               stream: int = 0, total_bases: int = 0) -> None:
        """Device buffers: d_cover (cover_words() uint64) is ORed into, d_report (0: none) six counters (accumulated into).
        `total_bases` as for streaming_query_device."""
        _check(_load().sshash_streaming_cover_device(self._h, int(device), C.c_void_p(d_bases), C.c_void_p(d_read_offsets), int(num_reads),
                                                     int(total_bases), C.c_void_p(d_cover), C.c_void_p(d_report), C.c_void_p(stream)))

    def streaming_cover_from_file(self, filename: str, cover: Optional[np.ndarray] = None, multiline: bool = False):
        """A query file into one bitmap -> (cover, StreamingQueryReport); `cover` as for streaming_cover."""
        cover = self._cover_array(cover)
        r = _Report()
        _check(_load().sshash_streaming_cover_from_file(self._h, os.fsencode(filename), 1 if multiline else 0, cover.ctypes.data, C.byref(r)))
        return cover, self._report(r)

    def cover_string_counts(self, cover: np.ndarray):
        """-> (counts, total): covered k-mers of every string (num_strings uint64) and in all. CPU, no GPU needed."""
        cover = self._cover_array(cover)
        counts = np.zeros(max(self.num_strings(), 1), dtype=np.uint64)
        total = C.c_uint64(0)
        _check(_load().sshash_cover_string_counts(self._h, cover.ctypes.data if cover.size else counts.ctypes.data, counts.ctypes.data, C.byref(total)))
        return counts[:self.num_strings()], int(total.value)

    def cover_string_counts_device(self, device: int, d_cover: int, d_counts: int, d_total: int = 0, stream: int = 0) -> None:
        """Device buffers: d_counts (num_strings uint64) and d_total (0: none; one uint64) are overwritten."""
        _check(_load().sshash_cover_string_counts_device(self._h, int(device), C.c_void_p(d_cover), C.c_void_p(d_counts), C.c_void_p(d_total),
                                                         C.c_void_p(stream)))

    # ---- streaming depth: how often a read set holds each k-mer of the dictionary ---------------------
    def _depth_array(self, depth) -> np.ndarray:
        return _accumulator(depth, self.num_kmers(), np.uint32, "depth", "num_kmers()")

    def streaming_depth(self, reads: Sequence[Union[str, bytes]], depth: Optional[np.ndarray] = None):
        """HOW OFTEN the reads hold each k-mer of the dictionary -> (depth, StreamingQueryReport): depth[i] grows by the number of places
        where streaming_lookup over the same reads returns kmer_id == i (either strand, every occurrence; modulo 2^32, nothing
        saturates). `depth` (None: a zeroed one), num_kmers() uint32, is added into, in place, and returned."""
        bases, offsets, n = _reads_arrays(reads)
        depth = self._depth_array(depth)
        r = _Report()
        _check(_load().sshash_streaming_depth(self._h, bases.ctypes.data, offsets.ctypes.data, n, depth.ctypes.data, C.byref(r)))
        return depth, self._report(r)

    def streaming_depth_device(self, device: int, d_bases: int, d_read_offsets: int, num_reads: int, d_deltas: int, d_report: int = 0,
                               stream: int = 0, total_bases: int = 0) -> None:
        """Device buffers: d_deltas (num_kmers() uint32, a difference array: +1 where a run of ids begins, -1 behind it) is added into,
        d_report (0: none) six counters (accumulated into). `total_bases` as for streaming_query_device. depth_finish_device() turns the
        deltas into depths."""
        _check(_load().sshash_streaming_depth_device(self._h, int(device), C.c_void_p(d_bases), C.c_void_p(d_read_offsets), int(num_reads),
                                                     int(total_bases), C.c_void_p(d_deltas), C.c_void_p(d_report), C.c_void_p(stream)))

    def set_read_segments(self, kmers: Optional[int] = None, device_calls: bool = False) -> None:
        """Long reads: the streaming calls cut a read of more than `kmers` k-mers into segments of that many, one lane of the run kernel
        each, and give word for word what the uncut reads give (counters, rows, cover, depth). Opt-in: a new dictionary never segments. None or 0: the library's default S;
        SEGMENTS_OFF: never (a piece that holds a read above 2^16 bases then takes the position-parallel pipeline); else 1 .. 2^30.
        The host and file calls segment by themselves; the device calls only with `device_calls`. Never the runs, never a minimizer
        shard. Not to be changed while a call on this dictionary is in flight."""
        _check(_load().sshash_set_read_segments(self._h, 0 if kmers is None else int(kmers), 1 if device_calls else 0))

    def read_segments(self) -> dict:
        """-> {"kmers": S or SEGMENTS_OFF, "device_calls": bool, "segmented_launches": launches of the run kernel over a segment table}"""
        kmers, device_calls, launches = C.c_uint64(0), C.c_int(0), C.c_uint64(0)
        _check(_load().sshash_get_read_segments(self._h, C.byref(kmers), C.byref(device_calls), C.byref(launches)))
        return {"kmers": int(kmers.value), "device_calls": bool(device_calls.value), "segmented_launches": int(launches.value)}

    def depth_finish_device(self, device: int, d_deltas: int, d_depth: int, stream: int = 0) -> None:
        """Device buffers: d_depth[i] = d_deltas[0] + .. + d_deltas[i] modulo 2^32 over num_kmers() uint32; d_depth may be d_deltas."""
        _check(_load().sshash_depth_finish_device(self._h, int(device), C.c_void_p(d_deltas), C.c_void_p(d_depth), C.c_void_p(stream)))

    def streaming_depth_from_file(self, filename: str, depth: Optional[np.ndarray] = None, multiline: bool = False):
        """A query file into one depth array -> (depth, StreamingQueryReport); `depth` as for streaming_depth."""
        depth = self._depth_array(depth)
        r = _Report()
        _check(_load().sshash_streaming_depth_from_file(self._h, os.fsencode(filename), 1 if multiline else 0, depth.ctypes.data, C.byref(r)))
        return depth, self._report(r)

    def depth_string_sums(self, depth: np.ndarray):
        """-> (sums, total): the sum of depth over the ids of every string (num_strings uint64) and over all; the mean depth of string s
        is sums[s] / string_size(s). CPU, no GPU needed."""
        depth = self._depth_array(depth)
        sums = np.zeros(max(self.num_strings(), 1), dtype=np.uint64)
        total = C.c_uint64(0)
        _check(_load().sshash_depth_string_sums(self._h, depth.ctypes.data if depth.size else sums.ctypes.data, sums.ctypes.data, C.byref(total)))
        return sums[:self.num_strings()], int(total.value)

    def depth_string_sums_device(self, device: int, d_depth: int, d_sums: int, d_total: int = 0, stream: int = 0) -> None:
        """Device buffers: d_sums (num_strings uint64) and d_total (0: none; one uint64) are overwritten."""
        _check(_load().sshash_depth_string_sums_device(self._h, int(device), C.c_void_p(d_depth), C.c_void_p(d_sums), C.c_void_p(d_total),
                                                       C.c_void_p(stream)))

    # ---- streaming sums: reads scored against a value per k-mer --------------------------------------
    def _values_array(self, values) -> np.ndarray:
        """`values` as the calls want it (num_kmers() uint32, contiguous); None: the weights of a weighted dictionary, expanded per
        k-mer id through weight(), a chunk of ids at a time."""
        n = self.num_kmers()
        if values is None:
            if not self.weighted():
                raise ValueError("values=None asks for the dictionary's weights, and this dictionary stores none")
            out = np.empty(n, dtype=np.uint32)
            chunk = 1 << 22
            for at in range(0, n, chunk):
                w = self.weight(np.arange(at, min(n, at + chunk), dtype=np.uint64))
                if w.size and int(w.max()) >> 32:
                    raise ValueError("a weight does not fit 32 bits")
                out[at:at + w.size] = w
            return out
        return _u32_per_id(values, n, "values", "k-mer id")

    def value_prefix_device(self, device: int, d_values: int, d_prefix: int, at_least: int = 0, stream: int = 0) -> None:
        """Device buffers: d_prefix (num_kmers() + 1 uint64, overwritten) becomes the exclusive prefix sums of d_values (num_kmers()
        uint32) -- at_least >= 1: of whether d_values[i] >= at_least --, d_prefix[num_kmers()] the total. What streaming_sums_device reads."""
        _check(_load().sshash_value_prefix_device(self._h, int(device), C.c_void_p(d_values), int(at_least), C.c_void_p(d_prefix), C.c_void_p(stream)))

    def streaming_sums_device(self, device: int, d_bases: int, d_read_offsets: int, num_reads: int, d_prefix: int, d_sums: int,
                              d_report: int = 0, stream: int = 0, total_bases: int = 0) -> None:
        """Device buffers: d_sums receives num_reads rows of READ_SUM_DTYPE (overwritten; 8-byte aligned), out of d_prefix
        (value_prefix_device; only read); d_report (0: none) six counters (accumulated into). `total_bases` as for streaming_query_device."""
        _check(_load().sshash_streaming_sums_device(self._h, int(device), C.c_void_p(d_bases), C.c_void_p(d_read_offsets), int(num_reads),
                                                    int(total_bases), C.c_void_p(d_prefix), C.c_void_p(d_sums), C.c_void_p(d_report), C.c_void_p(stream)))

    def streaming_sums(self, reads: Sequence[Union[str, bytes]], values=None, at_least: int = 0):
        """Reads scored against a value per k-mer -> (sums, StreamingQueryReport): sums is a READ_SUM_DTYPE array, row r for read r:
        `sum` = the sum of values[id] over the places of the read where streaming_lookup returns a k-mer id (either strand, every
        occurrence; modulo 2^64) -- at_least >= 1: the number of those with values[id] >= at_least --, `positive_kmers` = the number of
        those places. `values`: num_kmers() integers within 32 bits (a depth array, say); None: the weights of a weighted dictionary."""
        values = self._values_array(values)
        bases, offsets, n = _reads_arrays(reads)
        sums = np.zeros(n, dtype=READ_SUM_DTYPE)
        r = _Report()
        _check(_load().sshash_streaming_sums(self._h, bases.ctypes.data, offsets.ctypes.data, n,
                                             values.ctypes.data if values.size else bases.ctypes.data, int(at_least),
                                             sums.ctypes.data if n else None, C.byref(r)))
        return sums, self._report(r)

    def streaming_sums_from_file(self, filename: str, values=None, at_least: int = 0, multiline: bool = False,
                                 per_read: Optional[Callable[[int, np.ndarray], Optional[int]]] = None):
        """A query file scored like streaming_sums. per_read(first_read, sums) is called for one batch of the file after the other, in
        file order, sums a READ_SUM_DTYPE array with row i for record first_read + i (every record has a row); a return value other
        than None / 0 stops the query (SSHashError), an exception raised by the callable stops it too and is raised again here.
        per_read=None: -> (sums of the whole file, StreamingQueryReport); otherwise -> StreamingQueryReport."""
        values = self._values_array(values)
        spare = np.zeros(1, dtype=np.uint32)
        return self._rows_from_file(
            lambda fn, r: _load().sshash_streaming_sums_from_file(self._h, os.fsencode(filename), 1 if multiline else 0,
                                                                  values.ctypes.data if values.size else spare.ctypes.data, int(at_least), fn, None, r),
            lambda rows, n: _owned(rows, C.c_uint64, (n, 2)).view(READ_SUM_DTYPE).reshape(n), per_read, np.zeros(0, dtype=READ_SUM_DTYPE))

    # ---- streaming classes: a read's positive k-mers by class of string --------------------------------
    def _labels_array(self, labels, num_classes: int) -> np.ndarray:
        """`labels` as the calls want it: num_strings() uint32, contiguous."""
        if not 1 <= int(num_classes) <= MAX_CLASSES:
            raise ValueError(f"num_classes: 1 .. {MAX_CLASSES}")
        return _u32_per_id(labels, self.num_strings(), "labels", "string id")

    def streaming_classes_device(self, device: int, d_bases: int, d_read_offsets: int, num_reads: int, d_labels: int, num_classes: int,
                                 d_rows: int, d_report: int = 0, stream: int = 0, total_bases: int = 0) -> None:
        """Device buffers: d_rows receives num_reads x num_classes uint32 (overwritten; 4-byte aligned), out of d_labels (num_strings()
        uint32, only read); d_report (0: none) six counters (accumulated into). `total_bases` as for streaming_query_device."""
        _check(_load().sshash_streaming_classes_device(self._h, int(device), C.c_void_p(d_bases), C.c_void_p(d_read_offsets), int(num_reads),
                                                       int(total_bases), C.c_void_p(d_labels), int(num_classes), C.c_void_p(d_rows),
                                                       C.c_void_p(d_report), C.c_void_p(stream)))

    def streaming_classes(self, reads: Sequence[Union[str, bytes]], labels, num_classes: int):
        """Whose a read's hits are -> (rows, StreamingQueryReport): rows is an (n, num_classes) uint32 array, rows[r, c] = the number of
        places of read r where streaming_lookup returns a k-mer whose string s has labels[s] == c (either strand, every occurrence;
        modulo 2^32). `labels`: num_strings() integers within 32 bits; a label >= num_classes is no class and counted in no column."""
        labels = self._labels_array(labels, num_classes)
        bases, offsets, n = _reads_arrays(reads)
        rows = np.zeros((n, int(num_classes)), dtype=np.uint32)
        r = _Report()
        _check(_load().sshash_streaming_classes(self._h, bases.ctypes.data, offsets.ctypes.data, n,
                                                labels.ctypes.data if labels.size else bases.ctypes.data, int(num_classes),
                                                rows.ctypes.data if n else None, C.byref(r)))
        return rows, self._report(r)

    def streaming_classes_from_file(self, filename: str, labels, num_classes: int, multiline: bool = False,
                                    per_read: Optional[Callable[[int, np.ndarray], Optional[int]]] = None):
        """A query file classified like streaming_classes. per_read(first_read, rows) is called for one batch of the file after the
        other, in file order, rows an (n, num_classes) uint32 array with row i for record first_read + i (every record has a row); a
        return value other than None / 0 stops the query (SSHashError), an exception raised by the callable stops it too and is raised
        again here. per_read=None: -> (rows of the whole file, StreamingQueryReport); otherwise -> StreamingQueryReport."""
        labels = self._labels_array(labels, num_classes)
        spare = np.zeros(1, dtype=np.uint32)
        return self._rows_from_file(
            lambda fn, r: _load().sshash_streaming_classes_from_file(self._h, os.fsencode(filename), 1 if multiline else 0,
                                                                     labels.ctypes.data if labels.size else spare.ctypes.data, int(num_classes), fn, None, r),
            lambda rows, n: _owned(rows, C.c_uint32, (n, int(num_classes))), per_read, np.zeros((0, int(num_classes)), dtype=np.uint32))

    def class_best_device(self, device: int, d_rows: int, num_reads: int, num_classes: int, d_best: int, stream: int = 0) -> None:
        """Device buffers: d_best receives num_reads rows of READ_CLASS_DTYPE (overwritten) out of d_rows (num_reads x num_classes uint32)."""
        _check(_load().sshash_class_best_device(self._h, int(device), C.c_void_p(d_rows), int(num_reads), int(num_classes), C.c_void_p(d_best),
                                                C.c_void_p(stream)))

    def class_totals_device(self, device: int, d_rows: int, num_reads: int, num_classes: int, d_totals: int, stream: int = 0) -> None:
        """Device buffers: d_totals receives num_classes uint64 (overwritten), the sum of every column of d_rows over the reads."""
        _check(_load().sshash_class_totals_device(self._h, int(device), C.c_void_p(d_rows), int(num_reads), int(num_classes), C.c_void_p(d_totals),
                                                  C.c_void_p(stream)))

    # ---- streaming anchors: a read's longest run -----------------------------------------------------
    def streaming_best_run_device(self, device: int, d_bases: int, d_read_offsets: int, num_reads: int, d_best: int, d_report: int = 0,
                                  stream: int = 0, total_bases: int = 0) -> None:
        """Device buffers: d_best receives num_reads records of RUN_DTYPE (overwritten; 16-byte aligned), d_report (0: none) six counters
        (accumulated into). `total_bases` as for streaming_query_device. Reads below 2^31 bases; segments never apply."""
        _check(_load().sshash_streaming_best_run_device(self._h, int(device), C.c_void_p(d_bases), C.c_void_p(d_read_offsets), int(num_reads),
                                                        int(total_bases), C.c_void_p(d_best), C.c_void_p(d_report), C.c_void_p(stream)))

    def streaming_best_run(self, reads: Sequence[Union[str, bytes]]):
        """The one place per read -> (best, StreamingQueryReport): best is a RUN_DTYPE array, best[r] the longest run of read r (the
        record of streaming_runs with the largest num_kmers & 0x7FFFFFFF, among equals the first in read order); a read without a hit
        has a record of zeros, num_kmers == 0."""
        bases, offsets, n = _reads_arrays(reads)
        best = np.zeros(n, dtype=RUN_DTYPE)
        r = _Report()
        _check(_load().sshash_streaming_best_run(self._h, bases.ctypes.data, offsets.ctypes.data, n,
                                                 best.ctypes.data if n else None, C.byref(r)))
        return best, self._report(r)

    def streaming_best_run_from_file(self, filename: str, multiline: bool = False,
                                     per_read: Optional[Callable[[int, np.ndarray], Optional[int]]] = None):
        """A query file answered like streaming_best_run. per_read(first_read, best) is called for one batch of the file after the other,
        in file order, best a RUN_DTYPE array with record i for record first_read + i of the file (every record has one); a return
        value other than None / 0 stops the query (SSHashError), an exception raised by the callable stops it too and is raised again
        here. per_read=None: -> (the records of the whole file, StreamingQueryReport); otherwise -> StreamingQueryReport."""
        return self._rows_from_file(
            lambda fn, r: _load().sshash_streaming_best_run_from_file(self._h, os.fsencode(filename), 1 if multiline else 0, fn, None, r),
            lambda best, n: _owned(best, C.c_uint8, (n * RUN_DTYPE.itemsize,)).view(RUN_DTYPE), per_read, np.zeros(0, dtype=RUN_DTYPE))

    def runs_best_device(self, device: int, d_run_offsets: int, d_runs: int, num_reads: int, d_best: int, stream: int = 0) -> None:
        """Device buffers: d_best receives num_reads records of RUN_DTYPE (overwritten), the longest of every read's records of a complete
        CSR (d_run_offsets: num_reads + 1 uint64; d_runs: d_run_offsets[num_reads] records)."""
        _check(_load().sshash_runs_best_device(self._h, int(device), C.c_void_p(d_run_offsets), C.c_void_p(d_runs), int(num_reads),
                                               C.c_void_p(d_best), C.c_void_p(stream)))

    def streaming_lookup(self, reads: Sequence[Union[str, bytes]], full: bool = False):
        """streaming_query::lookup for every k-mer of every read (reference include/streaming_query.hpp:56-109), batched.
        -> (list of LookupResult, one per read, len(read) - k + 1 entries each; StreamingQueryReport)."""
        bases, offsets, n = _reads_arrays(reads)
        total = max(int(offsets[-1]), 1)
        arrays = {"kmer_id": np.full(total, INVALID_U64, dtype=np.uint64)}
        if full:
            for name in ("kmer_id_in_string", "kmer_offset", "string_id", "string_begin", "string_end"):
                arrays[name] = np.full(total, INVALID_U64, dtype=np.uint64)
            arrays["kmer_orientation"] = np.ones(total, dtype=np.int8)
        r = _Results()
        for name, a in arrays.items():
            setattr(r, name, a.ctypes.data)
        rep = _Report()
        _check(_load().sshash_streaming_lookup(self._h, bases.ctypes.data, offsets.ctypes.data, n, C.byref(r), C.byref(rep)))
        per_read = []
        k = self.k()
        for i in range(n):
            lo = int(offsets[i])
            kmers = max(0, int(offsets[i + 1]) - lo - k + 1)
            per_read.append(LookupResult(**{name: a[lo:lo + kmers] for name, a in arrays.items()}))
        return per_read, self._report(rep)

    def streaming_lookup_device(self, device: int, d_bases: int, d_read_offsets: int, num_reads: int, total_bases: int,
                                d_kmer_id: int, d_report: int = 0, stream: int = 0, **optional_outputs: int) -> None:
        r = _Results()
        r.kmer_id = d_kmer_id
        for name, ptr in optional_outputs.items():
            setattr(r, name, ptr)
        _check(_load().sshash_streaming_lookup_device(self._h, int(device), C.c_void_p(d_bases), C.c_void_p(d_read_offsets),
                                                      int(num_reads), int(total_bases), C.byref(r), C.c_void_p(d_report), C.c_void_p(stream)))

    def streaming_query_device(self, device: int, d_bases: int, d_read_offsets: int, num_reads: int, d_report: int,
                               stream: int = 0, total_bases: int = 0) -> None:
        """`total_bases` = read_offsets[num_reads] when the caller knows it: the call then only enqueues work (0: it reads the
        eight bytes back and waits for the stream first)."""
        _check(_load().sshash_streaming_query_device(self._h, int(device), C.c_void_p(d_bases), C.c_void_p(d_read_offsets),
                                                     int(num_reads), int(total_bases), C.c_void_p(d_report), C.c_void_p(stream)))


def expand_runs(run_offsets, runs, read_lengths, k: int):
    """The inverse of Dictionary.streaming_runs: one LookupResult per read with len(read) - k + 1 entries each of kmer_id, string_id,
    kmer_id_in_string and kmer_orientation -- what streaming_lookup(reads, full=True) returns in those fields for every POSITIVE k-mer;
    k-mers outside every run are INVALID_U64 / +1. (That +1 is NOT always streaming_lookup's: for a negative k-mer the lookup reports the
    strand of its last probe, -1 in a regular dictionary, which no run carries.) k-mer j of a run starts at base read_pos + j and has kmer_id +/- j and kmer_id_in_string +/- j (+ forward, -
    backward), the run's string_id and orientation."""
    run_offsets = np.asarray(run_offsets, dtype=np.uint64)
    runs = np.asarray(runs, dtype=RUN_DTYPE)
    if len(run_offsets) != len(read_lengths) + 1:
        raise ValueError("run_offsets has len(read_lengths) + 1 entries")
    out = []
    for r, length in enumerate(read_lengths):
        n = max(0, int(length) - int(k) + 1)
        ids = np.full(n, INVALID_U64, dtype=np.uint64)
        sid = np.full(n, INVALID_U64, dtype=np.uint64)
        in_string = np.full(n, INVALID_U64, dtype=np.uint64)
        ori = np.ones(n, dtype=np.int8)
        for rec in runs[int(run_offsets[r]):int(run_offsets[r + 1])]:
            count = int(rec["num_kmers"]) & 0x7FFFFFFF
            at = int(rec["read_pos"])
            if count == 0 or at + count > n:
                raise ValueError(f"read {r}: a run of {count} k-mers at base {at} does not fit {n} k-mers")
            backward = (int(rec["num_kmers"]) & RUN_BACKWARD) != 0
            step = np.arange(count, dtype=np.uint64)
            ids[at:at + count] = rec["kmer_id"] - step if backward else rec["kmer_id"] + step
            in_string[at:at + count] = rec["kmer_id_in_string"] - step if backward else rec["kmer_id_in_string"] + step
            sid[at:at + count] = rec["string_id"]
            ori[at:at + count] = -1 if backward else 1
        out.append(LookupResult(kmer_id=ids, kmer_id_in_string=in_string, kmer_orientation=ori, string_id=sid))
    return out


def write_weighted_fasta(d: "Dictionary", depth, path: str) -> None:
    """The dictionary's strings in id order with `depth` (num_kmers() counts, one per k-mer id) as their abundances, in the format a
    weighted build reads: '>s LN:i:len ab:Z:c0 c1 ...' and the string on the next line (gzip when `path` ends in .gz).
    Dictionary.build(path, k, m, weighted=True) over the file gives a dictionary with the same ids whose weight(i) is depth[i];
    zeros are written as they are. CPU only: the strings come from the k-mer iterator, a few thousand strings at a time."""
    import gzip

    depth = np.asarray(depth)
    n_kmers, n_strings, k = d.num_kmers(), d.num_strings(), d.k()
    if depth.ndim != 1 or depth.size != n_kmers or depth.dtype.kind not in "ui":
        raise ValueError(f"depth: {n_kmers} integer counts, one per k-mer id")
    if depth.dtype.kind == "i" and depth.size and int(depth.min()) < 0:
        raise ValueError("depth: counts are not negative")
    with (gzip.open(path, "wt") if str(path).endswith(".gz") else open(path, "w")) as f:
        for s, first, text in _strings_in_id_order(d):
            counts = " ".join(map(str, depth[first:first + len(text) - k + 1].tolist()))
            f.write(f">{s} LN:i:{len(text)} ab:Z:{counts}\n{text}\n")


def _strings_in_id_order(d: "Dictionary"):
    """-> (string id, id of its first k-mer, the string) for every string of the dictionary, decoded on the CPU through the k-mer
    iterator, a few thousand strings at a time."""
    n_strings, k = d.num_strings(), d.k()
    letters = np.frombuffer(b"ACTG", dtype=np.uint8)  # 2-bit code -> character
    W = d.words_per_kmer()
    last_word, last_shift = (k - 1) // 32, np.uint64(2 * ((k - 1) % 32))
    begin, end = d.string_offsets(np.arange(n_strings, dtype=np.uint64))
    sid = np.arange(n_strings, dtype=np.uint64)
    first_id = (begin - sid * np.uint64(k - 1)).astype(np.int64)  # ids of string s: [first_id[s], first_id[s] + size[s])
    size = (end - begin).astype(np.int64) - (k - 1)
    s0 = 0
    while s0 < n_strings:
        s1 = s0 + 1
        while s1 < n_strings and s1 - s0 < 4096 and int(first_id[s1]) - int(first_id[s0]) < (1 << 22):
            s1 += 1
        lo, hi = int(first_id[s0]), int(first_id[s1 - 1] + size[s1 - 1])
        packed = d.kmers(lo, hi).reshape(-1, W)
        last = letters[((packed[:, last_word] >> last_shift) & np.uint64(3)).astype(np.uint8)]  # the last character of every k-mer
        for s in range(s0, s1):
            a, n = int(first_id[s]) - lo, int(size[s])
            head = np.empty(k - 1, dtype=np.uint8)  # the first k-mer's characters but its last
            for i in range(k - 1):
                head[i] = letters[int((int(packed[a, i // 32]) >> (2 * (i % 32))) & 3)]
            yield s, lo + a, (head.tobytes() + last[a:a + n].tobytes()).decode("ascii")
        s0 = s1


def link_degrees(link_offsets, links):
    """-> (out_at_end, out_at_start): per string of a string_links() range, how many links leave its end and its start."""
    link_offsets = np.asarray(link_offsets, dtype=np.uint64)
    n = link_offsets.size - 1
    owner = np.repeat(np.arange(n), np.diff(link_offsets).astype(np.int64))
    at_start = (links["flags"] & 4) != 0
    return (np.bincount(owner[~at_start], minlength=n).astype(np.uint8), np.bincount(owner[at_start], minlength=n).astype(np.uint8))


def adjacency_degrees(masks):
    """-> (forward, backward): per k-mer of a kmer_adjacency() range, how many of its forward and of its backward neighbours the
    dictionary holds."""
    masks = np.asarray(masks, dtype=np.uint8)
    ones = np.array([bin(i).count("1") for i in range(16)], dtype=np.uint8)
    return ones[masks & 15], ones[masks >> 4]


def links_gfa(links):
    """The sign rule of include/sshash_amd.h -> (is_end_to_end, from_sign, to_sign): which links join two string ends (the L lines of
    a GFA), and the orientation of both strings in them, as arrays of b'+' / b'-'."""
    flags = links["flags"]
    at_start, rc, first, last = ((flags & bit) != 0 for bit in (4, 8, 16, 32))
    end_to_end = np.where(at_start, np.where(rc, first, last), np.where(rc, last, first))
    sign = np.array([b"-", b"+"])
    return end_to_end, sign[(~at_start).astype(np.int64)], sign[(rc == at_start).astype(np.int64)]


def write_gfa(d: "Dictionary", path: str, link_offsets=None, links=None) -> None:
    """The dictionary as a GFA 1: H, one S line per string (named by its id) and one 'L from sign to sign (k-1)M' line per end-to-end
    link, each as seen from its from_string -- a link between two string ends appears once from either side, as BCALM-style GFAs
    list them. Links that land inside a string (junctions inside stitched strings) have no L line. `links` None: string_links() over
    all strings (needs a replica); the strings are decoded on the CPU. gzip when `path` ends in .gz."""
    import gzip

    if links is None:
        link_offsets, links = d.string_links()
    end_to_end, from_sign, to_sign = links_gfa(links)
    overlap = f"{d.k() - 1}M"
    with (gzip.open(path, "wt") if str(path).endswith(".gz") else open(path, "w")) as f:
        f.write("H\tVN:Z:1.0\n")
        for s, _, text in _strings_in_id_order(d):
            f.write(f"S\t{s}\t{text}\tLN:i:{len(text)}\n")
        for i in np.flatnonzero(end_to_end):
            f.write(f"L\t{int(links['from_string'][i])}\t{from_sign[i].decode()}\t{int(links['to_string'][i])}\t{to_sign[i].decode()}\t{overlap}\n")


def _class_rows(rows) -> np.ndarray:
    """`rows` as the finish calls want them: (reads, classes) uint32, contiguous. Refused as the labels are: nothing is cast that would
    change a count."""
    rows = np.asarray(rows)
    if rows.ndim != 2 or not 1 <= rows.shape[1] <= MAX_CLASSES or rows.dtype.kind not in "ui":
        raise ValueError(f"rows: (reads, classes) unsigned integers with 1 .. {MAX_CLASSES} classes")
    if rows.dtype != np.uint32:
        if rows.size and (int(rows.min()) < 0 or int(rows.max()) >> 32):
            raise ValueError("rows: every count within 32 bits")
        rows = rows.astype(np.uint32)
    return np.ascontiguousarray(rows)


def class_best(rows) -> np.ndarray:
    """The finish of streaming_classes on the host (sshash_class_best) -> a READ_CLASS_DTYPE array, one entry per row: the class with the
    largest count (among equals the smallest), that count, the largest count among the other classes, the row's sum modulo 2^32; a
    row of zeros: (NO_CLASS, 0, 0, 0)."""
    rows = _class_rows(rows)
    best = np.zeros(rows.shape[0], dtype=READ_CLASS_DTYPE)
    _check(_load().sshash_class_best(rows.ctypes.data if rows.shape[0] else None, rows.shape[0], rows.shape[1],
                                     best.ctypes.data if rows.shape[0] else None))
    return best


def class_totals(rows) -> np.ndarray:
    """The 64-bit sum of every column of streaming_classes' rows over the reads (sshash_class_totals): the sample's profile by class."""
    rows = _class_rows(rows)
    totals = np.zeros(rows.shape[1], dtype=np.uint64)
    _check(_load().sshash_class_totals(rows.ctypes.data if rows.shape[0] else None, rows.shape[0], rows.shape[1], totals.ctypes.data))
    return totals


def runs_best(run_offsets, runs) -> np.ndarray:
    """The finish of streaming_runs on the host (sshash_runs_best) -> a RUN_DTYPE array, one record per read: the record of
    runs[run_offsets[r]:run_offsets[r + 1]] with the largest num_kmers & 0x7FFFFFFF, among equals the first; zeros for an empty range."""
    run_offsets = np.asarray(run_offsets)
    if run_offsets.ndim != 1 or run_offsets.size == 0 or run_offsets.dtype.kind not in "ui":
        raise ValueError("run_offsets: num_reads + 1 unsigned integers")
    run_offsets = np.ascontiguousarray(run_offsets, dtype=np.uint64)
    runs = np.asarray(runs)
    if runs.dtype != RUN_DTYPE or runs.ndim != 1:
        raise ValueError("runs: a one-dimensional RUN_DTYPE array")
    runs = np.ascontiguousarray(runs)
    n = run_offsets.size - 1
    if n and (int(run_offsets[0]) != 0 or (np.diff(run_offsets.astype(np.int64)) < 0).any() or int(run_offsets[-1]) > runs.size):
        raise ValueError("run_offsets: a CSR over the records of runs, from 0 and never going down")
    best = np.zeros(n, dtype=RUN_DTYPE)
    _check(_load().sshash_runs_best(run_offsets.ctypes.data, runs.ctypes.data if runs.size else None, n, best.ctypes.data if n else None))
    return best


def cover_to_ids(cover) -> np.ndarray:
    """The k-mer ids a cover bitmap holds, ascending (uint64): id i is bit i & 63 of word i >> 6."""
    words = np.ascontiguousarray(cover, dtype="<u8")
    bits = np.unpackbits(words.view(np.uint8), bitorder="little")
    return np.flatnonzero(bits).astype(np.uint64)


def ids_to_cover(ids, words: int) -> np.ndarray:
    """The inverse: a bitmap of `words` uint64 with the bits of `ids` set (INVALID_U64 entries are skipped)."""
    ids = np.asarray(ids, dtype=np.uint64).reshape(-1)
    ids = ids[ids != np.uint64(INVALID_U64)]
    cover = np.zeros(int(words), dtype=np.uint64)
    np.bitwise_or.at(cover, (ids >> np.uint64(6)).astype(np.int64), np.uint64(1) << (ids & np.uint64(63)))
    return cover
