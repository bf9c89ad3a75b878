"""The streaming sums (per read, the sum of a value per k-mer over the read's positive k-mers, and their number) at the C ABI and in the
binding, as far as a machine without a GPU can tell: the symbols are declared, exported, bound and present in the facade; a row is 16
bytes; argument errors are reported before anything else and write nothing; num_reads == 0 is no work; a dictionary that is not
resident fails with SSHASH_ERR_NO_DEVICE; values=None wants a weighted dictionary."""
from __future__ import annotations

import ctypes as C
import os
import re

import numpy as np
import pytest

import sshash_amd
from sshash_amd import _binding as B
from conftest import FASTQ, ROOT

SYMBOLS = ("sshash_value_prefix_device", "sshash_streaming_sums", "sshash_streaming_sums_device", "sshash_streaming_sums_from_file")
METHODS = ("value_prefix_device", "streaming_sums", "streaming_sums_device", "streaming_sums_from_file")
ERR_ARGUMENT, ERR_NO_DEVICE = 1, 5


def _batch(reads):
    chunks = [r.encode() for r in reads]
    offsets = np.zeros(len(chunks) + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum([len(c) for c in chunks], dtype=np.uint64)
    return np.frombuffer(b"".join(chunks) or b"\0", dtype=np.uint8), offsets


def test_symbols_are_declared_exported_bound_and_in_the_facade():
    header = open(os.path.join(ROOT, "include", "sshash_amd.h")).read()
    facade = open(os.path.join(ROOT, "include", "sshash_amd.hpp")).read()
    lib = C.CDLL(sshash_amd.library_path())
    bound = B._load()
    for name in SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert hasattr(lib, name), name
        assert name in B.C_ABI_SYMBOLS
        assert getattr(bound, name).argtypes is not None and getattr(bound, name).restype is C.c_int
        assert name + "(" in facade, name
    for method in METHODS:
        assert callable(getattr(sshash_amd.Dictionary, method)), method
        assert re.search(r"\b" + method + r"\s*\(", facade), method
    # what the header has to say: semantics, alignment, footprints, modulo arithmetic, which calls segment, what a shard returns
    section = header[header.index("SCORING reads"):header.index("sshash_streaming_sums_from_file(")]
    for words in ("modulo 2^64", "8-byte alignment", "8 bytes per k-mer", "OVERWRITTEN", "minimizer shard", "sshash_set_read_segments", "memory pool"):
        assert words in section, words


def test_a_row_is_sixteen_bytes():
    """sizeof(sshash_read_sum) == 16: the header's struct, the dtype and the static_assert of the library's own source agree"""
    header = open(os.path.join(ROOT, "include", "sshash_amd.h")).read()
    body = re.search(r"typedef struct sshash_read_sum \{(.*?)\} sshash_read_sum;", header, re.S).group(1)
    assert re.findall(r"uint64_t\s+(\w+);", body) == ["sum", "positive_kmers"]
    assert sshash_amd.READ_SUM_DTYPE.itemsize == 16 and sshash_amd.READ_SUM_DTYPE.names == ("sum", "positive_kmers")
    assert sshash_amd.READ_SUM_DTYPE.fields["sum"][1] == 0 and sshash_amd.READ_SUM_DTYPE.fields["positive_kmers"][1] == 8
    capi = open(os.path.join(ROOT, "sshash_amd", "csrc", "capi.cpp")).read()
    assert "static_assert(sizeof(sshash_read_sum) == 2 * sizeof(uint64_t)" in capi


def test_argument_errors_come_first(case_skew_regular):
    """a null dictionary, or null bases / read_offsets / values or prefix / sums with num_reads > 0: SSHASH_ERR_ARGUMENT whether or not a
    device is there, and nothing is written"""
    d = case_skew_regular.dict
    lib = B._load()
    bases, offsets = _batch([case_skew_regular.sequences[0], "ACGT"])
    values = np.full(d.num_kmers(), 3, dtype=np.uint32)
    prefix = np.full(d.num_kmers() + 1, 0x55, dtype=np.uint64)
    sums = np.full(2, 0x77, dtype=sshash_amd.READ_SUM_DTYPE)
    rep = B._Report(1, 2, 3, 4, 5, 6)
    b, o, v, p, s = bases.ctypes.data, offsets.ctypes.data, values.ctypes.data, prefix.ctypes.data, sums.ctypes.data
    fn = B._PerReadFn(lambda *a: 0)
    host, device, from_file, make_prefix = (lib.sshash_streaming_sums, lib.sshash_streaming_sums_device, lib.sshash_streaming_sums_from_file,
                                            lib.sshash_value_prefix_device)
    assert host(None, b, o, 2, v, 0, s, C.byref(rep)) == ERR_ARGUMENT
    assert rep.num_kmers == 1  # (a null dictionary: not even the report is touched)
    assert host(d._h, None, o, 2, v, 0, s, None) == ERR_ARGUMENT
    assert host(d._h, b, None, 2, v, 0, s, None) == ERR_ARGUMENT
    assert host(d._h, b, o, 2, None, 0, s, None) == ERR_ARGUMENT
    assert host(d._h, b, o, 2, v, 0, None, None) == ERR_ARGUMENT
    assert lib.sshash_last_error()
    # (host pointers stand in for device pointers: the call must refuse before it touches them)
    assert device(None, 0, b, o, 2, 0, p, s, None, None) == ERR_ARGUMENT
    assert device(d._h, 0, None, o, 2, 0, p, s, None, None) == ERR_ARGUMENT
    assert device(d._h, 0, b, None, 2, 0, p, s, None, None) == ERR_ARGUMENT
    assert device(d._h, 0, b, o, 2, 0, None, s, None, None) == ERR_ARGUMENT
    assert device(d._h, 0, b, o, 2, 0, p, None, None, None) == ERR_ARGUMENT
    assert make_prefix(None, 0, v, 0, p, None) == ERR_ARGUMENT
    assert make_prefix(d._h, 0, None, 0, p, None) == ERR_ARGUMENT
    assert make_prefix(d._h, 0, v, 0, None, None) == ERR_ARGUMENT
    assert from_file(None, os.fsencode(FASTQ), 0, v, 0, fn, None, None) == ERR_ARGUMENT
    assert from_file(d._h, None, 0, v, 0, fn, None, None) == ERR_ARGUMENT
    assert from_file(d._h, os.fsencode(FASTQ), 0, None, 0, fn, None, None) == ERR_ARGUMENT
    assert from_file(d._h, os.fsencode(FASTQ), 0, v, 0, B._PerReadFn(), None, None) == ERR_ARGUMENT
    assert (prefix == 0x55).all() and (sums["sum"] == 0x77).all() and (sums["positive_kmers"] == 0x77).all() and (values == 3).all()
    with pytest.raises(ValueError):
        d.streaming_sums(["ACGT"], values=np.zeros(d.num_kmers() + 1, dtype=np.uint32))
    with pytest.raises(ValueError):
        d.streaming_sums(["ACGT"], values=np.zeros(d.num_kmers(), dtype=np.float64))
    with pytest.raises(ValueError):
        d.streaming_sums(["ACGT"], values=np.full(d.num_kmers(), 1 << 32, dtype=np.uint64))


def test_no_reads_is_no_work_for_the_host_call(case_skew_regular):
    """num_reads == 0 succeeds without a device and touches nothing but the report, which it zeroes"""
    d = case_skew_regular.dict
    lib = B._load()
    values = np.full(d.num_kmers(), 3, dtype=np.uint32)
    sums = np.full(2, 0x33, dtype=sshash_amd.READ_SUM_DTYPE)
    rep = B._Report(1, 2, 3, 4, 5, 6)
    assert lib.sshash_streaming_sums(d._h, None, None, 0, values.ctypes.data, 0, sums.ctypes.data, C.byref(rep)) == 0
    assert (sums["sum"] == 0x33).all() and (sums["positive_kmers"] == 0x33).all() and rep.num_kmers == 0 and rep.num_searches == 0
    assert lib.sshash_streaming_sums(d._h, None, None, 0, None, 0, None, None) == 0
    got, report = d.streaming_sums([], values)
    assert got.dtype == sshash_amd.READ_SUM_DTYPE and got.shape == (0,) and report == B.StreamingQueryReport()


def test_a_dictionary_that_is_not_resident_is_no_device(tmp_path):
    """a dictionary of its own that nobody uploaded: every call that needs a replica says SSHASH_ERR_NO_DEVICE, with or without a GPU in
    the machine, and writes nothing"""
    rng = np.random.default_rng(3)
    path = str(tmp_path / "tiny.fa")
    with open(path, "w") as f:
        for i in range(40):
            f.write(f">{i}\n{''.join('ACGT'[c] for c in rng.integers(0, 4, int(rng.integers(15, 300))))}\n")
    d = sshash_amd.Dictionary.build(path, k=15, m=7)
    lib = B._load()
    reads = ["ACGTTGCATGCATGCAAGTCGATCGAT", "ACGT"]
    values = np.full(d.num_kmers(), 3, dtype=np.uint32)
    with pytest.raises(sshash_amd.SSHashError) as e:
        d.streaming_sums(reads, values)
    assert e.value.status == ERR_NO_DEVICE
    with pytest.raises(sshash_amd.SSHashError) as e:
        d.streaming_sums_from_file(path, values)
    assert e.value.status == ERR_NO_DEVICE
    bases, offsets = _batch(reads)
    prefix = np.full(d.num_kmers() + 1, 0x55, dtype=np.uint64)
    sums = np.full(2, 0x77, dtype=sshash_amd.READ_SUM_DTYPE)
    rep = np.full(6, 9, dtype=np.uint64)
    assert lib.sshash_streaming_sums_device(d._h, 0, bases.ctypes.data, offsets.ctypes.data, 2, 0, prefix.ctypes.data, sums.ctypes.data,
                                            rep.ctypes.data, None) == ERR_NO_DEVICE
    assert lib.sshash_value_prefix_device(d._h, 0, values.ctypes.data, 0, prefix.ctypes.data, None) == ERR_NO_DEVICE
    assert (prefix == 0x55).all() and (sums["sum"] == 0x77).all() and (rep == 9).all()


def test_an_unsupported_extension_is_an_empty_report_without_any_device(tmp_path):
    """a query file whose extension says nothing: the call says "unsupported query file format" and returns before any device is asked for -- this dictionary is resident
    nowhere, and the call succeeds --, the report all zeros, per_read never called, no rows"""
    rng = np.random.default_rng(3)
    path = str(tmp_path / "tiny.fa")
    with open(path, "w") as f:
        for i in range(40):
            f.write(f">{i}\n{''.join('ACGT'[c] for c in rng.integers(0, 4, int(rng.integers(15, 300))))}\n")
    d = sshash_amd.Dictionary.build(path, k=15, m=7)
    q = tmp_path / "q.txt"
    q.write_text("ACGT\n")
    values = np.full(d.num_kmers(), 3, dtype=np.uint32)
    seen = []
    assert d.streaming_sums_from_file(str(q), values, per_read=lambda first, rows: seen.append(first)) == B.StreamingQueryReport()
    assert seen == []
    got, report = d.streaming_sums_from_file(str(q), values, at_least=2, multiline=True)
    assert got.dtype == sshash_amd.READ_SUM_DTYPE and got.shape == (0,) and report == B.StreamingQueryReport()
    rep = B._Report(1, 2, 3, 4, 5, 6)
    fn = B._PerReadFn(lambda ctx, first, n, rows: seen.append(first) or 0)
    assert B._load().sshash_streaming_sums_from_file(d._h, os.fsencode(str(q)), 0, values.ctypes.data, 0, fn, None, C.byref(rep)) == 0
    assert d._report(rep) == B.StreamingQueryReport() and seen == []
    assert B._load().sshash_streaming_sums_from_file(d._h, os.fsencode(str(q)), 0, values.ctypes.data, 0, fn, None, None) == 0
    with pytest.raises(sshash_amd.SSHashError) as e:  # (a file that cannot be opened: said before any device is asked for, too)
        d.streaming_sums_from_file(str(tmp_path / "missing.fa"), values, per_read=lambda first, rows: seen.append(first))
    assert e.value.status == 2 and seen == []


def test_values_none_wants_a_weighted_dictionary(case_skew_regular):
    """values=None stands for the dictionary's weights: a dictionary that stores none raises before anything else happens"""
    d = case_skew_regular.dict
    assert not d.weighted()
    with pytest.raises(ValueError):
        d.streaming_sums(["ACGT"])
    with pytest.raises(ValueError):
        d.streaming_sums_from_file(FASTQ)
