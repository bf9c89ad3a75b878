"""The per-read streaming query at the C ABI and in the binding, as far as a machine without a GPU can tell: the three symbols
are declared, exported and bound; argument errors are reported before anything else; without a device the calls fail loudly; the
existing streaming_query_from_file(filename) call is what it was."""
from __future__ import annotations

import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import sshash_amd
from sshash_amd import _binding as B
from conftest import ROOT, has_gpu

SYMBOLS = ("sshash_streaming_query_per_read", "sshash_streaming_query_per_read_device", "sshash_streaming_query_from_file_per_read")
ERR_ARGUMENT, ERR_NO_DEVICE = 1, 5


def _batch(reads):
    chunks = [r.encode() for r in reads]
    offsets = np.zeros(len(chunks) + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum([len(c) for c in chunks], dtype=np.uint64)
    return np.frombuffer(b"".join(chunks) or b"\0", dtype=np.uint8), offsets


def test_symbols_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "sshash_amd.h")).read()
    lib = C.CDLL(sshash_amd.library_path())
    bound = B._load()
    for name in SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert hasattr(lib, name), name
        assert name in B.C_ABI_SYMBOLS
        assert getattr(bound, name).argtypes is not None and getattr(bound, name).restype is C.c_int
    assert "sshash_per_read_fn" in header
    for method in ("streaming_query_per_read", "streaming_query_per_read_device"):
        assert callable(getattr(sshash_amd.Dictionary, method))
    facade = open(os.path.join(ROOT, "include", "sshash_amd.hpp")).read()
    for name in SYMBOLS:
        assert name + "(" in facade, name


def test_a_row_is_the_report_struct():
    assert C.sizeof(B._Report) == 48
    assert [f[0] for f in B._Report._fields_] == ["num_kmers", "num_positive_kmers", "num_negative_kmers", "num_invalid_kmers",
                                                  "num_searches", "num_extensions"]


def test_argument_errors_come_first(case_skew_regular, tmp_path):
    """null dictionary, null reads, per_read == NULL with num_reads > 0, fn == NULL: SSHASH_ERR_ARGUMENT whether or not a device is
    there -- they are looked at before the device is."""
    d = case_skew_regular.dict
    lib = B._load()
    bases, offsets = _batch([case_skew_regular.sequences[0], "ACGT"])
    rows = np.zeros((2, 6), dtype=np.uint64)
    rep = B._Report()
    host, device, from_file = (getattr(lib, s) for s in SYMBOLS)
    assert host(None, bases.ctypes.data, offsets.ctypes.data, 2, rows.ctypes.data, C.byref(rep)) == ERR_ARGUMENT
    assert host(d._h, bases.ctypes.data, offsets.ctypes.data, 2, None, C.byref(rep)) == ERR_ARGUMENT
    assert host(d._h, None, offsets.ctypes.data, 2, rows.ctypes.data, C.byref(rep)) == ERR_ARGUMENT
    assert host(d._h, bases.ctypes.data, None, 2, rows.ctypes.data, None) == ERR_ARGUMENT
    assert lib.sshash_last_error()
    # (host pointers stand in for device pointers: the call must refuse before it touches them)
    assert device(None, 0, bases.ctypes.data, offsets.ctypes.data, 2, 0, rows.ctypes.data, None, None) == ERR_ARGUMENT
    assert device(d._h, 0, bases.ctypes.data, offsets.ctypes.data, 2, 0, None, None, None) == ERR_ARGUMENT
    assert device(d._h, 0, None, offsets.ctypes.data, 2, 0, rows.ctypes.data, None, None) == ERR_ARGUMENT
    fq = tmp_path / "q.fastq"
    fq.write_text("@r\n" + case_skew_regular.sequences[0] + "\n+\n\n")
    called = []
    fn = B._PerReadFn(lambda ctx, first, n, rows_: called.append(first) or 0)
    null_fn = C.cast(None, B._PerReadFn)
    assert from_file(d._h, os.fsencode(str(fq)), 0, null_fn, None, C.byref(rep)) == ERR_ARGUMENT
    assert from_file(None, os.fsencode(str(fq)), 0, fn, None, C.byref(rep)) == ERR_ARGUMENT
    assert from_file(d._h, None, 0, fn, None, C.byref(rep)) == ERR_ARGUMENT
    totals = lib.sshash_streaming_query_from_file  # (the total alone: its report is no option)
    assert totals(None, os.fsencode(str(fq)), 0, C.byref(rep)) == ERR_ARGUMENT
    assert totals(d._h, None, 0, C.byref(rep)) == ERR_ARGUMENT
    assert totals(d._h, os.fsencode(str(fq)), 0, None) == ERR_ARGUMENT
    assert called == []
    assert (rows == 0).all()


def test_no_reads_is_no_work_for_the_host_call(case_skew_regular):
    """num_reads == 0 writes nothing and succeeds (as sshash_streaming_query does), per_read may then be NULL"""
    d = case_skew_regular.dict
    rep = B._Report(1, 2, 3, 4, 5, 6)
    assert B._load().sshash_streaming_query_per_read(d._h, None, None, 0, None, C.byref(rep)) == 0
    assert rep.num_kmers == 0 and rep.num_extensions == 0
    rows, report = d.streaming_query_per_read([])
    assert rows.shape == (0, 6) and rows.dtype == np.uint64 and report == B.StreamingQueryReport()


@pytest.mark.skipif(has_gpu(), reason="checks the no-GPU failure mode")
def test_without_a_device_the_calls_fail_loudly(case_skew_regular, tmp_path):
    d = case_skew_regular.dict
    lib = B._load()
    reads = [case_skew_regular.sequences[0], "ACGT"]
    with pytest.raises(sshash_amd.SSHashError) as e:
        d.streaming_query_per_read(reads)
    assert e.value.status == ERR_NO_DEVICE
    bases, offsets = _batch(reads)
    rows = np.full((2, 6), 7, dtype=np.uint64)
    assert lib.sshash_streaming_query_per_read_device(d._h, 0, bases.ctypes.data, offsets.ctypes.data, 2, int(offsets[-1]), rows.ctypes.data,
                                                      None, None) == ERR_NO_DEVICE
    assert (rows == 7).all()
    with pytest.raises(sshash_amd.SSHashError) as e:
        d.streaming_query_per_read_device(0, bases.ctypes.data, offsets.ctypes.data, 2, rows.ctypes.data)
    assert e.value.status == ERR_NO_DEVICE
    fq = tmp_path / "q.fastq"
    fq.write_text("@r\n" + reads[0] + "\n+\n\n")
    seen = []
    with pytest.raises(sshash_amd.SSHashError) as e:
        d.streaming_query_from_file(str(fq), per_read=lambda first, block: seen.append(first))
    assert e.value.status == ERR_NO_DEVICE and seen == []
    with pytest.raises(sshash_amd.SSHashError) as e:
        d.streaming_query_from_file(str(fq))
    assert e.value.status == ERR_NO_DEVICE


def test_the_file_query_keeps_its_signature(case_skew_regular, tmp_path):
    """streaming_query_from_file(filename) and (filename, multiline) as before; per_read is a keyword that defaults to None, and
    without it the call is the C ABI's sshash_streaming_query_from_file -- an unsupported extension still gives an empty report
    without any device."""
    sig = inspect.signature(sshash_amd.Dictionary.streaming_query_from_file)
    assert list(sig.parameters) == ["self", "filename", "multiline", "per_read"]
    assert sig.parameters["multiline"].default is False and sig.parameters["per_read"].default is None
    d = case_skew_regular.dict
    q = tmp_path / "q.txt"
    q.write_text("ACGT\n")
    assert d.streaming_query_from_file(str(q)) == B.StreamingQueryReport()
    assert d.streaming_query_from_file(str(q), True) == B.StreamingQueryReport()
    seen = []
    assert d.streaming_query_from_file(str(q), per_read=lambda first, block: seen.append(first)) == B.StreamingQueryReport()
    assert seen == []
    with pytest.raises(sshash_amd.SSHashError) as e:
        d.streaming_query_from_file(str(tmp_path / "missing.fq"), per_read=lambda first, block: None)
    assert e.value.status == 2
