"""The streaming runs (WHERE a read hits: one record per search and the extensions behind it) at the C ABI and in the binding, as far as
a machine without a GPU can tell: the two symbols are declared, exported and bound; the record is the 32-byte struct of the header;
argument errors are reported before anything else; without a device the calls fail loudly; expand_runs is the inverse the record's
comment describes."""
from __future__ import annotations

import ctypes as C
import os
import re

import numpy as np
import pytest

import sshash_amd
from sshash_amd import _binding as B
from conftest import ROOT, has_gpu

SYMBOLS = ("sshash_streaming_runs", "sshash_streaming_runs_device")
ERR_ARGUMENT, ERR_NO_DEVICE = 1, 5
INVALID = sshash_amd.INVALID_U64


def _batch(reads):
    chunks = [r.encode() for r in reads]
    offsets = np.zeros(len(chunks) + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum([len(c) for c in chunks], dtype=np.uint64)
    return np.frombuffer(b"".join(chunks) or b"\0", dtype=np.uint8), offsets


def test_symbols_are_declared_exported_and_bound():
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
    for method in ("streaming_runs", "streaming_runs_device"):
        assert callable(getattr(sshash_amd.Dictionary, method))
        assert re.search(r"\b" + method + r"\s*\(", facade), method
    assert callable(sshash_amd.expand_runs)


def test_the_record_is_the_struct_of_the_header():
    header = open(os.path.join(ROOT, "include", "sshash_amd.h")).read()
    body = re.search(r"typedef struct sshash_streaming_run \{(.*?)\} sshash_streaming_run;", header, re.S).group(1)
    fields = re.findall(r"^\s*(uint64_t|uint32_t)\s+(\w+);", body, re.M)
    assert fields == [("uint64_t", "kmer_id"), ("uint64_t", "string_id"), ("uint64_t", "kmer_id_in_string"), ("uint32_t", "read_pos"),
                      ("uint32_t", "num_kmers")]
    assert re.search(r"#define\s+SSHASH_RUN_BACKWARD\s+0x80000000u", header)
    assert C.sizeof(B._Run) == 32 == sshash_amd.RUN_DTYPE.itemsize
    want = {"kmer_id": 0, "string_id": 8, "kmer_id_in_string": 16, "read_pos": 24, "num_kmers": 28}
    assert {name: getattr(B._Run, name).offset for name in want} == want
    assert {name: sshash_amd.RUN_DTYPE.fields[name][1] for name in want} == want
    assert [f[0] for f in B._Run._fields_] == list(sshash_amd.RUN_DTYPE.names) == [name for _, name in fields]
    assert sshash_amd.RUN_BACKWARD == 0x80000000


def test_argument_errors_come_first(case_skew_regular):
    """null dictionary / bases / read_offsets / run_offsets with num_reads > 0, runs == NULL with runs_capacity > 0:
    SSHASH_ERR_ARGUMENT whether or not a device is there, and nothing is written"""
    d = case_skew_regular.dict
    lib = B._load()
    bases, offsets = _batch([case_skew_regular.sequences[0], "ACGT"])
    ro = np.full(3, 7, dtype=np.uint64)
    runs = np.zeros(8, dtype=sshash_amd.RUN_DTYPE)
    rep = B._Report()
    host, device = (getattr(lib, s) for s in SYMBOLS)
    b, o, r, u = bases.ctypes.data, offsets.ctypes.data, ro.ctypes.data, runs.ctypes.data
    assert host(None, b, o, 2, r, u, 8, C.byref(rep)) == ERR_ARGUMENT
    assert host(d._h, None, o, 2, r, u, 8, C.byref(rep)) == ERR_ARGUMENT
    assert host(d._h, b, None, 2, r, u, 8, C.byref(rep)) == ERR_ARGUMENT
    assert host(d._h, b, o, 2, None, u, 8, C.byref(rep)) == ERR_ARGUMENT
    assert host(d._h, b, o, 2, r, None, 8, None) == ERR_ARGUMENT
    assert host(d._h, None, None, 0, r, None, 1, None) == ERR_ARGUMENT  # (no reads, but room promised at a null pointer)
    assert lib.sshash_last_error()
    # (host pointers stand in for device pointers: the call must refuse before it touches them)
    assert device(None, 0, b, o, 2, 0, r, u, 8, None, None) == ERR_ARGUMENT
    assert device(d._h, 0, None, o, 2, 0, r, u, 8, None, None) == ERR_ARGUMENT
    assert device(d._h, 0, b, None, 2, 0, r, u, 8, None, None) == ERR_ARGUMENT
    assert device(d._h, 0, b, o, 2, 0, None, u, 8, None, None) == ERR_ARGUMENT
    assert device(d._h, 0, b, o, 2, 0, r, None, 8, None, None) == ERR_ARGUMENT
    assert (ro == 7).all() and runs.tobytes() == bytes(8 * 32)


def test_the_host_call_refuses_a_read_of_2_to_31_bases(case_skew_regular):
    """read_pos and the length in num_kmers are 31 bits wide: a read of 2^31 bases or more is SSHASH_ERR_ARGUMENT, looked at before the
    device is and before a base is read (the bases here are ONE byte), run_offsets untouched; 2^31 - 1 bases get past that check"""
    d = case_skew_regular.dict
    host = B._load().sshash_streaming_runs
    bases = np.zeros(1, dtype=np.uint8)
    runs = np.zeros(2, dtype=sshash_amd.RUN_DTYPE)
    rep = B._Report()
    for lengths in ([1 << 31], [5, 1 << 31], [(1 << 31) + 1, 3], [0, 1 << 32, 0], [(1 << 31) - 1, 1 << 31]):
        offsets = np.concatenate([[0], np.cumsum(np.array(lengths, dtype=np.uint64))]).astype(np.uint64)
        ro = np.full(len(lengths) + 1, 7, dtype=np.uint64)
        for buffer, capacity in ((runs.ctypes.data, 2), (None, 0)):
            assert host(d._h, bases.ctypes.data, offsets.ctypes.data, len(lengths), ro.ctypes.data, buffer, capacity, C.byref(rep)) == ERR_ARGUMENT, lengths
        assert (ro == 7).all() and runs.tobytes() == bytes(2 * 32), lengths
    if not has_gpu():  # (with a device the call would go on to read the 2^31 - 1 bases that are not there)
        for lengths in ([(1 << 31) - 1], [4, (1 << 31) - 1]):
            offsets = np.concatenate([[0], np.cumsum(np.array(lengths, dtype=np.uint64))]).astype(np.uint64)
            ro = np.full(len(lengths) + 1, 7, dtype=np.uint64)
            assert host(d._h, bases.ctypes.data, offsets.ctypes.data, len(lengths), ro.ctypes.data, None, 0, None) == ERR_NO_DEVICE, lengths


def test_no_reads_is_no_work_for_the_host_call(case_skew_regular):
    """num_reads == 0 succeeds without a device and writes run_offsets[0] = 0 -- only if run_offsets is not NULL"""
    d = case_skew_regular.dict
    lib = B._load()
    rep = B._Report(1, 2, 3, 4, 5, 6)
    ro = np.full(1, 9, dtype=np.uint64)
    assert lib.sshash_streaming_runs(d._h, None, None, 0, ro.ctypes.data, None, 0, C.byref(rep)) == 0
    assert ro[0] == 0 and rep.num_kmers == 0 and rep.num_searches == 0
    assert lib.sshash_streaming_runs(d._h, None, None, 0, None, None, 0, None) == 0
    run_offsets, runs, report = d.streaming_runs([])
    assert run_offsets.tolist() == [0] and runs.shape == (0,) and runs.dtype == sshash_amd.RUN_DTYPE and report == B.StreamingQueryReport()


@pytest.mark.skipif(has_gpu(), reason="checks the no-GPU failure mode")
def test_without_a_device_the_calls_fail_loudly(case_skew_regular):
    d = case_skew_regular.dict
    lib = B._load()
    reads = [case_skew_regular.sequences[0], "ACGT"]
    with pytest.raises(sshash_amd.SSHashError) as e:
        d.streaming_runs(reads)
    assert e.value.status == ERR_NO_DEVICE
    bases, offsets = _batch(reads)
    ro = np.full(3, 7, dtype=np.uint64)
    runs = np.zeros(4, dtype=sshash_amd.RUN_DTYPE)
    assert lib.sshash_streaming_runs_device(d._h, 0, bases.ctypes.data, offsets.ctypes.data, 2, int(offsets[-1]), ro.ctypes.data, runs.ctypes.data, 4,
                                            None, None) == ERR_NO_DEVICE
    assert lib.sshash_streaming_runs_device(d._h, 0, None, None, 0, 0, ro.ctypes.data, None, 0, None, None) == ERR_NO_DEVICE
    assert (ro == 7).all()
    with pytest.raises(sshash_amd.SSHashError) as e:
        d.streaming_runs_device(0, bases.ctypes.data, offsets.ctypes.data, 2, ro.ctypes.data, runs.ctypes.data, 4)
    assert e.value.status == ERR_NO_DEVICE


def test_expand_runs_against_hand_written_records():
    """forward, backward, a run of one, an empty read, a read shorter than k, a last record ending at the read's last k-mer"""
    k = 5
    lengths = [12, 0, 9, 3, 5]  # 8, 0, 5, 0 and 1 k-mers
    runs = np.zeros(5, dtype=sshash_amd.RUN_DTYPE)
    runs[0] = (100, 7, 10, 1, 3)                             # read 0: k-mers 1..3 forward in string 7
    runs[1] = (50, 2, 20, 4, 4 | sshash_amd.RUN_BACKWARD)    # read 0: k-mers 4..7 backward in string 2, up to the read's last k-mer
    runs[2] = (9, 0, 9, 0, 1)                                # read 2: a run of one at the start
    runs[3] = (1000, 3, 3, 2, 3 | sshash_amd.RUN_BACKWARD)   # read 2: its last three k-mers, backward
    runs[4] = (77, 5, 0, 0, 1)                               # read 4: its only k-mer
    run_offsets = np.array([0, 2, 2, 4, 4, 5], dtype=np.uint64)
    got = sshash_amd.expand_runs(run_offsets, runs, lengths, k)
    assert [len(g.kmer_id) for g in got] == [8, 0, 5, 0, 1]
    assert got[0].kmer_id.tolist() == [INVALID, 100, 101, 102, 50, 49, 48, 47]
    assert got[0].kmer_id_in_string.tolist() == [INVALID, 10, 11, 12, 20, 19, 18, 17]
    assert got[0].string_id.tolist() == [INVALID, 7, 7, 7, 2, 2, 2, 2]
    assert got[0].kmer_orientation.tolist() == [1, 1, 1, 1, -1, -1, -1, -1]
    assert got[2].kmer_id.tolist() == [9, INVALID, 1000, 999, 998] and got[2].kmer_id_in_string.tolist() == [9, INVALID, 3, 2, 1]
    assert got[2].string_id.tolist() == [0, INVALID, 3, 3, 3] and got[2].kmer_orientation.tolist() == [1, 1, -1, -1, -1]
    assert got[4].kmer_id.tolist() == [77] and got[4].kmer_orientation.tolist() == [1]
    for g in got:
        assert g.kmer_id.dtype == np.uint64 and g.kmer_orientation.dtype == np.int8
    with pytest.raises(ValueError):  # a run that leaves its read
        sshash_amd.expand_runs(np.array([0, 1], dtype=np.uint64), runs[1:2], [10], k)
    with pytest.raises(ValueError):
        sshash_amd.expand_runs(run_offsets, runs, lengths[:-1], k)
