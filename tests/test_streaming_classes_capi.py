"""The streaming classes (per read, its positive k-mers by class of string) at the C ABI and in the binding, as far as a machine without a
GPU can tell: the symbols are declared, exported, bound and present in the facade; a finished row is 16 bytes; argument errors --
null pointers, num_classes of 0 or above the cap -- are reported before anything else and write nothing; num_reads == 0 is no work; a
dictionary that is not resident fails with SSHASH_ERR_NO_DEVICE; and the host variants of the two finish calls against numpy on rows
made by hand: a tie, a single column, a row of zeros, one class, a count of 0xFFFFFFFF, column sums above 2^32."""
from __future__ import annotations

import ctypes as C
import os
import re

import numpy as np
import pytest

import sshash_amd
from sshash_amd import _binding as B
from conftest import FASTQ, ROOT

SYMBOLS = ("sshash_streaming_classes", "sshash_streaming_classes_device", "sshash_streaming_classes_from_file", "sshash_class_best",
           "sshash_class_best_device", "sshash_class_totals", "sshash_class_totals_device")
METHODS = ("streaming_classes", "streaming_classes_device", "streaming_classes_from_file", "class_best_device", "class_totals_device")
ERR_ARGUMENT, ERR_NO_DEVICE = 1, 5
CAP = 4096
NONE = 0xFFFFFFFF


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
    assert callable(sshash_amd.class_best) and callable(sshash_amd.class_totals)
    assert re.search(r"#define\s+SSHASH_MAX_CLASSES\s+4096u", header) and sshash_amd.MAX_CLASSES == CAP
    assert re.search(r"#define\s+SSHASH_NO_CLASS\s+0xFFFFFFFFu", header) and sshash_amd.NO_CLASS == NONE
    # what the header has to say: semantics, alignment, the mask, modulo arithmetic, the cap on a piece, which calls segment, what a shard returns
    section = header[header.index("CLASSES: per read"):header.index("sshash_streaming_classes_from_file(")]
    for words in ("modulo 2^32", "4-byte", "no class", "OVERWRITTEN", "minimizer shard", "sshash_set_read_segments", "64 MiB", "nothing outside"):
        assert words in section, words


def test_a_finished_row_is_sixteen_bytes():
    """sizeof(sshash_read_class) == 16: the header's struct, the dtype and the static_assert of the library's own source agree"""
    header = open(os.path.join(ROOT, "include", "sshash_amd.h")).read()
    body = re.search(r"typedef struct sshash_read_class \{(.*?)\} sshash_read_class;", header, re.S).group(1)
    names = ("best_class", "best", "second", "total")
    assert tuple(re.findall(r"uint32_t\s+(\w+);", body)) == names
    assert sshash_amd.READ_CLASS_DTYPE.itemsize == 16 and sshash_amd.READ_CLASS_DTYPE.names == names
    assert [sshash_amd.READ_CLASS_DTYPE.fields[n][1] for n in names] == [0, 4, 8, 12]
    capi = open(os.path.join(ROOT, "sshash_amd", "csrc", "capi.cpp")).read()
    assert "static_assert(sizeof(sshash_read_class) == 4 * sizeof(uint32_t)" in capi


def test_argument_errors_come_first(case_skew_regular):
    """a null dictionary, null bases / read_offsets / labels / rows with num_reads > 0, num_classes of 0 or above the cap:
    SSHASH_ERR_ARGUMENT whether or not a device is there -- this dictionary is not resident --, and nothing is written"""
    d = case_skew_regular.dict
    lib = B._load()
    bases, offsets = _batch([case_skew_regular.sequences[0], "ACGT"])
    labels = np.full(d.num_strings(), 2, dtype=np.uint32)
    rows = np.full((2, 3), 0x77, dtype=np.uint32)
    rep = B._Report(1, 2, 3, 4, 5, 6)
    b, o, l, r = bases.ctypes.data, offsets.ctypes.data, labels.ctypes.data, rows.ctypes.data
    fn = B._PerReadFn(lambda *a: 0)
    host, device, from_file = lib.sshash_streaming_classes, lib.sshash_streaming_classes_device, lib.sshash_streaming_classes_from_file
    assert host(None, b, o, 2, l, 3, r, C.byref(rep)) == ERR_ARGUMENT
    assert rep.num_kmers == 1  # (a null dictionary: not even the report is touched)
    assert host(d._h, None, o, 2, l, 3, r, None) == ERR_ARGUMENT
    assert host(d._h, b, None, 2, l, 3, r, None) == ERR_ARGUMENT
    assert host(d._h, b, o, 2, None, 3, r, None) == ERR_ARGUMENT
    assert host(d._h, b, o, 2, l, 3, None, None) == ERR_ARGUMENT
    assert host(d._h, b, o, 2, l, 0, r, C.byref(rep)) == ERR_ARGUMENT
    assert host(d._h, b, o, 2, l, CAP + 1, r, C.byref(rep)) == ERR_ARGUMENT
    assert rep.num_kmers == 1 and lib.sshash_last_error()
    # (host pointers stand in for device pointers: the call must refuse before it touches them)
    assert device(None, 0, b, o, 2, 0, l, 3, r, None, None) == ERR_ARGUMENT
    assert device(d._h, 0, None, o, 2, 0, l, 3, r, None, None) == ERR_ARGUMENT
    assert device(d._h, 0, b, None, 2, 0, l, 3, r, None, None) == ERR_ARGUMENT
    assert device(d._h, 0, b, o, 2, 0, None, 3, r, None, None) == ERR_ARGUMENT
    assert device(d._h, 0, b, o, 2, 0, l, 3, None, None, None) == ERR_ARGUMENT
    assert device(d._h, 0, b, o, 2, 0, l, 0, r, None, None) == ERR_ARGUMENT
    assert device(d._h, 0, b, o, 2, 0, l, CAP + 1, r, None, None) == ERR_ARGUMENT
    assert from_file(None, os.fsencode(FASTQ), 0, l, 3, fn, None, None) == ERR_ARGUMENT
    assert from_file(d._h, None, 0, l, 3, fn, None, None) == ERR_ARGUMENT
    assert from_file(d._h, os.fsencode(FASTQ), 0, None, 3, fn, None, None) == ERR_ARGUMENT
    assert from_file(d._h, os.fsencode(FASTQ), 0, l, 3, B._PerReadFn(), None, None) == ERR_ARGUMENT
    assert from_file(d._h, os.fsencode(FASTQ), 0, l, 0, fn, None, None) == ERR_ARGUMENT
    assert from_file(d._h, os.fsencode(FASTQ), 0, l, CAP + 1, fn, None, None) == ERR_ARGUMENT
    best = np.full(2, 0x33, dtype=sshash_amd.READ_CLASS_DTYPE)
    totals = np.full(3, 0x33, dtype=np.uint64)
    for finish, out in ((lib.sshash_class_best_device, best), (lib.sshash_class_totals_device, totals)):
        assert finish(None, 0, r, 2, 3, out.ctypes.data, None) == ERR_ARGUMENT
        assert finish(d._h, 0, None, 2, 3, out.ctypes.data, None) == ERR_ARGUMENT
        assert finish(d._h, 0, r, 2, 3, None, None) == ERR_ARGUMENT
        assert finish(d._h, 0, r, 2, 0, out.ctypes.data, None) == ERR_ARGUMENT
        assert finish(d._h, 0, r, 2, CAP + 1, out.ctypes.data, None) == ERR_ARGUMENT
    for finish, out in ((lib.sshash_class_best, best), (lib.sshash_class_totals, totals)):
        assert finish(None, 2, 3, out.ctypes.data) == ERR_ARGUMENT
        assert finish(r, 2, 3, None) == ERR_ARGUMENT
        assert finish(r, 2, 0, out.ctypes.data) == ERR_ARGUMENT
        assert finish(r, 2, CAP + 1, out.ctypes.data) == ERR_ARGUMENT
    assert (rows == 0x77).all() and (labels == 2).all() and (best.view(np.uint32) == 0x33).all() and (totals == 0x33).all()
    with pytest.raises(ValueError):
        d.streaming_classes(["ACGT"], np.zeros(d.num_strings() + 1, dtype=np.uint32), 3)
    with pytest.raises(ValueError):
        d.streaming_classes(["ACGT"], np.zeros(d.num_strings(), dtype=np.float64), 3)
    with pytest.raises(ValueError):
        d.streaming_classes(["ACGT"], np.full(d.num_strings(), 1 << 32, dtype=np.uint64), 3)
    for bad in (0, CAP + 1):
        with pytest.raises(ValueError):
            d.streaming_classes(["ACGT"], labels, bad)
        with pytest.raises(ValueError):
            d.streaming_classes_from_file(FASTQ, labels, bad)
    with pytest.raises(ValueError):
        sshash_amd.class_best(np.zeros((2, CAP + 1), dtype=np.uint32))
    with pytest.raises(ValueError):
        sshash_amd.class_totals(np.zeros(5, dtype=np.uint32))


def test_no_reads_is_no_work_for_the_host_call(case_skew_regular):
    """num_reads == 0 succeeds without a device and touches nothing but the report, which it zeroes"""
    d = case_skew_regular.dict
    lib = B._load()
    labels = np.full(d.num_strings(), 2, dtype=np.uint32)
    rows = np.full((2, 3), 0x33, dtype=np.uint32)
    rep = B._Report(1, 2, 3, 4, 5, 6)
    assert lib.sshash_streaming_classes(d._h, None, None, 0, labels.ctypes.data, 3, rows.ctypes.data, C.byref(rep)) == 0
    assert (rows == 0x33).all() and rep.num_kmers == 0 and rep.num_searches == 0
    assert lib.sshash_streaming_classes(d._h, None, None, 0, None, 3, None, None) == 0
    got, report = d.streaming_classes([], labels, 3)
    assert got.dtype == np.uint32 and got.shape == (0, 3) and report == B.StreamingQueryReport()
    best = sshash_amd.class_best(np.zeros((0, 3), dtype=np.uint32))
    assert best.dtype == sshash_amd.READ_CLASS_DTYPE and best.shape == (0,)
    assert (sshash_amd.class_totals(np.zeros((0, 3), dtype=np.uint32)) == 0).all()  # (no reads: the totals are still overwritten)


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
    labels = (np.arange(d.num_strings()) % 3).astype(np.uint32)
    with pytest.raises(sshash_amd.SSHashError) as e:
        d.streaming_classes(reads, labels, 3)
    assert e.value.status == ERR_NO_DEVICE
    with pytest.raises(sshash_amd.SSHashError) as e:
        d.streaming_classes_from_file(path, labels, 3)
    assert e.value.status == ERR_NO_DEVICE
    bases, offsets = _batch(reads)
    rows = np.full((2, 3), 0x77, dtype=np.uint32)
    rep = np.full(6, 9, dtype=np.uint64)
    best = np.full(2, 0x33, dtype=sshash_amd.READ_CLASS_DTYPE)
    totals = np.full(3, 0x33, dtype=np.uint64)
    assert lib.sshash_streaming_classes_device(d._h, 0, bases.ctypes.data, offsets.ctypes.data, 2, 0, labels.ctypes.data, 3, rows.ctypes.data,
                                               rep.ctypes.data, None) == ERR_NO_DEVICE
    assert lib.sshash_class_best_device(d._h, 0, rows.ctypes.data, 2, 3, best.ctypes.data, None) == ERR_NO_DEVICE
    assert lib.sshash_class_totals_device(d._h, 0, rows.ctypes.data, 2, 3, totals.ctypes.data, None) == ERR_NO_DEVICE
    assert (rows == 0x77).all() and (rep == 9).all() and (best.view(np.uint32) == 0x33).all() and (totals == 0x33).all()


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
    labels = (np.arange(d.num_strings()) % 3).astype(np.uint32)
    seen = []
    assert d.streaming_classes_from_file(str(q), labels, 3, per_read=lambda first, rows: seen.append(first)) == B.StreamingQueryReport()
    assert seen == []
    got, report = d.streaming_classes_from_file(str(q), labels, 5, multiline=True)
    assert got.dtype == np.uint32 and got.shape == (0, 5) and report == B.StreamingQueryReport()
    rep = B._Report(1, 2, 3, 4, 5, 6)
    fn = B._PerReadFn(lambda ctx, first, n, rows: seen.append(first) or 0)
    assert B._load().sshash_streaming_classes_from_file(d._h, os.fsencode(str(q)), 0, labels.ctypes.data, 3, fn, None, C.byref(rep)) == 0
    assert d._report(rep) == B.StreamingQueryReport() and seen == []
    assert B._load().sshash_streaming_classes_from_file(d._h, os.fsencode(str(q)), 0, labels.ctypes.data, 3, fn, None, None) == 0
    with pytest.raises(sshash_amd.SSHashError) as e:  # (a file that cannot be opened: said before any device is asked for, too)
        d.streaming_classes_from_file(str(tmp_path / "missing.fa"), labels, 3, per_read=lambda first, rows: seen.append(first))
    assert e.value.status == 2 and seen == []
    # the order of the checks: num_classes is looked at before the report is zeroed
    rep = B._Report(1, 2, 3, 4, 5, 6)
    assert B._load().sshash_streaming_classes_from_file(d._h, os.fsencode(str(q)), 0, labels.ctypes.data, 0, fn, None, C.byref(rep)) == ERR_ARGUMENT
    assert rep.num_kmers == 1 and rep.num_extensions == 6


def _numpy_best(rows):
    n, classes = rows.shape
    out = np.zeros(n, dtype=sshash_amd.READ_CLASS_DTYPE)
    order = np.argsort(-rows.astype(np.int64), axis=1, kind="stable")  # (descending by count; among equals ascending by class)
    out["best_class"] = order[:, 0]
    out["best"] = rows[np.arange(n), order[:, 0]]
    out["second"] = rows[np.arange(n), order[:, 1]] if classes > 1 else 0
    out["total"] = (rows.sum(axis=1, dtype=np.uint64) & np.uint64(NONE)).astype(np.uint32)
    out["best_class"][out["best"] == 0] = NONE
    return out


def test_the_finish_on_the_host_against_numpy_on_rows_made_by_hand():
    rows = np.array([[3, 9, 0, 9, 1],        # a tie between classes 1 and 3: the smaller wins, second == best
                     [0, 0, 0, 6, 0],        # a single column that is not zero: second == 0
                     [0, 0, 0, 0, 0],        # zeros: no class
                     [NONE, 5, NONE, 0, 0],  # counts of 0xFFFFFFFF, tied; the total wraps
                     [NONE, 0, 0, 0, 0],
                     [1, 2, 3, 4, 5],
                     [5, 4, 3, 2, 1],
                     [2, 2, 2, 2, 2]], dtype=np.uint32)
    best = sshash_amd.class_best(rows)
    assert best.dtype == sshash_amd.READ_CLASS_DTYPE
    assert best.tolist() == [(1, 9, 9, 22), (3, 6, 0, 6), (NONE, 0, 0, 0), (0, NONE, NONE, (2 * NONE + 5) & NONE), (0, NONE, 0, NONE), (4, 5, 4, 15),
                             (0, 5, 4, 15), (0, 2, 2, 10)]
    assert best.tobytes() == _numpy_best(rows).tobytes()
    totals = sshash_amd.class_totals(rows)
    assert totals.dtype == np.uint64 and totals.tolist() == rows.sum(axis=0, dtype=np.uint64).tolist()
    assert int(totals[0]) > 1 << 32  # a column sum above 2^32
    # one class
    one = np.array([[7], [0], [NONE], [NONE]], dtype=np.uint32)
    assert sshash_amd.class_best(one).tolist() == [(0, 7, 0, 7), (NONE, 0, 0, 0), (0, NONE, 0, NONE), (0, NONE, 0, NONE)]
    assert sshash_amd.class_totals(one).tolist() == [7 + 2 * NONE]
    # random rows with few distinct counts (ties everywhere), at the widths on both sides of 64 and at the cap; garbage is overwritten
    rng = np.random.default_rng(5)
    lib = B._load()
    for classes in (1, 2, 3, 64, 65, CAP):
        rows = rng.integers(0, 3, (50, classes)).astype(np.uint32)
        rows[::5] = 0
        rows[1::5, classes - 1] = NONE
        assert sshash_amd.class_best(rows).tobytes() == _numpy_best(rows).tobytes(), classes
        out = np.full(classes + 2, 0x77, dtype=np.uint64)
        assert lib.sshash_class_totals(rows.ctypes.data, 50, classes, out[1:].ctypes.data) == 0
        assert out[0] == 0x77 and out[-1] == 0x77 and (out[1:-1] == rows.sum(axis=0, dtype=np.uint64)).all(), classes


def test_the_finish_refuses_rows_it_would_have_to_change():
    """rows are counts of 32 bits: other integer types are taken when every count fits, nothing else is cast"""
    rows = np.array([[3, 9, 0], [0, 0, 6]], dtype=np.int64)
    assert sshash_amd.class_best(rows).tolist() == [(1, 9, 3, 12), (2, 6, 0, 6)]
    assert sshash_amd.class_totals(rows.astype(np.uint16)).tolist() == [3, 9, 6]
    for bad in (rows.astype(np.float64), -rows, rows << 32, rows[0], rows.reshape(2, 3, 1), np.zeros((2, 0), dtype=np.uint32),
                np.zeros((1, CAP + 1), dtype=np.uint32)):
        for finish in (sshash_amd.class_best, sshash_amd.class_totals):
            with pytest.raises(ValueError):
                finish(bad)
