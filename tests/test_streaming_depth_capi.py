"""The streaming depth (HOW OFTEN a read set holds each k-mer of the dictionary: num_kmers words of uint32) at the C ABI and in the
binding, as far as a machine without a GPU can tell: the symbols are declared, exported, bound and present in the facade; argument
errors are reported before anything else and write nothing; num_reads == 0 is no work; a dictionary that is not resident fails with
SSHASH_ERR_NO_DEVICE; the segmented sum sshash_depth_string_sums, which is CPU code, against numpy.add.reduceat with values that a
32-bit accumulator could not hold; write_weighted_fasta -> weighted build -> weight(i) == depth[i] for every id."""
from __future__ import annotations

import ctypes as C
import os
import re

import numpy as np
import pytest

import sshash_amd
from sshash_amd import _binding as B
from conftest import FASTQ, ROOT

SYMBOLS = ("sshash_streaming_depth", "sshash_streaming_depth_device", "sshash_depth_finish_device", "sshash_streaming_depth_from_file",
           "sshash_depth_string_sums", "sshash_depth_string_sums_device")
METHODS = ("streaming_depth", "streaming_depth_device", "depth_finish_device", "streaming_depth_from_file", "depth_string_sums",
           "depth_string_sums_device")
ERR_ARGUMENT, ERR_NO_DEVICE = 1, 5
CASES = ["case_skew_regular", "case_k63_canonical", "case_small_k", "case_se_regular"]


def _batch(reads):
    chunks = [r.encode() for r in reads]
    offsets = np.zeros(len(chunks) + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum([len(c) for c in chunks], dtype=np.uint64)
    return np.frombuffer(b"".join(chunks) or b"\0", dtype=np.uint8), offsets


def _string_id_ranges(d):
    """[first id, one past the last id) of every string, out of sshash_string_offsets"""
    sids = np.arange(d.num_strings(), dtype=np.uint64)
    begin, end = d.string_offsets(sids)
    k1 = np.uint64(d.k() - 1)
    return begin - sids * k1, end - (sids + np.uint64(1)) * k1


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
    assert callable(sshash_amd.write_weighted_fasta)
    # what the header has to say: the arithmetic wraps and does not saturate, in place is allowed, where the scan's scratch comes from
    section = header[header.index("HOW OFTEN"):header.index("sshash_depth_string_sums(")]
    assert "modulo 2^32" in section and "WRAPS" in section and "saturates" in section
    assert "depth == deltas" in section and "memory pool" in section


def test_argument_errors_come_first(case_skew_regular):
    """a null dictionary, or null bases / read_offsets / output with num_reads > 0: SSHASH_ERR_ARGUMENT whether or not a device is there,
    and nothing is written"""
    d = case_skew_regular.dict
    lib = B._load()
    bases, offsets = _batch([case_skew_regular.sequences[0], "ACGT"])
    depth = np.full(d.num_kmers() + 1, 0x55, dtype=np.uint32)
    sums = np.full(d.num_strings(), 7, dtype=np.uint64)
    total = C.c_uint64(9)
    rep = B._Report(1, 2, 3, 4, 5, 6)
    b, o, c = bases.ctypes.data, offsets.ctypes.data, depth.ctypes.data
    host, device, from_file, finish = (lib.sshash_streaming_depth, lib.sshash_streaming_depth_device, lib.sshash_streaming_depth_from_file,
                                       lib.sshash_depth_finish_device)
    assert host(None, b, o, 2, c, C.byref(rep)) == ERR_ARGUMENT
    assert rep.num_kmers == 1  # (a null dictionary: not even the report is touched)
    assert host(d._h, None, o, 2, c, None) == ERR_ARGUMENT
    assert host(d._h, b, None, 2, c, None) == ERR_ARGUMENT
    assert host(d._h, b, o, 2, None, None) == ERR_ARGUMENT
    assert lib.sshash_last_error()
    # (host pointers stand in for device pointers: the call must refuse before it touches them)
    assert device(None, 0, b, o, 2, 0, c, None, None) == ERR_ARGUMENT
    assert device(d._h, 0, None, o, 2, 0, c, None, None) == ERR_ARGUMENT
    assert device(d._h, 0, b, None, 2, 0, c, None, None) == ERR_ARGUMENT
    assert device(d._h, 0, b, o, 2, 0, None, None, None) == ERR_ARGUMENT
    assert finish(None, 0, c, c, None) == ERR_ARGUMENT
    assert finish(d._h, 0, None, c, None) == ERR_ARGUMENT
    assert finish(d._h, 0, c, None, None) == ERR_ARGUMENT
    assert from_file(None, os.fsencode(FASTQ), 0, c, None) == ERR_ARGUMENT
    assert from_file(d._h, None, 0, c, None) == ERR_ARGUMENT
    assert from_file(d._h, os.fsencode(FASTQ), 0, None, None) == ERR_ARGUMENT
    assert lib.sshash_depth_string_sums(None, c, sums.ctypes.data, C.byref(total)) == ERR_ARGUMENT
    assert lib.sshash_depth_string_sums(d._h, None, sums.ctypes.data, C.byref(total)) == ERR_ARGUMENT
    assert lib.sshash_depth_string_sums(d._h, c, None, C.byref(total)) == ERR_ARGUMENT
    assert lib.sshash_depth_string_sums_device(None, 0, c, sums.ctypes.data, None, None) == ERR_ARGUMENT
    assert lib.sshash_depth_string_sums_device(d._h, 0, None, sums.ctypes.data, None, None) == ERR_ARGUMENT
    assert lib.sshash_depth_string_sums_device(d._h, 0, c, None, None, None) == ERR_ARGUMENT
    assert (depth == 0x55).all() and (sums == 7).all() and total.value == 9
    with pytest.raises(ValueError):
        d.streaming_depth(["ACGT"], depth=np.zeros(d.num_kmers() + 1, dtype=np.uint32))
    with pytest.raises(ValueError):
        d.streaming_depth(["ACGT"], depth=np.zeros(d.num_kmers(), dtype=np.uint64))
    with pytest.raises(ValueError):
        d.depth_string_sums(np.zeros(d.num_kmers(), dtype=np.int32))


def test_no_reads_is_no_work_for_the_host_call(case_skew_regular):
    """num_reads == 0 succeeds without a device and touches nothing but the report, which it zeroes"""
    d = case_skew_regular.dict
    lib = B._load()
    depth = np.full(d.num_kmers(), 0x33, dtype=np.uint32)
    rep = B._Report(1, 2, 3, 4, 5, 6)
    assert lib.sshash_streaming_depth(d._h, None, None, 0, depth.ctypes.data, C.byref(rep)) == 0
    assert (depth == 0x33).all() and rep.num_kmers == 0 and rep.num_searches == 0
    assert lib.sshash_streaming_depth(d._h, None, None, 0, None, None) == 0
    got, report = d.streaming_depth([])
    assert got.dtype == np.uint32 and got.shape == (d.num_kmers(),) and not got.any() and report == B.StreamingQueryReport()


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
    depth = np.full(d.num_kmers(), 0x11, dtype=np.uint32)
    with pytest.raises(sshash_amd.SSHashError) as e:
        d.streaming_depth(reads, depth=depth)
    assert e.value.status == ERR_NO_DEVICE
    with pytest.raises(sshash_amd.SSHashError) as e:
        d.streaming_depth_from_file(FASTQ, depth=depth)
    assert e.value.status == ERR_NO_DEVICE
    bases, offsets = _batch(reads)
    c = depth.ctypes.data
    assert lib.sshash_streaming_depth_device(d._h, 0, bases.ctypes.data, offsets.ctypes.data, 2, int(offsets[-1]), c, None, None) == ERR_NO_DEVICE
    assert lib.sshash_streaming_depth_device(d._h, 0, None, None, 0, 0, None, None, None) == ERR_NO_DEVICE
    assert lib.sshash_depth_finish_device(d._h, 0, c, c, None) == ERR_NO_DEVICE
    sums = np.full(d.num_strings(), 7, dtype=np.uint64)
    assert lib.sshash_depth_string_sums_device(d._h, 0, c, sums.ctypes.data, None, None) == ERR_NO_DEVICE
    with pytest.raises(sshash_amd.SSHashError) as e:
        d.streaming_depth_device(0, bases.ctypes.data, offsets.ctypes.data, 2, c)
    assert e.value.status == ERR_NO_DEVICE
    assert (depth == 0x11).all() and (sums == 7).all()
    got, total = d.depth_string_sums(depth)  # the host twin needs no device
    assert total == 0x11 * d.num_kmers() == int(got.sum())


def test_an_unsupported_extension_is_an_empty_report_without_any_device(tmp_path):
    """a query file whose extension says nothing: the call says "unsupported query file format" and returns before any device is asked for -- this dictionary is resident
    nowhere, and the call succeeds --, the report all zeros, a supplied depth array untouched"""
    rng = np.random.default_rng(3)
    path = str(tmp_path / "tiny.fa")
    with open(path, "w") as f:
        for i in range(40):
            f.write(f">{i}\n{''.join('ACGT'[c] for c in rng.integers(0, 4, int(rng.integers(15, 300))))}\n")
    d = sshash_amd.Dictionary.build(path, k=15, m=7)
    q = tmp_path / "q.txt"
    q.write_text("ACGT\n")
    depth = np.full(d.num_kmers(), 0x11, dtype=np.uint32)
    got, report = d.streaming_depth_from_file(str(q), depth=depth)
    assert got is depth and (depth == 0x11).all() and report == B.StreamingQueryReport()
    got, report = d.streaming_depth_from_file(str(q), multiline=True)
    assert got.shape == (d.num_kmers(),) and not got.any() and report == B.StreamingQueryReport()
    rep = B._Report(1, 2, 3, 4, 5, 6)
    assert B._load().sshash_streaming_depth_from_file(d._h, os.fsencode(str(q)), 0, depth.ctypes.data, C.byref(rep)) == 0
    assert d._report(rep) == B.StreamingQueryReport() and (depth == 0x11).all()
    assert B._load().sshash_streaming_depth_from_file(d._h, os.fsencode(str(q)), 0, depth.ctypes.data, None) == 0
    with pytest.raises(sshash_amd.SSHashError) as e:  # (a file that cannot be opened: said before any device is asked for, too)
        d.streaming_depth_from_file(str(tmp_path / "missing.fa"), depth=depth)
    assert e.value.status == 2 and (depth == 0x11).all()


@pytest.mark.parametrize("case_name", CASES)
def test_string_sums_against_numpy(case_name, request):
    """zeros, ones (the strings' sizes), random words over the whole 32-bit range -- most strings' sums pass 2^32 --, the overwrite rule"""
    case = request.getfixturevalue(case_name)
    d = case.dict
    n = d.num_kmers()
    sizes = d.string_size(np.arange(d.num_strings(), dtype=np.uint64))
    first, last = _string_id_ranges(d)
    assert first[0] == 0 and last[-1] == n and (first[1:] == last[:-1]).all() and (last - first == sizes).all()

    sums, total = d.depth_string_sums(np.zeros(n, dtype=np.uint32))
    assert sums.dtype == np.uint64 and sums.shape == (d.num_strings(),) and not sums.any() and total == 0
    sums, total = d.depth_string_sums(np.ones(n, dtype=np.uint32))
    assert (sums == sizes).all() and total == n

    rng = np.random.default_rng(11)
    depth = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    depth[rng.random(n) < 0.3] = 0
    depth[rng.random(n) < 0.2] = np.uint32(0xFFFFFFFF)
    depth[[0, n - 1]] = np.uint32(0xFFFFFFFE)
    want = np.add.reduceat(depth.astype(np.uint64), first.astype(np.int64))
    assert (want >> np.uint64(32)).any(), "a 32-bit accumulator must not be enough"
    sums, total = d.depth_string_sums(depth)
    assert (sums == want).all(), np.flatnonzero(sums != want)[:10]
    assert total == int(want.sum()) == int(depth.astype(np.uint64).sum()) and total > (1 << 32)

    # the overwrite rule, through the C ABI: sums and total hold something else before
    only = np.zeros(n, dtype=np.uint32)
    only[int(first[1]):int(last[1])] = 0xFFFFFFFF
    raw = np.full(d.num_strings(), 77, dtype=np.uint64)
    total = C.c_uint64(123)
    assert B._load().sshash_depth_string_sums(d._h, only.ctypes.data, raw.ctypes.data, C.byref(total)) == 0
    assert raw[1] == int(sizes[1]) * 0xFFFFFFFF and int(raw.sum()) == int(raw[1]) and total.value == int(raw[1])
    assert B._load().sshash_depth_string_sums(d._h, only.ctypes.data, raw.ctypes.data, None) == 0  # total may be NULL


@pytest.mark.parametrize("case_name", ["case_skew_regular", "case_k63_canonical"])
def test_weighted_fasta_closes_the_loop(case_name, request, tmp_path):
    """depths -> write_weighted_fasta -> Dictionary.build(weighted=True): the same ids, and weight(i) == depth[i] for every id. The depth
    array holds zeros, ones, a long constant stretch and values above 2^16."""
    case = request.getfixturevalue(case_name)
    d = case.dict
    n = d.num_kmers()
    rng = np.random.default_rng(17)
    depth = rng.integers(0, 4, n).astype(np.uint32)  # zeros, ones, short stretches
    depth[n // 3:n // 3 + n // 4] = 7                 # a long constant stretch, over many strings
    high = rng.integers(0, n, 50)
    depth[high] = rng.integers(1 << 16, 1 << 32, 50, dtype=np.uint64).astype(np.uint32)
    depth[-1] = 0xFFFFFFFF
    assert (depth == 0).any() and (depth == 1).any() and (depth > (1 << 16)).any()
    path = str(tmp_path / "weighted.fa")
    sshash_amd.write_weighted_fasta(d, depth, path)
    lines = open(path).read().split("\n")
    assert len(lines) == 2 * d.num_strings() + 1 and lines[-1] == ""
    sizes = d.string_size(np.arange(d.num_strings(), dtype=np.uint64))
    for s in (0, d.num_strings() - 1):
        header, text = lines[2 * s], lines[2 * s + 1]
        assert header.startswith(f">{s} LN:i:{len(text)} ab:Z:") and len(text) == int(sizes[s]) + d.k() - 1
        assert len(header.split("ab:Z:")[1].split(" ")) == int(sizes[s])
    w = sshash_amd.Dictionary.build(path, k=d.k(), m=d.m(), canonical=d.canonical(), weighted=True)
    assert w.weighted() and w.num_kmers() == n and w.num_strings() == d.num_strings()
    ids = np.arange(n, dtype=np.uint64)
    assert (w.weight(ids) == depth.astype(np.uint64)).all()
    probe = np.concatenate([ids[:500], ids[-500:], rng.integers(0, n, 2000).astype(np.uint64)])
    assert (w.access_packed(probe) == d.access_packed(probe)).all(), "the rebuilt dictionary numbers its k-mers as the first"
    with pytest.raises(ValueError):
        sshash_amd.write_weighted_fasta(d, depth[:-1], path)
