"""The streaming cover (WHICH k-mers of the dictionary a read set holds: a bitmap over the k-mer ids) at the C ABI and in the binding, as
far as a machine without a GPU can tell: the symbols are declared, exported, bound and present in the facade; sshash_cover_words; argument
errors are reported before anything else and write nothing; without a device the streaming calls fail loudly; the segmented popcount
sshash_cover_string_counts, which is CPU code, against numpy."""
from __future__ import annotations

import ctypes as C
import os
import re

import numpy as np
import pytest

import sshash_amd
from sshash_amd import _binding as B
from conftest import FASTQ, ROOT, has_gpu

SYMBOLS = ("sshash_cover_words", "sshash_streaming_cover", "sshash_streaming_cover_device", "sshash_streaming_cover_from_file",
           "sshash_cover_string_counts", "sshash_cover_string_counts_device")
METHODS = ("cover_words", "streaming_cover", "streaming_cover_device", "streaming_cover_from_file", "cover_string_counts",
           "cover_string_counts_device")
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


def _numpy_counts(d, cover):
    """the segmented sum in numpy: one entry per k-mer id, summed between the strings' first ids"""
    bits = np.unpackbits(cover.view(np.uint8), bitorder="little")[: d.num_kmers()].astype(np.uint64)
    first, last = _string_id_ranges(d)
    assert first[0] == 0 and last[-1] == d.num_kmers() and (first[1:] == last[:-1]).all()
    return np.add.reduceat(bits, first.astype(np.int64)), int(bits.sum())


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
    assert callable(sshash_amd.cover_to_ids) and callable(sshash_amd.ids_to_cover)
    # the bit layout and the equivalence the issue asks the header to state
    assert "i & 63" in header and "i >> 6" in header and "SSHASH_INVALID_U64" in header and "sshash_streaming_lookup" in header


@pytest.mark.parametrize("case_name", CASES)
def test_cover_words(case_name, request):
    d = request.getfixturevalue(case_name).dict
    words = C.c_uint64(0)
    assert B._load().sshash_cover_words(d._h, C.byref(words)) == 0
    assert words.value == (d.num_kmers() + 63) // 64 == d.cover_words()
    assert B._load().sshash_cover_words(None, C.byref(words)) == ERR_ARGUMENT
    assert B._load().sshash_cover_words(d._h, None) == ERR_ARGUMENT


def test_ids_and_bitmaps_are_inverse():
    ids = np.array([0, 1, 63, 64, 65, 127, 128, 700, 703], dtype=np.uint64)
    cover = sshash_amd.ids_to_cover(np.concatenate([ids, ids[:3], [sshash_amd.INVALID_U64]]).astype(np.uint64), 11)
    assert cover.dtype == np.uint64 and cover.shape == (11,)
    assert cover[0] == (1 << 0) | (1 << 1) | (1 << 63) and cover[1] == (1 << 0) | (1 << 1) | (1 << 63) and cover[2] == 1
    assert cover[10] == (1 << (700 - 640)) | (1 << 63)
    assert (sshash_amd.cover_to_ids(cover) == ids).all() and sshash_amd.cover_to_ids(cover).dtype == np.uint64
    assert sshash_amd.cover_to_ids(np.zeros(3, dtype=np.uint64)).size == 0


def test_argument_errors_come_first(case_skew_regular):
    """a null dictionary, or null bases / read_offsets / cover with num_reads > 0: SSHASH_ERR_ARGUMENT whether or not a device is there,
    and nothing is written"""
    d = case_skew_regular.dict
    lib = B._load()
    bases, offsets = _batch([case_skew_regular.sequences[0], "ACGT"])
    cover = np.full(d.cover_words() + 1, 0x55, dtype=np.uint64)
    counts = np.full(d.num_strings(), 7, dtype=np.uint64)
    total = C.c_uint64(9)
    rep = B._Report(1, 2, 3, 4, 5, 6)
    b, o, c = bases.ctypes.data, offsets.ctypes.data, cover.ctypes.data
    host, device, from_file = lib.sshash_streaming_cover, lib.sshash_streaming_cover_device, lib.sshash_streaming_cover_from_file
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
    assert from_file(None, os.fsencode(FASTQ), 0, c, None) == ERR_ARGUMENT
    assert from_file(d._h, None, 0, c, None) == ERR_ARGUMENT
    assert from_file(d._h, os.fsencode(FASTQ), 0, None, None) == ERR_ARGUMENT
    assert lib.sshash_cover_string_counts(None, c, counts.ctypes.data, C.byref(total)) == ERR_ARGUMENT
    assert lib.sshash_cover_string_counts(d._h, None, counts.ctypes.data, C.byref(total)) == ERR_ARGUMENT
    assert lib.sshash_cover_string_counts(d._h, c, None, C.byref(total)) == ERR_ARGUMENT
    assert lib.sshash_cover_string_counts_device(None, 0, c, counts.ctypes.data, None, None) == ERR_ARGUMENT
    assert lib.sshash_cover_string_counts_device(d._h, 0, None, counts.ctypes.data, None, None) == ERR_ARGUMENT
    assert lib.sshash_cover_string_counts_device(d._h, 0, c, None, None, None) == ERR_ARGUMENT
    assert (cover == 0x55).all() and (counts == 7).all() and total.value == 9
    with pytest.raises(ValueError):
        d.streaming_cover(["ACGT"], cover=np.zeros(d.cover_words() + 1, dtype=np.uint64))
    with pytest.raises(ValueError):
        d.cover_string_counts(np.zeros(d.cover_words(), dtype=np.int64))


def test_no_reads_is_no_work_for_the_host_call(case_skew_regular):
    """num_reads == 0 succeeds without a device and touches nothing but the report, which it zeroes"""
    d = case_skew_regular.dict
    lib = B._load()
    cover = np.full(d.cover_words(), 0x33, dtype=np.uint64)
    rep = B._Report(1, 2, 3, 4, 5, 6)
    assert lib.sshash_streaming_cover(d._h, None, None, 0, cover.ctypes.data, C.byref(rep)) == 0
    assert (cover == 0x33).all() and rep.num_kmers == 0 and rep.num_searches == 0
    assert lib.sshash_streaming_cover(d._h, None, None, 0, None, None) == 0
    got, report = d.streaming_cover([])
    assert got.shape == (d.cover_words(),) and not got.any() and report == B.StreamingQueryReport()


@pytest.mark.skipif(has_gpu(), reason="checks the no-GPU failure mode")
def test_without_a_device_the_streaming_calls_fail_loudly(case_skew_regular):
    d = case_skew_regular.dict
    lib = B._load()
    reads = [case_skew_regular.sequences[0], "ACGT"]
    cover = np.full(d.cover_words(), 0x11, dtype=np.uint64)
    with pytest.raises(sshash_amd.SSHashError) as e:
        d.streaming_cover(reads, cover=cover)
    assert e.value.status == ERR_NO_DEVICE
    with pytest.raises(sshash_amd.SSHashError) as e:
        d.streaming_cover_from_file(FASTQ, cover=cover)
    assert e.value.status == ERR_NO_DEVICE
    bases, offsets = _batch(reads)
    assert lib.sshash_streaming_cover_device(d._h, 0, bases.ctypes.data, offsets.ctypes.data, 2, int(offsets[-1]), cover.ctypes.data, None,
                                             None) == ERR_NO_DEVICE
    assert lib.sshash_streaming_cover_device(d._h, 0, None, None, 0, 0, None, None, None) == ERR_NO_DEVICE
    counts = np.full(d.num_strings(), 7, dtype=np.uint64)
    assert lib.sshash_cover_string_counts_device(d._h, 0, cover.ctypes.data, counts.ctypes.data, None, None) == ERR_NO_DEVICE
    with pytest.raises(sshash_amd.SSHashError) as e:
        d.streaming_cover_device(0, bases.ctypes.data, offsets.ctypes.data, 2, cover.ctypes.data)
    assert e.value.status == ERR_NO_DEVICE
    assert (cover == 0x11).all() and (counts == 7).all()


def test_an_unsupported_extension_is_an_empty_report_without_any_device(tmp_path):
    """a query file whose extension says nothing: the call says "unsupported query file format" and returns before any device is asked for -- this dictionary is resident
    nowhere, and the call succeeds --, the report all zeros, a supplied bitmap untouched"""
    rng = np.random.default_rng(3)
    path = str(tmp_path / "tiny.fa")
    with open(path, "w") as f:
        for i in range(40):
            f.write(f">{i}\n{''.join('ACGT'[c] for c in rng.integers(0, 4, int(rng.integers(15, 300))))}\n")
    d = sshash_amd.Dictionary.build(path, k=15, m=7)
    q = tmp_path / "q.txt"
    q.write_text("ACGT\n")
    cover = np.full(d.cover_words(), 0x11, dtype=np.uint64)
    got, report = d.streaming_cover_from_file(str(q), cover=cover)
    assert got is cover and (cover == 0x11).all() and report == B.StreamingQueryReport()
    got, report = d.streaming_cover_from_file(str(q), multiline=True)
    assert got.shape == (d.cover_words(),) and not got.any() and report == B.StreamingQueryReport()
    rep = B._Report(1, 2, 3, 4, 5, 6)
    assert B._load().sshash_streaming_cover_from_file(d._h, os.fsencode(str(q)), 0, cover.ctypes.data, C.byref(rep)) == 0
    assert d._report(rep) == B.StreamingQueryReport() and (cover == 0x11).all()
    assert B._load().sshash_streaming_cover_from_file(d._h, os.fsencode(str(q)), 0, cover.ctypes.data, None) == 0
    with pytest.raises(sshash_amd.SSHashError) as e:  # (a file that cannot be opened: said before any device is asked for, too)
        d.streaming_cover_from_file(str(tmp_path / "missing.fa"), cover=cover)
    assert e.value.status == 2 and (cover == 0x11).all()


@pytest.mark.parametrize("case_name", CASES)
def test_string_counts_against_numpy(case_name, request):
    """the all-zero bitmap, the all-ones bitmap (valid bits only; and with the bits behind num_kmers set as well, which are not counted),
    random bitmaps of several densities, every string's own range alone"""
    case = request.getfixturevalue(case_name)
    d = case.dict
    n, words = d.num_kmers(), d.cover_words()
    sizes = d.string_size(np.arange(d.num_strings(), dtype=np.uint64))
    first, last = _string_id_ranges(d)
    assert (last - first == sizes).all() and int(sizes.sum()) == n
    if case_name != "case_se_regular":  # the synthetic dictionaries: strings of one k-mer, and strings that begin and end inside one word
        assert (sizes == 1).any()
        assert ((first >> np.uint64(6)) == ((last - np.uint64(1)) >> np.uint64(6))).any()
        assert ((first & np.uint64(63)) != 0).any() and ((last & np.uint64(63)) != 0).any()
    assert (sizes > 64).any()  # and strings over several words

    counts, total = d.cover_string_counts(np.zeros(words, dtype=np.uint64))
    assert counts.dtype == np.uint64 and counts.shape == (d.num_strings(),) and not counts.any() and total == 0

    ones = sshash_amd.ids_to_cover(np.arange(n, dtype=np.uint64), words)
    assert n % 64 == 0 or int(ones[-1]) == (1 << (n % 64)) - 1
    counts, total = d.cover_string_counts(ones)
    assert (counts == sizes).all() and total == n
    counts, total = d.cover_string_counts(np.full(words, ~np.uint64(0), dtype=np.uint64))  # bits at or above num_kmers are no k-mers
    assert (counts == sizes).all() and total == n

    rng = np.random.default_rng(5)
    for density in (0.5, 0.03, 0.97):
        ids = np.flatnonzero(rng.random(n) < density).astype(np.uint64)
        cover = sshash_amd.ids_to_cover(ids, words)
        counts, total = d.cover_string_counts(cover)
        want, want_total = _numpy_counts(d, cover)
        assert (counts == want).all(), np.flatnonzero(counts != want)[:10]
        assert total == want_total == ids.size
    # the overwrite rule, through the C ABI: counts and total hold something else before
    cover = sshash_amd.ids_to_cover(np.arange(int(first[1]), int(last[1]), dtype=np.uint64), words)
    raw = np.full(d.num_strings(), 77, dtype=np.uint64)
    total = C.c_uint64(123)
    assert B._load().sshash_cover_string_counts(d._h, cover.ctypes.data, raw.ctypes.data, C.byref(total)) == 0
    assert raw[1] == sizes[1] and raw.sum() == sizes[1] and total.value == sizes[1]
    assert B._load().sshash_cover_string_counts(d._h, cover.ctypes.data, raw.ctypes.data, None) == 0  # total may be NULL
