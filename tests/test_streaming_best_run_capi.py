"""The streaming anchors (per read, its longest run) at the C ABI and in the binding, as far as a machine without a GPU can tell: the
five symbols are declared, exported, bound and present in the facade; the header states the rule; argument errors -- null pointers --
are reported before anything else and write nothing, guard bytes around `best` included; num_reads == 0 is no work; a dictionary that
is not resident fails with SSHASH_ERR_NO_DEVICE; and the host variant of the finish, sshash_runs_best, against numpy on CSR arrays made
by hand: empty ranges at the front, in the middle and at the end, a tie (the first wins), a tie between a forward and a backward run
(bit 31 takes no part), a single record, a read of 5 000 records whose longest is the last, one read alone."""
from __future__ import annotations

import ctypes as C
import os
import re

import numpy as np
import pytest

import sshash_amd
from sshash_amd import _binding as B
from conftest import FASTQ, ROOT

SYMBOLS = ("sshash_streaming_best_run", "sshash_streaming_best_run_device", "sshash_streaming_best_run_from_file", "sshash_runs_best",
           "sshash_runs_best_device")
METHODS = ("streaming_best_run", "streaming_best_run_device", "streaming_best_run_from_file", "runs_best_device")
ERR_ARGUMENT, ERR_NO_DEVICE = 1, 5
BACKWARD = 0x80000000
GUARD = 0x5A


def _batch(reads):
    chunks = [r.encode() for r in reads]
    offsets = np.zeros(len(chunks) + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum([len(c) for c in chunks], dtype=np.uint64)
    return np.frombuffer(b"".join(chunks) or b"\0", dtype=np.uint8), offsets


def hand_made_csr():
    """-> (run_offsets, runs, the index of every read's best record or -1): the CSR the GPU worker hands to runs_best_device as well"""
    lengths = [[], [], [3, 7, 7, 2], [], [4 | BACKWARD, 4], [6, 6 | BACKWARD, 1], [9 | BACKWARD], [], list(range(1, 5000)) + [5000], [2, 1], [], []]
    want = [-1, -1, 1, -1, 0, 0, 0, -1, 4999, 0, -1, -1]
    counts = [len(l) for l in lengths]
    run_offsets = np.zeros(len(lengths) + 1, dtype=np.uint64)
    run_offsets[1:] = np.cumsum(counts, dtype=np.uint64)
    runs = np.zeros(int(run_offsets[-1]), dtype=sshash_amd.RUN_DTYPE)
    flat = np.array([n for l in lengths for n in l], dtype=np.uint32)
    runs["num_kmers"] = flat
    runs["kmer_id"] = np.arange(runs.size, dtype=np.uint64) * np.uint64(1000003) + np.uint64(1 << 40)  # (every record its own bytes)
    runs["string_id"] = np.arange(runs.size, dtype=np.uint64) % np.uint64(17)
    runs["kmer_id_in_string"] = np.arange(runs.size, dtype=np.uint64) * np.uint64(7)
    runs["read_pos"] = np.concatenate([np.arange(c, dtype=np.uint32) * np.uint32(3) for c in counts])
    return run_offsets, runs, want


def numpy_runs_best(run_offsets, runs):
    """the header's rule by a stable sort: the largest num_kmers & 0x7FFFFFFF, among equals the first; zeros for an empty range"""
    n = run_offsets.size - 1
    best = np.zeros(n, dtype=sshash_amd.RUN_DTYPE)
    for r in range(n):
        mine = runs[int(run_offsets[r]):int(run_offsets[r + 1])]
        if mine.size:
            best[r] = mine[np.argsort(-(mine["num_kmers"] & np.uint32(0x7FFFFFFF)).astype(np.int64), kind="stable")[0]]
    return best


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
    assert callable(sshash_amd.runs_best) and "runs_best" in sshash_amd.__all__
    assert re.search(r"\bruns_best\s*\(", facade)
    assert "typedef int (*sshash_read_best_run_fn)(void* ctx, uint64_t first_read, uint64_t n, const sshash_streaming_run* best);" in header
    # the section stands behind the class finish calls, on its own
    assert header.index("ANCHORS: per read") > header.index("sshash_class_totals(")
    # what the header has to say: the tie rule, the zero record, what is written, that segments never apply, what a shard returns
    section = header[header.index("ANCHORS: per read"):header.index("sshash_runs_best(")]
    for words in ("num_kmers & 0x7FFFFFFF", "smallest read_pos", "first in read order", "32 zero bytes", "num_kmers == 0", "OVERWRITTEN",
                  "nothing outside", "Segments never apply", "sshash_set_read_segments", "not additive", "minimizer shard", "SSHASH_ERR_ARGUMENT",
                  "do not combine", "sshash_streaming_runs", "run_offsets[r + 1]", "2^31", "2^16", "SSHASH_ERR_NO_DEVICE"):
        assert words in section, words
    capi = open(os.path.join(ROOT, "sshash_amd", "csrc", "capi.cpp")).read()
    assert "static_assert(sizeof(sshash_streaming_run) == 32" in capi and sshash_amd.RUN_DTYPE.itemsize == 32


def test_argument_errors_come_first_and_write_nothing(case_skew_regular):
    """a null dictionary, null bases / read_offsets / best with num_reads > 0, a null callback: SSHASH_ERR_ARGUMENT whether or not a
    device is there -- this dictionary is not resident --, and not a byte of `best` or around it is written"""
    d = case_skew_regular.dict
    lib = B._load()
    bases, offsets = _batch([case_skew_regular.sequences[0], "ACGT"])
    room = np.full(32 + 2 * 32 + 32, GUARD, dtype=np.uint8)  # guard bytes on both sides of two records
    best = room[32:].ctypes.data
    rep = B._Report(1, 2, 3, 4, 5, 6)
    b, o = bases.ctypes.data, offsets.ctypes.data
    fn = B._PerReadFn(lambda *a: 0)
    host, device, from_file = lib.sshash_streaming_best_run, lib.sshash_streaming_best_run_device, lib.sshash_streaming_best_run_from_file
    assert host(None, b, o, 2, best, C.byref(rep)) == ERR_ARGUMENT
    assert rep.num_kmers == 1  # (a null dictionary: not even the report is touched)
    assert host(d._h, None, o, 2, best, None) == ERR_ARGUMENT
    assert host(d._h, b, None, 2, best, None) == ERR_ARGUMENT
    assert host(d._h, b, o, 2, None, None) == ERR_ARGUMENT and lib.sshash_last_error()
    # (host pointers stand in for device pointers: the call must refuse before it touches them)
    assert device(None, 0, b, o, 2, 0, best, None, None) == ERR_ARGUMENT
    assert device(d._h, 0, None, o, 2, 0, best, None, None) == ERR_ARGUMENT
    assert device(d._h, 0, b, None, 2, 0, best, None, None) == ERR_ARGUMENT
    assert device(d._h, 0, b, o, 2, 0, None, None, None) == ERR_ARGUMENT
    assert from_file(None, os.fsencode(FASTQ), 0, fn, None, None) == ERR_ARGUMENT
    assert from_file(d._h, None, 0, fn, None, None) == ERR_ARGUMENT
    assert from_file(d._h, os.fsencode(FASTQ), 0, B._PerReadFn(), None, None) == ERR_ARGUMENT
    run_offsets, runs, _ = hand_made_csr()
    ro, ru = run_offsets.ctypes.data, runs.ctypes.data
    assert lib.sshash_runs_best_device(None, 0, ro, ru, 2, best, None) == ERR_ARGUMENT
    assert lib.sshash_runs_best_device(d._h, 0, None, ru, 2, best, None) == ERR_ARGUMENT
    assert lib.sshash_runs_best_device(d._h, 0, ro, ru, 2, None, None) == ERR_ARGUMENT
    assert lib.sshash_runs_best(None, ru, 2, best) == ERR_ARGUMENT
    assert lib.sshash_runs_best(ro, ru, 2, None) == ERR_ARGUMENT
    assert lib.sshash_runs_best(ro, None, 3, best) == ERR_ARGUMENT  # (read 2 has records, and there are none to read)
    assert (room == GUARD).all(), "an argument error wrote into best or around it"
    for bad in ((run_offsets.astype(np.float64), runs), (run_offsets, runs.view(np.uint8)), (run_offsets[:0], runs), (run_offsets[::-1], runs),
                (run_offsets, runs[:5]), (run_offsets[3:], runs)):
        with pytest.raises(ValueError):
            sshash_amd.runs_best(*bad)


def test_no_reads_is_no_work(case_skew_regular):
    """num_reads == 0 succeeds without a device and touches nothing but the report, which the host call zeroes"""
    d = case_skew_regular.dict
    lib = B._load()
    room = np.full(3 * 32, GUARD, dtype=np.uint8)
    rep = B._Report(1, 2, 3, 4, 5, 6)
    assert lib.sshash_streaming_best_run(d._h, None, None, 0, room.ctypes.data, C.byref(rep)) == 0
    assert rep.num_kmers == 0 and rep.num_searches == 0
    assert lib.sshash_streaming_best_run(d._h, None, None, 0, None, None) == 0
    assert lib.sshash_runs_best(None, None, 0, None) == 0
    assert lib.sshash_runs_best(None, None, 0, room.ctypes.data) == 0
    assert (room == GUARD).all()
    best, report = d.streaming_best_run([])
    assert best.dtype == sshash_amd.RUN_DTYPE and best.shape == (0,) and report == B.StreamingQueryReport()
    none = sshash_amd.runs_best(np.zeros(1, dtype=np.uint64), np.zeros(0, dtype=sshash_amd.RUN_DTYPE))
    assert none.dtype == sshash_amd.RUN_DTYPE and none.shape == (0,)


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
    with pytest.raises(sshash_amd.SSHashError) as e:
        d.streaming_best_run(reads)
    assert e.value.status == ERR_NO_DEVICE
    with pytest.raises(sshash_amd.SSHashError) as e:
        d.streaming_best_run_from_file(path)
    assert e.value.status == ERR_NO_DEVICE
    bases, offsets = _batch(reads)
    room = np.full(32 + 2 * 32 + 32, GUARD, dtype=np.uint8)
    rep = np.full(6, 9, dtype=np.uint64)
    run_offsets, runs, _ = hand_made_csr()
    assert lib.sshash_streaming_best_run_device(d._h, 0, bases.ctypes.data, offsets.ctypes.data, 2, 0, room[32:].ctypes.data, rep.ctypes.data, None) == ERR_NO_DEVICE
    assert lib.sshash_streaming_best_run(d._h, bases.ctypes.data, offsets.ctypes.data, 2, room[32:].ctypes.data, None) == ERR_NO_DEVICE
    assert lib.sshash_runs_best_device(d._h, 0, run_offsets.ctypes.data, runs.ctypes.data, 2, room[32:].ctypes.data, None) == ERR_NO_DEVICE
    assert (room == GUARD).all() and (rep == 9).all()


def test_an_unsupported_extension_comes_behind_the_readiness_check(tmp_path):
    """a query file whose extension says nothing, on a dictionary that is resident nowhere: SSHASH_ERR_NO_DEVICE, not the empty report
    of the other file calls -- best_run_ready() comes before the file is opened --; the report is zeroed all the same, per_read is
    never called"""
    rng = np.random.default_rng(3)
    path = str(tmp_path / "tiny.fa")
    with open(path, "w") as f:
        for i in range(40):
            f.write(f">{i}\n{''.join('ACGT'[c] for c in rng.integers(0, 4, int(rng.integers(15, 300))))}\n")
    d = sshash_amd.Dictionary.build(path, k=15, m=7)
    q = tmp_path / "q.txt"
    q.write_text("ACGT\n")
    seen = []
    for per_read in (None, lambda first, best: seen.append(first)):
        with pytest.raises(sshash_amd.SSHashError) as e:
            d.streaming_best_run_from_file(str(q), per_read=per_read)
        assert e.value.status == ERR_NO_DEVICE
    rep = B._Report(1, 2, 3, 4, 5, 6)
    fn = B._PerReadFn(lambda ctx, first, n, rows: seen.append(first) or 0)
    assert B._load().sshash_streaming_best_run_from_file(d._h, os.fsencode(str(q)), 0, fn, None, C.byref(rep)) == ERR_NO_DEVICE
    assert d._report(rep) == B.StreamingQueryReport() and seen == []
    assert B._load().sshash_streaming_best_run_from_file(d._h, os.fsencode(str(q)), 0, fn, None, None) == ERR_NO_DEVICE
    with pytest.raises(sshash_amd.SSHashError) as e:  # (nor is a file that cannot be opened looked for before that)
        d.streaming_best_run_from_file(str(tmp_path / "missing.fa"))
    assert e.value.status == ERR_NO_DEVICE


def test_runs_best_on_the_host_against_numpy_on_a_csr_made_by_hand():
    run_offsets, runs, want_at = hand_made_csr()
    counts = np.diff(run_offsets.astype(np.int64))
    assert counts[0] == 0 and counts[1] == 0 and counts[3] == 0 and counts[-1] == 0 and counts[-2] == 0  # empty: front, middle, end
    assert counts[6] == 1 and counts[8] == 5000
    got = sshash_amd.runs_best(run_offsets, runs)
    assert got.dtype == sshash_amd.RUN_DTYPE and got.shape == (len(want_at),)
    want = np.zeros(len(want_at), dtype=sshash_amd.RUN_DTYPE)
    for r, at in enumerate(want_at):
        if at >= 0:
            want[r] = runs[int(run_offsets[r]) + at]
    assert got.tobytes() == want.tobytes(), [r for r in range(len(want_at)) if got[r] != want[r]]
    assert got.tobytes() == numpy_runs_best(run_offsets, runs).tobytes()
    # the tie between the strands: the first wins whichever of the two is backward
    assert got["num_kmers"][4] == 4 | BACKWARD and got["num_kmers"][5] == 6 and got["read_pos"][4] == 0 and got["read_pos"][5] == 0
    assert got["num_kmers"][8] == 5000 and got["read_pos"][8] == 3 * 4999
    assert not got[[0, 1, 3, 7, 10, 11]].tobytes().strip(b"\0")
    # a backward run that is longer than every forward run wins by its length, not by bit 31; a forward one beats a shorter backward one
    offsets = np.array([0, 2, 4], dtype=np.uint64)
    two = np.zeros(4, dtype=sshash_amd.RUN_DTYPE)
    two["num_kmers"] = [5, 9 | BACKWARD, 3 | BACKWARD, 4]
    two["read_pos"] = [0, 40, 0, 40]
    assert sshash_amd.runs_best(offsets, two)["read_pos"].tolist() == [40, 40]
    # one read alone; the output is overwritten, and nothing around it
    lib = B._load()
    room = np.full(32 + 32 + 32, 0x77, dtype=np.uint8)
    one = np.array([0, 3], dtype=np.uint64)
    assert lib.sshash_runs_best(one.ctypes.data, runs[2:].ctypes.data, 1, room[32:].ctypes.data) == 0
    assert (room[:32] == 0x77).all() and (room[64:] == 0x77).all() and room[32:64].tobytes() == runs[2:3].tobytes()
    empty = np.array([0, 0], dtype=np.uint64)
    assert lib.sshash_runs_best(empty.ctypes.data, None, 1, room[32:].ctypes.data) == 0
    assert (room[:32] == 0x77).all() and (room[64:] == 0x77).all() and not room[32:64].any()
    # random CSRs with few distinct lengths: ties everywhere
    rng = np.random.default_rng(5)
    for n in (1, 2, 300):
        counts = rng.integers(0, 6, n)
        offsets = np.zeros(n + 1, dtype=np.uint64)
        offsets[1:] = np.cumsum(counts, dtype=np.uint64)
        recs = np.zeros(int(offsets[-1]), dtype=sshash_amd.RUN_DTYPE)
        recs["num_kmers"] = rng.integers(1, 4, recs.size).astype(np.uint32) | (rng.integers(0, 2, recs.size).astype(np.uint32) << np.uint32(31))
        recs["kmer_id"] = np.arange(recs.size)
        assert sshash_amd.runs_best(offsets, recs).tobytes() == numpy_runs_best(offsets, recs).tobytes(), n
