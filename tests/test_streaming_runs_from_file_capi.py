"""The runs of a query file (sshash_streaming_runs_from_file) and the run records over segments, as far as a machine without a GPU can
tell: the symbol is declared, exported, bound and present in the facade; the callback type has the stated signature; argument errors --
a null dictionary, filename or callback -- are reported before anything else, whether or not a device is there, and call nothing; a
dictionary that is not resident fails with SSHASH_ERR_NO_DEVICE; a file whose extension says nothing gives the zeroed report of the
other file calls; the header states the routes; and the host model of the merge (tests/cpp/check_segment_runs.cpp, over the arithmetic
of sshash_amd/csrc/segments.hpp) passes."""
from __future__ import annotations

import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import sshash_amd
from sshash_amd import _binding as B
from conftest import FASTQ, ROOT

SYMBOL = "sshash_streaming_runs_from_file"
ERR_ARGUMENT, ERR_NO_DEVICE = 1, 5


def test_the_symbol_is_declared_exported_bound_and_in_the_facade():
    header = open(os.path.join(ROOT, "include", "sshash_amd.h")).read()
    facade = open(os.path.join(ROOT, "include", "sshash_amd.hpp")).read()
    lib = C.CDLL(sshash_amd.library_path())
    bound = B._load()
    assert re.search(r"\b" + SYMBOL + r"\s*\(", header)
    assert hasattr(lib, SYMBOL) and SYMBOL in B.C_ABI_SYMBOLS
    assert getattr(bound, SYMBOL).restype is C.c_int
    assert SYMBOL + "(" in facade and re.search(r"\bstreaming_runs_from_file\s*\(", facade)
    assert callable(sshash_amd.Dictionary.streaming_runs_from_file)
    assert "sshash_read_runs_fn fn, void* ctx, sshash_streaming_report* report);" in header
    capi = open(os.path.join(ROOT, "sshash_amd", "csrc", "capi.cpp")).read()
    body = capi[capi.index("sshash_status " + SYMBOL):]
    body = body[:body.index("\n}\n")]
    assert "with_query_file(d, filename, multiline, true" in body and "for_each_batch(" in body, "every record of the file, through the sequential reader"


def test_the_callback_type_has_the_stated_signature():
    header = open(os.path.join(ROOT, "include", "sshash_amd.h")).read()
    stated = re.search(r"typedef int \(\*sshash_read_runs_fn\)\((.*?)\);", header, re.S).group(1)
    stated = re.sub(r"/\*.*?\*/", "", stated, flags=re.S)
    assert [" ".join(a.split()) for a in stated.split(",")] == ["void* ctx", "uint64_t first_read", "uint64_t n", "const uint64_t* run_offsets",
                                                               "const sshash_streaming_run* runs"]
    fn = B._ReadRunsFn
    assert fn._restype_ is C.c_int and list(fn._argtypes_) == [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p]
    assert B._SIGNATURES[SYMBOL] == (C.c_int, [C.c_void_p, C.c_char_p, C.c_int, B._ReadRunsFn, C.c_void_p, C.POINTER(B._Report)])


def test_argument_errors_come_first(case_skew_regular):
    """a null dictionary, filename or callback: SSHASH_ERR_ARGUMENT whether or not a device is there -- this dictionary is not resident --,
    the callback is never called, and with a null dictionary not even the report is touched"""
    d = case_skew_regular.dict
    lib = B._load()
    seen = []
    fn = B._ReadRunsFn(lambda ctx, first, n, ro, runs: seen.append(first) or 0)
    call = getattr(lib, SYMBOL)
    rep = B._Report(1, 2, 3, 4, 5, 6)
    assert call(None, os.fsencode(FASTQ), 0, fn, None, C.byref(rep)) == ERR_ARGUMENT
    assert rep.num_kmers == 1 and rep.num_extensions == 6
    assert call(d._h, None, 0, fn, None, C.byref(rep)) == ERR_ARGUMENT and lib.sshash_last_error()
    assert call(d._h, os.fsencode(FASTQ), 0, B._ReadRunsFn(), None, C.byref(rep)) == ERR_ARGUMENT
    assert call(d._h, None, 1, B._ReadRunsFn(), None, None) == ERR_ARGUMENT
    assert rep.num_kmers == 1 and seen == []


def test_a_dictionary_that_is_not_resident_is_no_device(tmp_path):
    """the errors of the arguments come before that of the device, and that one before any callback"""
    rng = np.random.default_rng(3)
    path = str(tmp_path / "tiny.fa")
    with open(path, "w") as f:
        for i in range(40):
            f.write(f">{i}\n{''.join('ACGT'[c] for c in rng.integers(0, 4, int(rng.integers(15, 300))))}\n")
    d = sshash_amd.Dictionary.build(path, k=15, m=7)
    seen = []
    for per_batch in (None, lambda first, ro, runs: seen.append(first)):
        with pytest.raises(sshash_amd.SSHashError) as e:
            d.streaming_runs_from_file(path, per_batch=per_batch)
        assert e.value.status == ERR_NO_DEVICE
    fn = B._ReadRunsFn(lambda ctx, first, n, ro, runs: seen.append(first) or 0)
    rep = B._Report(1, 2, 3, 4, 5, 6)
    call = getattr(B._load(), SYMBOL)
    assert call(d._h, os.fsencode(path), 0, fn, None, C.byref(rep)) == ERR_NO_DEVICE
    assert d._report(rep) == B.StreamingQueryReport() and seen == []
    assert call(d._h, None, 0, fn, None, None) == ERR_ARGUMENT
    # a file whose extension says nothing: the zeroed report of the other file calls, nothing called, nothing kept
    q = tmp_path / "q.txt"
    q.write_text("ACGT\n")
    ro, runs, report = d.streaming_runs_from_file(str(q))
    assert ro.dtype == np.uint64 and ro.tolist() == [0] and runs.dtype == sshash_amd.RUN_DTYPE and runs.shape == (0,)
    assert report == B.StreamingQueryReport() and seen == []


def test_the_header_states_the_routes():
    header = open(os.path.join(ROOT, "include", "sshash_amd.h")).read()
    segments = header[header.index("LONG READS"):header.index("sshash_set_read_segments(")]
    never = segments[segments.index("Never segmented"):]
    assert "sshash_streaming_runs" not in never and "sshash_streaming_best_run" in never and "sshash_streaming_lookup" in never
    host_calls = segments[segments.index("Host and file calls"):segments.index("Device calls")]
    device_calls = segments[segments.index("Device calls"):segments.index("Never segmented")]
    assert "_runs," in host_calls and "_runs_device" in device_calls and "13 more" in device_calls
    runs = header[header.index("WHERE a read hits"):header.index("WHICH k-mers of the dictionary a read set holds")]
    assert "never cut into segments" not in runs
    for words in ("sshash_set_read_segments", "one 32-bit add per joined seam", "byte for byte", "LOCAL TO THE BATCH", "IN FILE ORDER", "EVERY record",
                  "empty range", "2^31", "SSHASH_ERR_ARGUMENT", "sequential reader"):
        assert " ".join(words.split()) in " ".join(runs.replace(" * ", " ").split()), words


def test_the_host_model_of_the_merge():
    """tests/cpp/check_segment_runs.cpp: c, joined, c', E and cont over synthetic per-k-mer sequences cut at S in {1, 2, 7, 64}, merged,
    against the runs of the uncut sequences, at every capacity; `make sanitize` runs the same program under the sanitizers
    (tests/test_read_segments_capi.py)"""
    exe = os.path.join(ROOT, "tests", "cpp", "check_segment_runs")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "sshash_amd", "csrc"), exe.replace(ROOT, "../..")])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "EVERYTHING OK!" in p.stdout, p.stdout[-3000:] + p.stderr[-3000:]
    makefile = open(os.path.join(ROOT, "sshash_amd", "csrc", "Makefile")).read()
    assert "tools: ../../tests/cpp/check_segment_runs" in makefile and "build/check_segment_runs" in makefile
