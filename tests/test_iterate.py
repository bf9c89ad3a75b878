"""The dictionary's k-mer iterator on the host (sshash_iterate_packed: Dictionary.kmers / string_kmers, the C++ facade's
begin / at_kmer_id / at_string_id). Expected k-mers always come from the input strings (GroundTruth, input order)."""
from __future__ import annotations

import os
import subprocess

import numpy as np
import pytest

import sshash_amd
from conftest import K63_FASTA, ROOT, SE_FASTA

CASES = ["case_skew_regular", "case_skew_canonical", "case_small_k", "case_m_equals_k", "case_k63_regular", "case_se_regular"]


def string_first_ids(case) -> np.ndarray:
    """first k-mer id of every string, plus num_kmers at the end"""
    sizes = np.array([len(s) - case.k + 1 for s in case.sequences], dtype=np.int64)
    return np.concatenate([[0], np.cumsum(sizes)])


def sub_ranges(case, seed=0, n_random=200):
    """[begin, end) ranges: whole strings, one id either side of string boundaries, single-k-mer strings, empty ranges,
    ranges ending at num_kmers, random ranges"""
    first = string_first_ids(case)
    n = int(first[-1])
    rng = np.random.default_rng(seed)
    out = [(0, n), (n, n), (0, 0), (5, 5), (max(0, n - 7), n), (n - 1, n)]
    picks = sorted(set(rng.integers(0, len(first) - 1, 12).tolist()) | {0, len(first) - 2})
    for s in picks:
        b, e = int(first[s]), int(first[s + 1])
        out += [(b, e), (b, min(n, e + 1)), (max(0, b - 1), e), (max(0, b - 1), min(n, b + 1)), (b, b + 1), (e - 1, e)]
    singles = [s for s in range(len(first) - 1) if first[s + 1] - first[s] == 1]
    out += [(int(first[s]), int(first[s]) + 1) for s in singles]
    out += [(max(0, int(first[s]) - 2), min(n, int(first[s]) + 3)) for s in singles]
    for _ in range(n_random):
        a, b = sorted(int(x) for x in rng.integers(0, n + 1, 2))
        out.append((a, b))
    return out


@pytest.mark.parametrize("case_name", CASES)
def test_whole_dictionary_equals_input_order(case_name, request):
    case = request.getfixturevalue(case_name)
    n = case.dict.num_kmers()
    assert n == case.gt.num_kmers
    got = case.dict.kmers()
    want = case.gt.kmers(np.arange(n))
    assert got.dtype == np.uint64 and got.size == n * case.W
    assert np.array_equal(got, want)
    assert np.array_equal(case.dict.kmers(0, n), want)


@pytest.mark.parametrize("case_name", CASES)
def test_sub_ranges(case_name, request):
    case = request.getfixturevalue(case_name)
    W = case.W
    for b, e in sub_ranges(case):
        got = case.dict.kmers(b, e)
        assert got.size == (e - b) * W, (b, e)
        want = case.gt.kmers(np.arange(b, e))
        assert np.array_equal(got, want), (b, e)
        assert np.array_equal(got, case.dict.access_packed(np.arange(b, e))), (b, e)


@pytest.mark.parametrize("case_name", ["case_skew_regular", "case_k63_regular", "case_m_equals_k"])
def test_string_kmers(case_name, request):
    case = request.getfixturevalue(case_name)
    from oracle.ground_truth import GroundTruth

    for s, seq in enumerate(case.sequences):
        want = GroundTruth([seq], case.k).kmers(np.arange(len(seq) - case.k + 1))
        assert np.array_equal(case.dict.string_kmers(s), want), s
    with pytest.raises(sshash_amd.SSHashError):
        case.dict.string_kmers(len(case.sequences))


def test_argument_errors(case_skew_regular):
    d = case_skew_regular.dict
    n = d.num_kmers()
    for b, e in ((5, 4), (0, n + 1), (n, n + 1), (n + 1, n + 1)):
        with pytest.raises(sshash_amd.SSHashError) as err:
            d.kmers(b, e)
        assert err.value.status == 1, (b, e)
    assert d.kmers(n, n).size == 0


def test_null_output_with_a_range_is_refused(case_skew_regular):
    import ctypes as C

    from sshash_amd import _binding

    lib = _binding._load()
    d = case_skew_regular.dict
    assert lib.sshash_iterate_packed(d._h, 0, 3, None) == 1
    assert lib.sshash_iterate_packed(d._h, 3, 3, None) == 0
    out = np.zeros(8, dtype=np.uint64)
    assert lib.sshash_iterate_packed(d._h, 0, 2, out.ctypes.data_as(C.c_void_p)) == 0
    assert np.array_equal(out[:2], case_skew_regular.gt.kmers(np.arange(2)))
    assert (out[2:] == 0).all()


@pytest.mark.parametrize("args", [(SE_FASTA, "31", "13"), (SE_FASTA, "31", "13", "--canonical"), (K63_FASTA, "63", "25")],
                         ids=["se_regular", "se_canonical", "k63_regular"])
def test_cpp_facade_iterators(args):
    """tests/cpp/check_iterators.cpp: the reference's check_correctness_kmer_iterator / _string_iterator over the facade"""
    exe = os.path.join(ROOT, "tests", "cpp", "check_iterators")
    if not os.path.exists(exe):  # a build product inside tests/: gone when tests/ is replaced after build(). Host code by g++, linked
        # against the library as it stands (-o: make takes it as given and rebuilds nothing of it)
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "sshash_amd", "csrc"), "-o", "../libsshash_amd.so", "../../tests/cpp/check_iterators"])
    assert os.path.exists(exe), "built by the tools target of sshash_amd/csrc/Makefile"
    p = subprocess.run([exe, *args], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout + p.stderr
    assert p.stdout.count("EVERYTHING OK!") == 3, p.stdout
