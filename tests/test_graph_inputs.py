"""CPU: the inputs and the ground truth of tests/test_gpu_graph.py, the argument checks of the graph calls and the GFA helpers.

At every k of the GPU test the strings of gpu_graph_worker.make_graph must reach what the issue's cases need -- all 16 combinations of the
flag bits 2-5 of a link, links that land inside a string, string ends of degree 2, the circular string's link to itself, the hairpin's link
to its own reverse, a string without links, more than 8 192 strings -- and the ground truth (a plain Python dict) must agree with the CPU
oracle's lookups on the eight neighbours of every string. No device is needed: the argument errors come before anything runs."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np
import pytest

import sshash_amd
from conftest import Case
from gpu_graph_worker import (KS, U64_FIELDS, end_rows, expected_links, expected_masks, expected_string_neighbours, link_cases, m_of, make_graph, sub_ranges,
                              adjacency_ranges, truth)
from sshash_amd import _binding

INVALID = np.uint64(0xFFFFFFFFFFFFFFFF)


@pytest.mark.parametrize("k", KS, ids=[f"k{k}" for k in KS])
def test_generator_reaches_every_case_and_truth_agrees_with_the_oracle(k, tmp_path):
    from test_gpu_parity import _expand_neighbours

    strings, what = make_graph(k, 6000 + k)
    T = truth(strings, k)
    c = link_cases(T, what)
    assert c["strings"] > 8192 and 30000 <= c["kmers"] <= 60000, c
    assert c["combinations"] == list(range(16)), c  # (bit 2, bit 3, bit 4, bit 5): every one occurs
    assert c["interior_targets"] >= 40 and c["ends_of_degree_2"] >= 40 and c["signs"] == ["++", "+-", "-+", "--"], c
    assert c["loop_links"] == [16, 36], c  # END -> its own first k-mer; START -> its own last k-mer
    assert c["hairpin_links"] == [8 | 32], c  # END -> its own last k-mer, reversed: s+ -> s-
    assert c["isolated_has_no_links"] and c["strings_without_links"] >= 1, c
    one_strand = link_cases(T, what, both_strands=False)
    assert one_strand["hairpin_links"] == [] and 0 < one_strand["links"] < c["links"], one_strand
    sub_ranges(T, what), adjacency_ranges(T, what)  # (their own assertions: the tile edges, the stretches)
    # a junction inside a string: a k-mer that is no string end and has two neighbours on one side
    masks = expected_masks(T, True)
    forward, backward = sshash_amd.adjacency_degrees(masks)
    inner = np.ones(T.num_kmers, dtype=bool)
    inner[T.first[1:] - 1] = inner[T.first[:-1]] = False
    assert int(((forward > 1) | (backward > 1))[inner].sum()) >= 20

    # the oracle's lookups of the eight neighbours of every string, both flavours, both settings of check_reverse_complement
    sids = np.arange(T.num_strings)
    rows = end_rows(T, sids)
    for canonical in (False, True):
        case = Case(f"graph_k{k}_{int(canonical)}", strings, k, m_of(k), canonical, str(tmp_path))
        assert case.gt.num_kmers == T.num_kmers
        last = _expand_neighbours(case.gt.kmers(rows[:, 0].astype(np.uint64)), k, case.W).reshape(-1, 8 * case.W)
        first = _expand_neighbours(case.gt.kmers(rows[:, 4].astype(np.uint64)), k, case.W).reshape(-1, 8 * case.W)
        queries = np.ascontiguousarray(np.concatenate([last[:, :4 * case.W], first[:, 4 * case.W:]], 1)).reshape(-1)
        for check_rc in (True, False):
            got = case.oracle.lookup_packed(queries, check_rc)
            want = expected_string_neighbours(T, sids, canonical or check_rc)
            for f in U64_FIELDS:
                assert np.array_equal(got[f], want[f]), (canonical, check_rc, f)
            found = want["found"]
            assert np.array_equal(got["kmer_orientation"][found], want["kmer_orientation"][found].astype(got["kmer_orientation"].dtype)), (canonical, check_rc)


SIX = ["GATTACAG", "ACAGTC", "CCGACT", "TCGGA", "ACAGCT", "TACACC"]  # k = 5
# string 1 follows string 0, string 2 is the reverse of what follows string 1, string 3 (one k-mer) follows that; string 4 is the other
# branch behind string 0 and ends in the hairpin C + AG + CT; string 5 begins inside string 0 (T + TACA is its k-mer TTACA)
SIX_LINKS = [(0, 4, 9, 1 | 16), (0, 1, 4, 2 | 16), (1, 2, 7, 3 | 8 | 32), (1, 0, 3, 2 | 4 | 32), (2, 1, 5, 3 | 8 | 32), (2, 3, 8, 2 | 4 | 8 | 16 | 32),
             (3, 2, 6, 3 | 4 | 8 | 16), (4, 4, 10, 3 | 8 | 32), (4, 0, 3, 2 | 4 | 32), (5, 0, 2, 2 | 4)]
SIX_OFFSETS = [0, 2, 4, 6, 7, 9, 10]
SIX_GFA = """H\tVN:Z:1.0
S\t0\tGATTACAG\tLN:i:8
S\t1\tACAGTC\tLN:i:6
S\t2\tCCGACT\tLN:i:6
S\t3\tTCGGA\tLN:i:5
S\t4\tACAGCT\tLN:i:6
S\t5\tTACACC\tLN:i:6
L\t0\t+\t4\t+\t4M
L\t0\t+\t1\t+\t4M
L\t1\t+\t2\t-\t4M
L\t1\t-\t0\t-\t4M
L\t2\t+\t1\t-\t4M
L\t2\t-\t3\t+\t4M
L\t3\t-\t2\t+\t4M
L\t4\t+\t4\t-\t4M
L\t4\t-\t0\t-\t4M
"""


def six_links():
    links = np.zeros(len(SIX_LINKS), dtype=sshash_amd.LINK_DTYPE)
    for i, (a, b, kmer, flags) in enumerate(SIX_LINKS):
        links[i] = (a, b, kmer, flags, 0)
    return np.array(SIX_OFFSETS, dtype=np.uint64), links


@pytest.fixture(scope="module")
def six(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("six") / "six.fa")
    with open(path, "w") as f:
        f.write("".join(">\n" + s + "\n" for s in SIX))
    return path, sshash_amd.Dictionary.build(path, k=5, m=3, num_threads=1)


def test_gfa_of_six_strings(six, tmp_path):
    _, d = six
    offsets, links = six_links()
    w_offsets, w_links = expected_links(truth(SIX, 5), 0, 6, True)  # the hand-written records are what the ground truth gives
    assert np.array_equal(offsets, w_offsets) and links.tobytes() == w_links.tobytes()
    end_to_end, from_sign, to_sign = sshash_amd.links_gfa(links)
    assert end_to_end.tolist() == [True] * 9 + [False]
    assert b"".join(from_sign).decode() == "+++-+--+--" and b"".join(to_sign).decode() == "++---++---"
    at_end, at_start = sshash_amd.link_degrees(offsets, links)
    assert at_end.tolist() == [2, 1, 1, 0, 1, 0] and at_start.tolist() == [0, 1, 1, 1, 1, 1]
    forward, backward = sshash_amd.adjacency_degrees(np.array([0x00, 0x01, 0x81, 0xF0, 0x3C, 0xFF], dtype=np.uint8))
    assert forward.tolist() == [0, 1, 1, 0, 2, 4] and backward.tolist() == [0, 0, 1, 4, 2, 4]
    for name in ("six.gfa", "six.gfa.gz"):
        path = str(tmp_path / name)
        sshash_amd.write_gfa(d, path, offsets, links)
        if name.endswith(".gz"):
            import gzip

            assert gzip.open(path, "rt").read() == SIX_GFA
        else:
            assert open(path).read() == SIX_GFA


def test_link_record_layout():
    t = sshash_amd.LINK_DTYPE
    assert t.itemsize == 32 and [t.fields[f][1] for f in ("from_string", "to_string", "to_kmer_id", "flags", "reserved")] == [0, 8, 16, 24, 28]
    assert {"sshash_string_neighbours_device", "sshash_string_links_device", "sshash_string_links", "sshash_kmer_adjacency_device",
            "sshash_kmer_adjacency"} <= set(_binding.C_ABI_SYMBOLS)


def test_argument_errors_come_before_any_device(six):
    path, d = six
    lib = _binding._load()
    n, kmers = d.num_strings(), d.num_kmers()
    offsets = np.zeros(n + 1, dtype=np.uint64)
    links = np.zeros(8, dtype=sshash_amd.LINK_DTYPE)
    masks = np.zeros(kmers, dtype=np.uint8)
    ids = np.zeros(8, dtype=np.uint64)
    r = _binding._Results()
    r.kmer_id = ids.ctypes.data
    o, l, m = offsets.ctypes.data, links.ctypes.data, masks.ctypes.data
    ARGUMENT = 1
    for args in ((2, 1, 1, o, None, 0), (0, n + 1, 1, o, None, 0), (0, n, 1, None, None, 0), (0, n, 1, o, None, 8)):
        assert lib.sshash_string_links(d._h, *args) == ARGUMENT, args
        assert lib.sshash_string_links_device(d._h, 0, *args, None) == ARGUMENT, args
    assert lib.sshash_string_links(None, 0, n, 1, o, l, 8) == ARGUMENT
    for args in ((2, 1, 1, m), (0, kmers + 1, 1, m), (0, kmers, 1, None)):
        assert lib.sshash_kmer_adjacency(d._h, *args) == ARGUMENT, args
        assert lib.sshash_kmer_adjacency_device(d._h, 0, *args, None) == ARGUMENT, args
    assert lib.sshash_kmer_adjacency(None, 0, 0, 1, m) == ARGUMENT
    assert lib.sshash_string_neighbours_device(d._h, 0, None, n, 1, 1, C.byref(r), None) == ARGUMENT  # first_string + n > num_strings
    assert lib.sshash_string_neighbours_device(d._h, 0, None, 0, n + 1, 1, C.byref(r), None) == ARGUMENT
    assert lib.sshash_string_neighbours_device(d._h, 0, None, 0, 1, 1, None, None) == ARGUMENT
    assert lib.sshash_string_neighbours_device(d._h, 0, None, 0, 1, 1, C.byref(_binding._Results()), None) == ARGUMENT  # no kmer_id array
    with pytest.raises(sshash_amd.SSHashError):
        d.string_links(-1, 2)
    # a minimizer shard answers only the k-mers it owns: refused, as sshash_check_device refuses it
    shard = sshash_amd.Dictionary.build(path, k=5, m=3, num_threads=1, num_shards=2, shard_id=1)
    assert lib.sshash_string_links(shard._h, 0, n, 1, o, None, 0) == ARGUMENT and lib.sshash_string_links_device(shard._h, 0, 0, n, 1, o, None, 0, None) == ARGUMENT
    assert lib.sshash_kmer_adjacency(shard._h, 0, kmers, 1, m) == ARGUMENT and lib.sshash_kmer_adjacency_device(shard._h, 0, 0, kmers, 1, m, None) == ARGUMENT
