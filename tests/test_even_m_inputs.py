"""CPU: the inputs of tests/test_gpu_even_m.py (gpu_even_m_worker.make_point: dictionaries of an even minimizer length with planted
self-complementary m-mers) and the references the GPU test trusts, before a device is involved. For every point and flavour: the
canonical k-mers of the input are distinct; enough k-mers tie -- in the table key (tests/cpp/table_keys.cpp, the host's build of sk_key)
and, for a canonical dictionary, in the minimizer --, enough absent k-mers tie, and the reads walk over enough ties; the oracle returns
id i for k-mer i on both strands; its streaming counters equal a brute-force count over the input strings."""
from __future__ import annotations

import subprocess

import numpy as np
import pytest

from gpu_even_m_worker import (FLOOR, INVALID, POINTS, RECORD, assert_floors, build_host_tool, canonical_words, key_length_of, make_point,
                               table_keys)
from gpu_per_read_worker import revcomp as revcomp_str
from gpu_routing_worker import random_kmers, revcomp


@pytest.fixture(scope="module")
def table_keys_exe(tmp_path_factory):
    return build_host_tool("table_keys", tmp_path_factory.mktemp("table_keys"))


def test_table_keys_gives_what_sk_key_elects(table_keys_exe):
    """one 16-byte record per k-mer; a k-mer and its reverse complement tie together, and otherwise elect the same key at the same
    place of opposite strands; the key is the m-mer at the elected position of the elected strand"""
    for k, m in ((15, 4), (31, 12), (31, 30), (33, 12), (63, 16)):
        W, L = 1 if k <= 31 else 2, key_length_of(k, m)
        q = random_kmers(np.random.default_rng(k + m), 4000, k, W)
        there, back = table_keys(table_keys_exe, q, k, L), table_keys(table_keys_exe, revcomp(q, k, W), k, L)
        assert there.dtype == RECORD and there.shape == (4000,) and (there["zero"] == 0).all()
        assert (there["tie"] == back["tie"]).all() and set(np.unique(there["tie"])) <= {0, 1}
        keyed = there["tie"] == 0
        assert (there["key"][keyed] == back["key"][keyed]).all() and (there["pos"][keyed] == back["pos"][keyed]).all()
        assert (there["rc"][keyed] != back["rc"][keyed]).all() and (there["pos"] <= k - L).all()
        strand = np.where((there["rc"] != 0)[:, None], revcomp(q, k, W).reshape(-1, W), q.reshape(-1, W))
        for i in np.flatnonzero(keyed)[:500]:
            whole = int(strand[i, 0]) | (int(strand[i, 1]) << 64 if W == 2 else 0)
            assert (whole >> (2 * int(there["pos"][i]))) & ((1 << (2 * L)) - 1) == int(there["key"][i])
    assert subprocess.run([table_keys_exe, "31", "40"], input=b"", capture_output=True).returncode != 0


@pytest.mark.parametrize("canonical", [False, True], ids=["regular", "canonical"])
@pytest.mark.parametrize("k,m", POINTS, ids=[f"k{k}m{m}" for k, m in POINTS])
def test_inputs_and_references(k, m, canonical, table_keys_exe, tmp_path):
    pt = make_point(k, m, canonical, table_keys_exe, str(tmp_path))
    case, W, n = pt.case, pt.W, pt.case.gt.num_kmers
    # every canonical k-mer once
    assert np.unique(canonical_words(pt.every, k, W), axis=0).shape[0] == n
    assert 1000 <= n <= 10000
    # every planted P is its own reverse complement and lies where the generator says
    assert len(pt.planted) >= 12
    for p, s, at in pt.planted:
        assert len(p) == m and p == revcomp_str(p) and pt.sequences[s][at:at + m] == p
    assert any(at == 0 for p, s, at in pt.planted) and any(at + m == len(pt.sequences[s]) for p, s, at in pt.planted)
    if k - m >= m + 1:  # two copies inside one window
        places = {}
        for p, s, at in pt.planted:
            places.setdefault((p, s), []).append(at)
        assert any(len(v) == 2 and m <= v[1] - v[0] <= k - m for v in places.values())
    # the floors, from the references alone
    counts = assert_floors(pt)
    print(f"k={k} m={m} canonical={canonical}: {n} k-mers in {len(pt.sequences)} strings, ties {counts}")
    for kind in pt.kinds:
        assert (pt.pool_ties[kind] & pt.pool_found).sum() >= FLOOR and (pt.pool_ties[kind] & ~pt.pool_found).sum() >= FLOOR
    # the oracle: id i for k-mer i, on both strands, every field of a hit from the input
    ids = np.arange(n, dtype=np.uint64)
    for q, orientation in ((pt.every, 1), (pt.every_rc, -1)):
        got = case.oracle.lookup_packed(q, True)
        assert (got["kmer_id"] == ids).all() and (got["kmer_orientation"] == orientation).all()
        assert (got["string_id"] == case.gt.string_id).all() and (got["kmer_id_in_string"] == case.gt.in_string).all()
    for kind in pt.kinds:
        assert (case.oracle.lookup_ids(pt.negative_ties[kind]) == INVALID).all()
        assert (case.gt.lookup(pt.negative_ties[kind])["kmer_id"] == INVALID).all()
    # the oracle's streaming counters against a brute-force count over the input strings
    present = set()
    for s in pt.sequences:
        for i in range(len(s) - k + 1):
            x = s[i:i + k]
            present.add(min(x, revcomp_str(x)))
    assert len(present) == n
    valid = set("ACGT")
    total = positive = invalid = 0
    for r in pt.reads:
        r = r.upper()
        for i in range(len(r) - k + 1):
            x = r[i:i + k]
            total += 1
            if not set(x) <= valid:
                invalid += 1
            elif min(x, revcomp_str(x)) in present:
                positive += 1
    rep = case.oracle.streaming_query(pt.reads)
    assert (rep["num_kmers"], rep["num_positive_kmers"], rep["num_negative_kmers"], rep["num_invalid_kmers"]) == (total, positive, total - positive - invalid, invalid)
    assert positive >= 1000 and invalid > 0 and total - positive - invalid > 0
