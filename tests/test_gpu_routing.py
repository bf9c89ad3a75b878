"""GPU: the routing layer of the multi-GPU lookup -- sshash_route_bucket_device, sshash_route_bucket_by_key_device,
sshash_route_combine_device and sshash_sharded_lookup_device beyond two k = 31 ranks. Every case is one run of tests/gpu_routing_worker.py
in a fresh process with a time limit of its own, on one dictionary of conftest.skewed_sequences. The worker holds the owners of every
query against a numpy restatement of the minimizer rules (itself held against route_device first) and against the host's election of the
table key (tests/cpp/route_owners.cpp, built here with g++); runs the public two-call protocol -- whose scattering launch elects the owners
again, a branch the sharded lookup never takes -- at 1 .. 1024 shards and at the sizes around a tile and a workgroup, checking the counts
added to non-zero cursors, the regions of `slots` as sets, `send` word for word, guard words and the cursors it leaves; route_combine
against the same loop in numpy with two replies per query in both orders; the argument errors, n = 0 and a caller's stream; and the whole
sharded lookup at 1, 3 and 8 ranks (threads, one handle and stream each) over minimizer and table shards against the whole dictionary's
oracle, with ragged batches: empty, one k-mer, one k-mer 4097 times, negatives only, positives of a single owner. Which kinds of input
were there is asserted from the references and reported; so is which form of route_bucket_kernel<W, SCATTER, BY_KEY> ran."""
from __future__ import annotations

import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT

POINTS = [(31, 11, False), (31, 11, True), (63, 17, False), (63, 17, True)]
_STOPPED = []  # why no further worker is started: one of them faulted, aborted or ran out of time


@pytest.fixture(scope="module")
def route_owners(tmp_path_factory):
    """tests/cpp/route_owners.cpp by plain g++: the host's election of a k-mer's table-key owner"""
    exe = str(tmp_path_factory.mktemp("route_owners") / "route_owners")
    subprocess.check_call(["g++", "-O2", "-std=c++17", os.path.join(ROOT, "tests", "cpp", "route_owners.cpp"), "-o", exe])
    return exe


def test_route_owners_builds_with_plain_gpp_and_is_strand_symmetric(tmp_path):
    """No GPU: the reference of the table-key owners compiles for the host, names a shard below num_shards, and gives a k-mer and its
    reverse complement the same owner (k-mers as bytes on stdin, one uint32 per k-mer and shard count on stdout)."""
    import numpy as np

    from gpu_routing_worker import host_key_owners, random_kmers, revcomp

    exe = str(tmp_path / "route_owners")
    subprocess.check_call(["g++", "-O2", "-std=c++17", os.path.join(ROOT, "tests", "cpp", "route_owners.cpp"), "-o", exe])
    for k, key_length in ((31, 11), (31, 21), (63, 17), (63, 25)):
        W = 1 if k <= 31 else 2
        q = random_kmers(np.random.default_rng(k), 3000, k, W)
        q[:W * 100] &= np.uint64(0x3333333333333333)  # low-complexity k-mers: repeated m-mers, ties
        there, back = (host_key_owners(exe, x, k, key_length, (1, 3, 1024)) for x in (q, revcomp(q, k, W)))
        for S in (1, 3, 1024):
            assert there[S].shape == (3000,) and (there[S] < S).all() and (there[S] == back[S]).all(), (k, key_length, S)
        assert len(np.unique(there[1024])) > 900
    assert subprocess.run([exe, "31", "11", "0"], input=b"", capture_output=True).returncode != 0


@pytest.mark.gpu
@pytest.mark.parametrize("k,m,canonical", POINTS, ids=[f"k{k}_{'canonical' if c else 'regular'}" for k, m, c in POINTS])
def test_routing(k, m, canonical, route_owners, tmp_path):
    assert not _STOPPED, "not started: " + _STOPPED[0]
    env = dict(os.environ)
    for name in ("SSHASH_AMD_TEST_HOOKS", "SSHASH_AMD_SKTABLE", "SSHASH_AMD_SK_M", "SSHASH_AMD_HBM_BUDGET"):
        env.pop(name, None)
    try:
        p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "gpu_routing_worker.py"), str(k), str(m), str(int(canonical)),
                            str(70 + k + int(canonical)), route_owners, str(tmp_path)], capture_output=True, text=True, timeout=600, env=env)
    except subprocess.TimeoutExpired:
        _STOPPED.append(f"the worker of k = {k}, canonical = {canonical} ran into its time limit")
        raise
    if p.returncode < 0 or p.returncode in (134, 139) or "illegal memory access" in p.stderr:  # a signal, an abort, a GPU fault: no further worker
        _STOPPED.append(f"the worker of k = {k}, canonical = {canonical} ended with status {p.returncode}")
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-6000:]
    got = json.loads(p.stdout.strip().splitlines()[-1])
    print(got)
    assert got["ok"] and got["k"] == k and got["canonical"] == canonical
    W = 1 if k <= 31 else 2
    # every form of route_bucket_kernel<W, SCATTER, BY_KEY> of this k: through the public calls (the scatter elects the owners again) and
    # through the sharded lookup (the scatter reads the owners the counting launch left)
    assert got["forms"] == sorted(f"W={W} SCATTER={s} BY_KEY={b}{how}" for s in (0, 1) for b in (0, 1) for how in ("", " known owners"))
    kinds, sharded = got["kinds"], got["sharded"]
    assert kinds["dictionary_kmers_in_the_mixed_batch"] > 0 and kinds["random_kmers_in_the_mixed_batch"] > 0
    assert kinds["repeated_kmer_batches"] > 0 and kinds["alternating_batches"] > 0 and kinds["side_stream_runs"] > 0 and kinds["reverse_complement_batches"] > 0
    assert all(kinds["empty_shards_at_S1000_n257_" + e] > 0 for e in ("minimizer1", "minimizer0", "key1"))
    assert all(lo > 0 for lo, hi in kinds["messages_per_shard_min_max"].values()) and "S64_key1" in kinds["messages_per_shard_min_max"]
    assert sum(kinds["table_keys_of_three_shards"]) == kinds["table_keys"]
    assert set(kinds["combine"]) == {"255", "257", "4097"} and all(v > 0 for c in kinds["combine"].values() for v in c.values())
    if not canonical:
        assert kinds["combinations_with_one_owner_and_two_owner_queries"] > 0 and sharded["runs_with_two_owner_queries"] > 0
        assert {"S1000_minimizer1", "S1024_minimizer1"} <= set(kinds["messages_per_shard_min_max"])
    assert sharded["runs_where_every_query_has_one_owner"] > 0 and sharded["check_rc_0_rounds"] >= 6
    assert sharded["ranks_whose_batch_has_a_single_owner"] > 0 and sharded["owners_that_get_nothing_from_a_rank"] > 0
    assert all(v > 0 for v in sharded["batches"].values()) and 0 < sharded["found"] < sharded["queries"]
