"""GPU: the streaming sums -- per read, the sum of a value per k-mer over the read's positive k-mers, and their number. Every case is
one run of tests/gpu_sums_worker.py in a fresh process with a time limit of its own (the environment switch that decides whether a
replica holds the super-k-mer table is read once per process). The worker checks, with exact integer equality, against values[ids].sum()
and (ids valid).sum() per read over streaming_lookup's kmer_id values and over the CPU oracle's point lookups of every k-mer of every
read: value_prefix_device against numpy.cumsum in 64 bits (word 0, the last word, guard words on both sides); the device, host and
file entry points row for row, over values that are random, all 0xFFFFFFFF (sums above 2^32), all ones (sum == positive_kmers) and
thresholded (at_least 1, 500, 0xFFFFFFFF); positive_kmers against column 1 of streaming_query_per_read; the six counters against
streaming_query's; rows that held garbage overwritten, hitless reads included; guard words around the rows, which lie at an address that
is a multiple of 8 and not of 16; identical rows under the hooks stream_piece_reads and stream_move_out_every; identical rows with the
reads cut into segments of 1, 7 and 64 k-mers through the device and the host call, the read above 2^16 bases at the default S and, with
segments off, through the per-k-mer route. Before it touches the GPU it asserts from the oracle's ids that every kind of read is there.
Two more workers: two minimizer shards, whose rows added are the whole index's, and the round trip depth -> weighted FASTA -> weighted
build, whose weights give the rows the depth array gives."""
from __future__ import annotations

import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def run_worker(args, table, tmp_path):
    env = dict(os.environ)
    env.pop("SSHASH_AMD_TEST_HOOKS", None)
    if table:
        env.pop("SSHASH_AMD_SKTABLE", None)
    else:
        env["SSHASH_AMD_SKTABLE"] = "0"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "gpu_sums_worker.py")] + [str(a) for a in args[:2]] + [str(tmp_path)] + list(args[2:]),
                       capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-6000:]
    got = json.loads(p.stdout.strip().splitlines()[-1])
    print(got)
    return got


@pytest.mark.parametrize("table", [1, 0], ids=["table", "no_table"])
@pytest.mark.parametrize("canonical", [0, 1], ids=["regular", "canonical"])
@pytest.mark.parametrize("which", ["k31", "k63"])
def test_sums(which, canonical, table, tmp_path):
    got = run_worker([which, canonical], table, tmp_path)
    assert got["ok"] and 1800 <= got["reads"] <= 2200 and got["positive"] > 0
    assert (got["sk_slots"] > 0) == bool(table)
    assert got["kinds"]["backward_steps"] > 0 and got["kinds"]["last_id"] > 0 and got["kinds"]["reads_above_2_16"] == 1


def test_two_minimizer_shards(tmp_path):
    """each shard adds the k-mers it owns: the shards' rows added together are the rows of the whole index; the device call refuses"""
    got = run_worker(["k31", 0, "shards"], 1, tmp_path)
    assert got["ok"] and got["shards"] == 2 and got["positive"] > 0


def test_weighted_round_trip(tmp_path):
    """streaming_depth -> write_weighted_fasta -> Dictionary.build(weighted=True): streaming_sums(reads) equals streaming_sums(reads, depth)"""
    got = run_worker(["k31", 0, "weighted"], 1, tmp_path)
    assert got["ok"] and got["weighted"] and got["positive"] > 0


@pytest.mark.parametrize("which,extra", [("k31", []), ("k63", ["--canonical"])])
def test_cpp_facade_checker(which, extra, tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from gpu_sums_worker import dictionary_input

    fasta, _, k, m = dictionary_input(which, False, str(tmp_path))
    exe = os.path.join(ROOT, "tests", "cpp", "check_sums")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "sshash_amd", "csrc"), "tools"])
    p = subprocess.run([exe, fasta, str(k), str(m)] + extra, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "EVERYTHING OK!" in p.stdout
