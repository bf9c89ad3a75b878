"""GPU: the streaming depth -- how often a read set holds each k-mer of the dictionary, num_kmers words of uint32. Every case is one run
of tests/gpu_depth_worker.py in a fresh process with a time limit of its own (the environment switch that decides whether a replica
holds the super-k-mer table is read once per process). The worker checks, against numpy.bincount over streaming_lookup's kmer_id values
and over the CPU oracle's point lookups of every k-mer of every read: the host, the device (deltas, then the finish in place and out of
place, at addresses that are and are not multiples of 16) and the file entry points word for word; (depth != 0) against the bits of
streaming_cover; depth.sum() against num_positive_kmers; the six counters against streaming_query's; accumulation (two batches into one
array, a host array that held values); guard words around every device array; identical results under the hooks stream_piece_reads and
stream_move_out_every; a read above 2^16 bases against the same bases in short reads; the finish alone on deltas of its own (a wrap, +1
in the first word and -1 in the last, random words against numpy.cumsum); depth_string_sums_device against the host function. Before it
touches the GPU it asserts from the oracle's ids that every kind of read and of run the kernel has a branch for is present (backward
runs, runs of one, of 64 and more, from id 0, to the last id, N, short, empty and hitless reads, substitutions that cut runs, one read
4096 times) and that the expected array holds zeros, ones and values of two and more."""
from __future__ import annotations

import json
import os
import subprocess
import sys

import pytest

from conftest import GOLDEN, K63_FASTA, ROOT, SE_FASTA

pytestmark = pytest.mark.gpu

K47_FASTA = os.path.join(GOLDEN, "se.ust.k47.fa.gz")
# (the last number: the rounds of 256 tile sums the middle launch of the finish makes over the dictionary's k-mers, 4096 a tile. The k = 31
# and k = 47 files hold 4.8 and 4.9 million k-mers: five rounds; the k = 63 file holds 806,471: one.)
DICTIONARIES = [(SE_FASTA, 31, 13, 5), (K47_FASTA, 47, 21, 5), (K63_FASTA, 63, 25, 1)]


def run_worker(args, table, tmp_path):
    env = dict(os.environ)
    env.pop("SSHASH_AMD_TEST_HOOKS", None)
    if table:
        env.pop("SSHASH_AMD_SKTABLE", None)
    else:
        env["SSHASH_AMD_SKTABLE"] = "0"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "gpu_depth_worker.py")] + [str(a) for a in args[:4]] + [str(tmp_path)] + list(args[4:]),
                       capture_output=True, text=True, timeout=600, env=env)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-6000:]
    got = json.loads(p.stdout.strip().splitlines()[-1])
    print(got)
    return got


@pytest.mark.parametrize("table", [1, 0], ids=["table", "no_table"])
@pytest.mark.parametrize("canonical", [0, 1], ids=["regular", "canonical"])
@pytest.mark.parametrize("fasta,k,m,finish_rounds", DICTIONARIES, ids=["k31", "k47", "k63"])
def test_depth(fasta, k, m, finish_rounds, canonical, table, tmp_path):
    got = run_worker([fasta, k, m, canonical], table, tmp_path)
    assert got["ok"] and 0 < got["held"] < got["num_kmers"] and got["held"] < got["positive"]
    assert (got["sk_slots"] > 0) == bool(table)
    assert got["finish_rounds"] == finish_rounds
    assert got["kinds"]["backward"] > 0 and got["kinds"]["runs_of_64_and_more"] > 0 and got["kinds"]["runs_to_the_last_id"] > 0


def test_two_minimizer_shards(tmp_path):
    """each shard counts the k-mers it owns under the ids of the whole index: the shards' arrays added are the whole index's"""
    got = run_worker([SE_FASTA, 31, 13, 0, "shards"], 1, tmp_path)
    assert got["ok"] and got["shards"] == 2 and got["positive"] > 0


@pytest.mark.parametrize("fasta,k,m,extra", [(SE_FASTA, 31, 13, []), (K63_FASTA, 63, 21, ["--canonical"])])
def test_cpp_facade_checker(fasta, k, m, extra):
    exe = os.path.join(ROOT, "tests", "cpp", "check_depth")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "sshash_amd", "csrc"), "tools"])
    p = subprocess.run([exe, fasta, str(k), str(m)] + extra, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "EVERYTHING OK!" in p.stdout
