"""GPU: the dictionary as a graph -- sshash_string_neighbours_device, sshash_string_links[_device], sshash_kmer_adjacency[_device] and the
GFA writer -- at k = 15, 31, 33 and 63 (m = min(k, 13)), regular then canonical, on the strings of gpu_graph_worker.make_graph: about
9 000 strings (more than two 4096-word tiles of the prefix sum over link_offsets and a partial one) whose links are known by
construction, tests/test_graph_inputs.py asserts on the CPU that they reach every combination of the flags. Per flavour the worker
compares, exactly: string_neighbours_device (ids and range form, every field, one strand) with the host's string_neighbours and the
ground truth; string_links over all strings and over sub-ranges, host and device form, under links_chunk unset, 1, 7, 256 and
num_strings - 1, with the ground truth byte for byte; capacities (counting, exact, exact - 1, half, 1) with sentinels around the
arrays; kmer_adjacency under adjacency_chunk unset, 1, 2047, 2049 and num_kmers - 1 with the ground truth, and its end k-mers with
link_degrees; a minimizer shard (refused) and two table shards (the same links); write_gfa read back. One further worker runs on the
stitched strings of the golden salmonella fixture. Every case is one run of tests/gpu_graph_worker.py in a fresh process with a time
limit of its own.

Measured on an MI355X, the six cases one after the other: 50 s together. The four workers: 16.3 s (k = 15, the first, on a machine that
had not run the library before), 8.3 s (k = 31), 8.3 s (k = 33), 9.1 s (k = 63); of that the strings and the ground truth take 0.5 to
0.7 s, the regular flavour 5.8 to 6.2 s (13.7 s in the first worker: the start of the runtime and the first upload are in it) and the
canonical flavour 1.7 to 2.4 s -- string_links and kmer_adjacency over the whole range in rounds of ONE string or k-mer are among its
calls (about 9 000 and 50 000 rounds, each a lookup of 8 queries). The worker on the salmonella fixture: 2.0 s;
tests/cpp/check_links on it: about 3 s."""
from __future__ import annotations

import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT
from gpu_graph_worker import KS, m_of

_STOPPED = []  # why no further worker is started: one of them faulted, aborted or ran out of time
TIME_LIMIT = 180  # seconds, as tests/test_gpu_idside.py


def run_worker(which, tmp_path):
    assert not _STOPPED, "not started: " + _STOPPED[0]
    env = {name: value for name, value in os.environ.items() if not name.startswith("SSHASH_AMD_")}
    try:
        p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "gpu_graph_worker.py"), str(which), str(tmp_path)], capture_output=True, text=True,
                           timeout=TIME_LIMIT, env=env)
    except subprocess.TimeoutExpired:
        _STOPPED.append(f"the worker of {which} ran into its time limit")
        raise
    if p.returncode < 0 or p.returncode in (134, 139) or "illegal memory access" in p.stderr:  # a signal, an abort, a GPU fault: no further worker
        _STOPPED.append(f"the worker of {which} ended with status {p.returncode}")
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-6000:]
    got = json.loads(p.stdout.strip().splitlines()[-1])
    assert got["ok"]
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("k", KS, ids=[f"k{k}" for k in KS])
def test_graph(k, tmp_path):
    got = run_worker(k, tmp_path)
    print({name: got[name] for name in ("k", "m", "seconds")}, got["dictionaries"])
    assert (got["k"], got["m"]) == (k, m_of(k)) and set(got["dictionaries"]) == {"regular", "canonical"}
    reached = got["reached"]
    assert reached["strings"] > 8192 and 30000 <= reached["kmers"] <= 60000 and reached["combinations"] == list(range(16)), reached
    for flavour, st in got["dictionaries"].items():
        assert st["links"] == reached["links"] and st["gfa_links"] == reached["end_to_end"], (flavour, st)
        assert st["neighbours_found"] > 1000 and st["junctions_inside_strings"] >= 20, (flavour, st)


@pytest.mark.gpu
def test_cpp_facade_links():
    """tests/cpp/check_links.cpp on the stitched strings of the golden fixture: string_links against string_neighbours and full lookups,
    kmer_adjacency against kmer_neighbours on every 97th id"""
    from conftest import SE_FASTA

    assert not _STOPPED, "not started: " + _STOPPED[0]
    exe = os.path.join(ROOT, "tests", "cpp", "check_links")
    if not os.path.exists(exe):  # (as tests/test_iterate.py: host code by g++, linked against the library as it stands)
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "sshash_amd", "csrc"), "-o", "../libsshash_amd.so", "../../tests/cpp/check_links"])
    try:
        p = subprocess.run([exe, SE_FASTA, "31", "13"], capture_output=True, text=True, timeout=TIME_LIMIT)
    except subprocess.TimeoutExpired:
        _STOPPED.append("check_links ran into its time limit")
        raise
    if p.returncode < 0 or p.returncode in (134, 139) or "illegal memory access" in p.stderr:
        _STOPPED.append(f"check_links ended with status {p.returncode}")
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert p.stdout.count("EVERYTHING OK!") == 2, p.stdout


@pytest.mark.gpu
def test_graph_of_stitched_strings(tmp_path):
    got = run_worker("salmonella", tmp_path)
    print(got)
    st = got["salmonella"]
    assert st["strings"] == 647 and st["links"] > 0 and st["junctions_inside_strings"] > 0, st
