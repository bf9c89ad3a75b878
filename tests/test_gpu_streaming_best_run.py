"""GPU: the streaming anchors -- per read, its longest run. Every case is one run of tests/gpu_best_run_worker.py in a fresh process with a
time limit of its own (the environment switch that decides whether a replica holds the super-k-mer table is read once per process). The
worker checks, with byte equality of the 32-byte records, against the CPU oracle's point lookups of every k-mer of every read, cut into
runs by the header's rule in numpy and reduced by the argmax with the tie rule, and against sshash_amd.runs_best over streaming_runs:
the device call into records that held garbage between guard records, with a report and without one, with total_bases given and with
0; the six counters against streaming_query's; the host call on all reads, the read above 2^16 bases included; the host call under the
hooks stream_piece_reads and stream_move_out_every; both calls with segments of 7 k-mers set, which must change nothing and count no
segmented launch; the file call on a FASTA and a FASTQ written from the reads; runs_best_device against runs_best on the device call's
own CSR and on the CSR made by hand of the CPU test. Before it touches the GPU it asserts from the oracle that the reads hold ties for
longest, longest runs that are not the first, backward ones, a best run of 2^15 k-mers or more, hitless reads, reads shorter than k and
exactly one read above 2^16 bases. One more worker: two minimizer shards, whose device, host and file calls refuse."""
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
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "gpu_best_run_worker.py")] + [str(a) for a in args[:2]] + [str(tmp_path)] + list(args[2:]),
                       capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-6000:]
    got = json.loads(p.stdout.strip().splitlines()[-1])
    print(got)
    return got


@pytest.mark.parametrize("table", [1, 0], ids=["table", "no_table"])
@pytest.mark.parametrize("canonical", [0, 1], ids=["regular", "canonical"])
@pytest.mark.parametrize("which", ["k31", "k63"])
def test_best_run(which, canonical, table, tmp_path):
    got = run_worker([which, canonical], table, tmp_path)
    assert got["ok"] and 1800 <= got["reads"] <= 2400 and got["runs"] > 0 and got["longest"] >= 1 << 15
    assert (got["sk_slots"] > 0) == bool(table)
    kinds = got["kinds"]
    assert kinds["ties_for_longest"] >= 20 and kinds["longest_is_not_the_first"] > 0 and kinds["longest_is_backward"] > 0
    assert kinds["best_of_2_15_or_more"] > 0 and kinds["hitless_reads"] > 0 and kinds["reads_shorter_than_k"] > 0 and kinds["reads_above_2_16"] == 1
    assert kinds["three_runs_of_one_string"] > 0


def test_two_minimizer_shards_refuse(tmp_path):
    """a shard's longest runs are not the whole index's: the device, host and file calls are SSHASH_ERR_ARGUMENT and say where to go"""
    got = run_worker(["k31", 0, "shards"], 1, tmp_path)
    assert got["ok"] and got["shards"] == 2 and got["refused"] == 8


@pytest.mark.parametrize("which,extra", [("k31", []), ("k63", ["--canonical"])])
def test_cpp_facade_checker(which, extra, tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from gpu_sums_worker import dictionary_input

    fasta, _, k, m = dictionary_input(which, False, str(tmp_path))
    exe = os.path.join(ROOT, "tests", "cpp", "check_best_run")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "sshash_amd", "csrc"), "tools"])
    p = subprocess.run([exe, fasta, str(k), str(m)] + extra, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "EVERYTHING OK!" in p.stdout
