"""GPU: the run records over segments (sshash_streaming_runs[_device] once Dictionary.set_read_segments has set an S) and the runs of a
query file (sshash_streaming_runs_from_file). Every case is one run of tests/gpu_runs_segments_worker.py in a fresh process with a time
limit of its own. With segments of S k-mers run_offsets and every record must be byte for byte what the uncut reads give -- against the
run rule over the CPU oracle's per-k-mer results, and against the same calls under SEGMENTS_OFF --: through the host call, and through
the device call at capacity 0, 1, total - 1, total and total + 3 with guard records behind the capacity, into a report that holds values
and with a NULL report. S = 1 makes every k-mer a segment -- tens of thousands of them, so runs cross the shares of waves --; 7 and 64 do
not divide the reads' lengths. The last read of the batch is a long one: the empty entries of the segment table lie behind its
segments. Before it touches the GPU the worker asserts that, for every S, seams fall inside forward and backward runs, on a run's first
k-mer, behind its last, on a negative and on an invalid k-mer, and that a run holds three whole segments. That the run kernel really was
launched over a segment table is read from the counter of read_segments(): it rises by exactly one per segmented device call -- which
is what fails where the runs are not segmented --, by at least one for the host call, and not at all for SEGMENTS_OFF, for
device_calls = 0 and for a minimizer shard. Further cases: one read above 2^16 bases at the default S; a multiline FASTA with a ~3 kb
record and a FASTQ through the file call in batches that seam inside the file; the C++ facade."""
from __future__ import annotations

import json
import os
import subprocess
import sys

import pytest

from conftest import K63_FASTA, ROOT, SE_FASTA

pytestmark = pytest.mark.gpu

DICTIONARIES = [(SE_FASTA, 31, 13), (K63_FASTA, 63, 25)]


def run_worker(args, table, tmp_path, limit=60):
    """`limit`: the case's time limit in seconds. A case takes a few seconds, most of them the build of its dictionary, the oracle and the
    start of the process; the cases that walk a 70,000-base read with one lane get twice the limit."""
    env = dict(os.environ)
    env.pop("SSHASH_AMD_TEST_HOOKS", None)
    if table:
        env.pop("SSHASH_AMD_SKTABLE", None)
    else:
        env["SSHASH_AMD_SKTABLE"] = "0"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "gpu_runs_segments_worker.py")] + [str(a) for a in args[:4]] + [str(tmp_path)] +
                       [str(a) for a in args[4:]], capture_output=True, text=True, timeout=limit, env=env)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-6000:]
    got = json.loads(p.stdout.strip().splitlines()[-1])
    print(got)
    return got


@pytest.mark.parametrize("S", [1, 2, 7, 64])
@pytest.mark.parametrize("table", [1, 0], ids=["table", "no_table"])
@pytest.mark.parametrize("canonical", [0, 1], ids=["regular", "canonical"])
@pytest.mark.parametrize("fasta,k,m", DICTIONARIES, ids=["k31", "k63"])
def test_runs_over_segments(fasta, k, m, canonical, table, S, tmp_path):
    got = run_worker([fasta, k, m, canonical, "segments", S], table, tmp_path)
    assert got["ok"] and got["S"] == S and got["segmented_launches"] > 0 and got["seams_in_runs"] > 0 and got["runs"] > 100
    assert (got["sk_slots"] > 0) == bool(table)


@pytest.mark.parametrize("table", [1, 0], ids=["table", "no_table"])
@pytest.mark.parametrize("fasta,k,m,canonical", [(SE_FASTA, 31, 13, 0), (K63_FASTA, 63, 25, 1)], ids=["k31_regular", "k63_canonical"])
def test_one_long_read_at_the_default_s(fasta, k, m, canonical, table, tmp_path):
    got = run_worker([fasta, k, m, canonical, "long"], table, tmp_path, limit=120)
    assert got["ok"] and got["bases"] > (1 << 16) and got["segmented_launches"] > 0


@pytest.mark.parametrize("fasta,k,m,canonical", [(SE_FASTA, 31, 13, 1), (K63_FASTA, 63, 25, 0)], ids=["k31_canonical", "k63_regular"])
def test_the_runs_of_a_query_file(fasta, k, m, canonical, tmp_path):
    got = run_worker([fasta, k, m, canonical, "file"], 1, tmp_path)
    assert got["ok"] and got["segmented_launches"] > 0 and got["runs"]["fasta"] > 0 and got["runs"]["fastq"] > 0


def test_where_the_counter_does_not_move(tmp_path):
    got = run_worker([SE_FASTA, 31, 13, 0, "counters"], 1, tmp_path, limit=120)
    assert got["ok"] and got["segmented_launches"] > 0 and got["shard_runs"] > 0


@pytest.mark.parametrize("fasta,k,m,extra", [(SE_FASTA, 31, 13, []), (K63_FASTA, 63, 21, ["--canonical"])])
def test_cpp_facade_checker(fasta, k, m, extra):
    exe = os.path.join(ROOT, "tests", "cpp", "check_runs_segments")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "sshash_amd", "csrc"), "tools"])
    p = subprocess.run([exe, fasta, str(k), str(m)] + extra, capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "EVERYTHING OK!" in p.stdout
