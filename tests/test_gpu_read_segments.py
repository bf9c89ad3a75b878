"""GPU: long reads cut into segments for the run kernel (Dictionary.set_read_segments). Every case is one run of
tests/gpu_segments_worker.py in a fresh process with a time limit of its own. With segments of S k-mers the six counters, every per-read
row, the cover bitmap and the finished depth array must be word for word what the uncut reads give -- through the host calls, and with
device_calls through the device calls: against the CPU oracle's state machine over the whole reads, and against the same calls under
SEGMENTS_OFF; with a NULL report for cover and depth, into a report, a bitmap and deltas that already hold values, with guard rows around
the device rows, and under the hooks stream_piece_reads and stream_move_out_every. S = 1 makes every k-mer a segment; 7 and 64 do not
divide the reads' lengths. Before it touches the GPU the worker asserts that, for every S, seams fall inside forward and backward runs,
on a run's first k-mer, behind its last, on a negative and on an invalid k-mer. That the run kernel really was launched over a segment
table is read from the counter of read_segments() -- and that it was NOT for SEGMENTS_OFF, for device_calls = 0 and for a minimizer
shard. Further cases: one read of ~70,000 bases at the default S; a multiline FASTA with a ~3 kb record through the four file calls; two
minimizer shards; the C++ facade."""
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
    """`limit`: the case's time limit in seconds. A case takes about six seconds, most of them the build of its dictionary and the start of
    the process; the cases that build two shards or walk a 70,000-base read with one lane get twice the limit."""
    env = dict(os.environ)
    env.pop("SSHASH_AMD_TEST_HOOKS", None)
    if table:
        env.pop("SSHASH_AMD_SKTABLE", None)
    else:
        env["SSHASH_AMD_SKTABLE"] = "0"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "gpu_segments_worker.py")] + [str(a) for a in args[:4]] + [str(tmp_path)] +
                       [str(a) for a in args[4:]], capture_output=True, text=True, timeout=limit, env=env)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-6000:]
    got = json.loads(p.stdout.strip().splitlines()[-1])
    print(got)
    return got


@pytest.mark.parametrize("S", [1, 2, 7, 64])
@pytest.mark.parametrize("table", [1, 0], ids=["table", "no_table"])
@pytest.mark.parametrize("canonical", [0, 1], ids=["regular", "canonical"])
@pytest.mark.parametrize("fasta,k,m", DICTIONARIES, ids=["k31", "k63"])
def test_segments(fasta, k, m, canonical, table, S, tmp_path):
    got = run_worker([fasta, k, m, canonical, "segments", S], table, tmp_path)
    assert got["ok"] and got["S"] == S and got["segmented_launches"] > 0 and got["seams_in_runs"] > 0
    assert (got["sk_slots"] > 0) == bool(table)
    assert got["totals"][4] > 0 and got["totals"][5] > got["totals"][4]


@pytest.mark.parametrize("table", [1, 0], ids=["table", "no_table"])
@pytest.mark.parametrize("fasta,k,m,canonical", [(SE_FASTA, 31, 13, 0), (K63_FASTA, 63, 25, 1)], ids=["k31_regular", "k63_canonical"])
def test_one_long_read_at_the_default_s(fasta, k, m, canonical, table, tmp_path):
    got = run_worker([fasta, k, m, canonical, "long"], table, tmp_path, limit=120)
    assert got["ok"] and got["bases"] > (1 << 16) and got["segmented_launches"] > 0


@pytest.mark.parametrize("fasta,k,m,canonical", [(SE_FASTA, 31, 13, 1), (K63_FASTA, 63, 25, 0)], ids=["k31_canonical", "k63_regular"])
def test_multiline_fasta_through_the_file_calls(fasta, k, m, canonical, tmp_path):
    got = run_worker([fasta, k, m, canonical, "file"], 1, tmp_path)
    assert got["ok"] and got["segmented_launches"] == 4


def test_two_minimizer_shards_do_not_segment(tmp_path):
    got = run_worker([SE_FASTA, 31, 13, 0, "shards"], 1, tmp_path, limit=120)
    assert got["ok"] and got["shards"] == 2 and all(p > 0 for p in got["positive"])


def test_device_calls_off_leaves_the_device_calls_alone(tmp_path):
    got = run_worker([SE_FASTA, 31, 13, 0, "device_off"], 1, tmp_path)
    assert got["ok"] and got["segmented_launches"] > 0


@pytest.mark.parametrize("fasta,k,m,extra", [(SE_FASTA, 31, 13, []), (K63_FASTA, 63, 21, ["--canonical"])])
def test_cpp_facade_checker(fasta, k, m, extra):
    exe = os.path.join(ROOT, "tests", "cpp", "check_segments")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "sshash_amd", "csrc"), "tools"])
    p = subprocess.run([exe, fasta, str(k), str(m)] + extra, capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "EVERYTHING OK!" in p.stdout
