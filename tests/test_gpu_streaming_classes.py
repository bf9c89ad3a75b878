"""GPU: the streaming classes -- per read, its positive k-mers by class of string. Every case is one run of tests/gpu_classes_worker.py in
a fresh process with a time limit of its own (the environment switch that decides whether a replica holds the super-k-mer table is read
once per process). The worker checks, with exact integer equality, against numpy.add.at over labels[string_id] of the valid places,
computed twice -- from streaming_lookup's per-k-mer string_id and from the CPU oracle's point lookups of every k-mer of every read --:
1, 3, 64, 65 and 4096 classes (at 4096 the first 64 reads); labels string_id % C, all strings in one class (the column is column 1 of
streaming_query_per_read) and random labels a third of which are no class (the rows sum to no more than the positive k-mers and equal
the masked truth); the device, host and file entry points row for row; rows that held garbage overwritten, hitless reads included; guard
words on both sides of the rows, which lie at an address that is a multiple of 4 and not of 8; the six counters against
streaming_query's; identical rows under the hooks stream_piece_reads and stream_move_out_every, with the cap on a piece's reads in force
(4096 classes and more reads than a piece holds), with the reads cut into segments of 1, 7 and 64 k-mers through the device and the host
call, the read above 2^16 bases at the default S and, with segments off, through the per-k-mer route; class_best_device and
class_totals_device against their host variants and numpy on all those rows and on rows made to tie. Before it touches the GPU it
asserts from the oracle that some read hits two strings of different classes, some read two strings of one class, and some read only a
string that is in no class. One more worker: two minimizer shards, whose rows added are the whole index's and whose device call refuses."""
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
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "gpu_classes_worker.py")] + [str(a) for a in args[:2]] + [str(tmp_path)] + list(args[2:]),
                       capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-6000:]
    got = json.loads(p.stdout.strip().splitlines()[-1])
    print(got)
    return got


@pytest.mark.parametrize("table", [1, 0], ids=["table", "no_table"])
@pytest.mark.parametrize("canonical", [0, 1], ids=["regular", "canonical"])
@pytest.mark.parametrize("which", ["k31", "k63"])
def test_classes(which, canonical, table, tmp_path):
    got = run_worker([which, canonical], table, tmp_path)
    assert got["ok"] and 1800 <= got["reads"] <= 2300 and 0 < got["counted"] <= got["positive"]
    assert (got["sk_slots"] > 0) == bool(table)
    kinds = got["kinds"]
    assert kinds["two_strings_of_different_classes"] > 0 and kinds["two_strings_of_the_same_class"] > 0 and kinds["reads_above_2_16"] == 1
    assert all(kinds[f"hits_only_in_no_class_{C}"] > 0 for C in (1, 3, 64, 65, 4096))


def test_two_minimizer_shards(tmp_path):
    """each shard counts the k-mers it owns: the shards' rows added together are the rows of the whole index; the device call refuses"""
    got = run_worker(["k31", 0, "shards"], 1, tmp_path)
    assert got["ok"] and got["shards"] == 2 and 0 < got["counted"] <= got["positive"]


@pytest.mark.parametrize("which,extra", [("k31", []), ("k63", ["--canonical"])])
def test_cpp_facade_checker(which, extra, tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from gpu_sums_worker import dictionary_input

    fasta, _, k, m = dictionary_input(which, False, str(tmp_path))
    exe = os.path.join(ROOT, "tests", "cpp", "check_classes")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "sshash_amd", "csrc"), "tools"])
    p = subprocess.run([exe, fasta, str(k), str(m)] + extra, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "EVERYTHING OK!" in p.stdout
