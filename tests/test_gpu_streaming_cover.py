"""GPU: the streaming cover -- which k-mers of the dictionary a read set holds, as a bitmap over the k-mer ids. Every case is one run
of tests/gpu_cover_worker.py in a fresh process with a time limit of its own (the environment switch that decides whether a replica
holds the super-k-mer table is read once per process). The worker checks, against the bitmap built in numpy from streaming_lookup's
kmer_id values and against the CPU oracle's point lookups of every k-mer of every read: the host, the device and the file entry points
word for word; the bitmap of streaming_runs + expand_runs; the report against streaming_query's; accumulation (bits set before survive,
two batches give the union), a guard word behind the bitmap, the bits at or above num_kmers; byte-identical bitmaps under the hooks
stream_piece_reads and stream_move_out_every; a read above 2^16 bases against the same bases in short reads; a FASTQ and a FASTA file
against their parsed reads; cover_string_counts_device against the host function and the popcount. It asserts that every kind of read
and of run the kernel has a branch for is present (backward runs, runs of one, of 64 and more, inside one word, id 0 and the last id,
N, short, empty and hitless reads, one read 4096 times, substitutions that cut runs) and that the expected bitmap has set and clear
bits."""
from __future__ import annotations

import json
import os
import subprocess
import sys

import pytest

from conftest import GOLDEN, K63_FASTA, ROOT, SE_FASTA

pytestmark = pytest.mark.gpu

K47_FASTA = os.path.join(GOLDEN, "se.ust.k47.fa.gz")
DICTIONARIES = [(SE_FASTA, 31, 13), (K47_FASTA, 47, 21), (K63_FASTA, 63, 25)]


@pytest.mark.parametrize("table", [1, 0], ids=["table", "no_table"])
@pytest.mark.parametrize("canonical", [0, 1], ids=["regular", "canonical"])
@pytest.mark.parametrize("fasta,k,m", DICTIONARIES, ids=["k31", "k47", "k63"])
def test_cover(fasta, k, m, canonical, table, tmp_path):
    env = dict(os.environ)
    env.pop("SSHASH_AMD_TEST_HOOKS", None)
    if table:
        env.pop("SSHASH_AMD_SKTABLE", None)
    else:
        env["SSHASH_AMD_SKTABLE"] = "0"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "gpu_cover_worker.py"), fasta, str(k), str(m), str(canonical), str(tmp_path)],
                       capture_output=True, text=True, timeout=900, env=env)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-6000:]
    got = json.loads(p.stdout.strip().splitlines()[-1])
    print(got)
    assert got["ok"] and 0 < got["covered"] < got["num_kmers"]
    assert (got["sk_slots"] > 0) == bool(table)
    assert got["kinds"]["backward"] > 0 and got["kinds"]["runs_of_64_and_more"] > 0


@pytest.mark.parametrize("fasta,k,m,extra", [(SE_FASTA, 31, 13, []), (K63_FASTA, 63, 21, ["--canonical"])])
def test_cpp_facade_checker(fasta, k, m, extra):
    exe = os.path.join(ROOT, "tests", "cpp", "check_cover")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "sshash_amd", "csrc"), "tools"])
    p = subprocess.run([exe, fasta, str(k), str(m)] + extra, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "EVERYTHING OK!" in p.stdout
