"""GPU: the streaming runs -- for every read, one record per search and the extensions behind it (string, offset in it, orientation,
length, position in the read). Expected records: the oracle's per-k-mer streaming results of every read on its own
(oracle.streaming_read), grouped by the rule of include/sshash_amd.h (gpu_runs_worker.runs_of_results); compared for exact equality of
run_offsets and of every field of every record, through the host and the device entry point."""
from __future__ import annotations

import json
import os
import subprocess
import sys

import numpy as np
import pytest

import sshash_amd
from conftest import K63_FASTA, ROOT, SE_FASTA
from gpu_runs_worker import (BACKWARD, RUN_DTYPE, check_both, chimeras, device_runs, genome_reads, oracle_runs, random_dna, read_genome, revcomp,
                             same_records, synthetic_reads)

pytestmark = pytest.mark.gpu

SEVEN = ["case_se_regular", "case_se_canonical", "case_skew_regular", "case_skew_canonical", "case_k63_canonical", "case_k63_regular",
         "case_small_k"]
_cache = {}
_genome = []


def genome():
    if not _genome:
        _genome.append(read_genome())
    return _genome[0]


def _expected(case, name, make):
    """(reads, run_offsets, records) of one read set of one dictionary, made once"""
    key = (case.name, name)
    if key not in _cache:
        reads = make()
        _cache[key] = (reads,) + oracle_runs(case.oracle, reads)
    return _cache[key]


def set_one(case):
    return _expected(case, "synthetic", lambda: synthetic_reads(case.sequences, case.k, 3000, seed=17))


def set_two(case):
    return _expected(case, "genome", lambda: genome_reads(genome(), 1500, 300, seed=3))


def set_three(case):
    return _expected(case, "chimeras", lambda: chimeras(case.sequences, case.k, 1000, 5 if case.k == 31 else 7))


def lengths_of(records):
    return (records["num_kmers"] & 0x7FFFFFFF).astype(np.uint64)


def report_row(rep):
    return [rep.num_kmers, rep.num_positive_kmers, rep.num_negative_kmers, rep.num_invalid_kmers, rep.num_searches, rep.num_extensions]


def round_trip(d, case, reads, run_offsets, runs):
    """expand_runs gives the per-k-mer results of the streaming lookup back: two device paths that share nothing beyond the index"""
    per_read, _ = d.streaming_lookup(reads, full=True)
    back = sshash_amd.expand_runs(run_offsets, runs, [len(r) for r in reads], case.k)
    for i, (a, b) in enumerate(zip(back, per_read)):
        for field in ("kmer_id", "string_id", "kmer_id_in_string"):
            assert (getattr(a, field) == getattr(b, field)).all(), (i, field, reads[i][:80])
        # the orientation of every k-mer that has one to speak of: the lookup reports the strand of its LAST PROBE for a negative k-mer
        # (-1 in a regular dictionary, whose second probe is the reverse complement's), which no run carries -- expand_runs says +1 there
        positive = b.kmer_id != sshash_amd.INVALID_U64
        assert (a.kmer_orientation[positive] == b.kmer_orientation[positive]).all(), (i, "kmer_orientation", reads[i][:80])
        assert (a.kmer_orientation[~positive] == 1).all(), (i, "kmer_orientation outside the runs", reads[i][:80])


@pytest.mark.parametrize("case_name", SEVEN)
def test_runs_of_synthetic_reads(case_name, request):
    case = request.getfixturevalue(case_name)
    d = case.dict.to_device(0)
    reads, want_offsets, want_runs = set_one(case)
    per_read = np.diff(want_offsets)
    assert (per_read > 0).sum() >= 0.2 * len(reads) and (per_read == 0).sum() >= 100 and (lengths_of(want_runs) > 1).sum() >= 100
    report = check_both(d, reads, want_offsets, want_runs)
    assert report.num_searches == int(want_offsets[-1]) and report.num_positive_kmers == int(lengths_of(want_runs).sum())
    round_trip(d, case, reads, want_offsets, want_runs)


@pytest.mark.parametrize("case_name", ["case_se_regular", "case_se_canonical"])
def test_reads_that_cross_unitig_boundaries(case_name, request):
    """reads cut from the genome the strings were made from: positive k-mers follow each other in DIFFERENT runs"""
    case = request.getfixturevalue(case_name)
    d = case.dict.to_device(0)
    reads, want_offsets, want_runs = set_two(case)
    per_read = np.diff(want_offsets).astype(np.int64)
    backward = (want_runs["num_kmers"] & BACKWARD) != 0
    adjacent = same_string = both = 0
    for r in range(len(reads)):
        mine = want_runs[int(want_offsets[r]):int(want_offsets[r + 1])]
        ends = mine["read_pos"].astype(np.int64) + lengths_of(mine).astype(np.int64)
        touch = ends[:-1] == mine["read_pos"][1:].astype(np.int64)
        adjacent += int(touch.sum())
        same_string += int((touch & (mine["string_id"][:-1] == mine["string_id"][1:])).sum())
        flags = (mine["num_kmers"] & BACKWARD) != 0
        both += int(flags.any() and not flags.all())
    print("reads with >= 2 runs", (per_read >= 2).mean(), "adjacent", adjacent, "in one string", same_string, "forward", int((~backward).sum()),
          "backward", int(backward.sum()), "both orientations", both, "most runs", int(per_read.max()))
    assert (per_read >= 2).mean() >= 0.35
    assert adjacent >= 100 and same_string >= 1
    assert (~backward).sum() >= 1000 and backward.sum() >= 1000
    assert both >= 15
    assert per_read.max() >= 10
    check_both(d, reads, want_offsets, want_runs)
    round_trip(d, case, reads, want_offsets, want_runs)


@pytest.mark.parametrize("case_name", ["case_se_regular", "case_se_canonical", "case_k63_regular"])
def test_chimeras(case_name, request):
    case = request.getfixturevalue(case_name)
    d = case.dict.to_device(0)
    reads, want_offsets, want_runs = set_three(case)
    per_read = np.diff(want_offsets).astype(np.int64)
    both = strings = 0
    for r in range(len(reads)):
        mine = want_runs[int(want_offsets[r]):int(want_offsets[r + 1])]
        flags = (mine["num_kmers"] & BACKWARD) != 0
        both += int(flags.any() and not flags.all())
        strings += int(len(set(mine["string_id"].tolist())) >= 2)
    print("fewest runs", int(per_read.min()), "both orientations", both, ">= 2 strings", strings, "runs of one", int((lengths_of(want_runs) == 1).sum()))
    assert per_read.min() >= 2
    assert both >= 0.5 * len(reads)
    assert strings >= 0.95 * len(reads)
    assert (lengths_of(want_runs) == 1).sum() >= 20
    check_both(d, reads, want_offsets, want_runs)
    round_trip(d, case, reads, want_offsets, want_runs)


def _hand_made_reads(case):
    """one substitution at every distance from either end, runs starting at every alignment of the strings' words, whole strings, off
    a string's end into random bases and back, an N next to a substitution (the reads of test_rows_of_hand_made_reads, regenerated)"""
    k = case.k
    rng = np.random.default_rng(11)
    long_seqs = sorted((s for s in case.sequences if len(s) >= 4 * k + 400), key=len)
    s = long_seqs[len(long_seqs) // 2]
    reads = []
    L = 2 * k + 40
    for where in range(0, L):
        r = list(s[37:37 + L])
        r[where] = "ACGT"[("ACGT".index(r[where]) + 1 + where % 3) % 4]
        reads.append("".join(r))
        reads.append(revcomp("".join(r)))
    for a in (0, 1, 31, 32, 33, 63, 64, 65, 95, 96):
        reads.append(s[a:a + 3 * k + 70])
        reads.append(revcomp(s[a:a + 3 * k + 70]))
    reads.append(s)
    reads.append(revcomp(s))
    tail = "".join(rng.choice(list("ACGT"), size=k + 20))
    reads.append(s[-(k + 50):] + tail)
    reads.append(revcomp(s[-(k + 50):] + tail))
    reads.append(tail + s[:k + 50])
    for gap in (1, 2, k - 1, k, k + 1):
        r = list(s[100:100 + 3 * k])
        r[k + 5] = "N"
        r[k + 5 + gap] = "ACGT"[("ACGT".index(r[k + 5 + gap]) + 2) % 4]
        reads.append("".join(r))
    return reads


@pytest.mark.parametrize("case_name", ["case_se_regular", "case_se_canonical", "case_k63_regular"])
def test_runs_of_hand_made_reads(case_name, request):
    case = request.getfixturevalue(case_name)
    d = case.dict.to_device(0)
    reads = _hand_made_reads(case)
    want_offsets, want_runs = oracle_runs(case.oracle, reads)
    assert int(want_offsets[-1]) > len(reads) and (lengths_of(want_runs) == 1).any() and (lengths_of(want_runs) > case.k).any()
    check_both(d, reads, want_offsets, want_runs)


@pytest.mark.parametrize("case_name", ["case_se_regular", "case_se_canonical"])
def test_capacity(case_name, request):
    """run_offsets is complete and exact whatever the capacity; record i is written iff i < runs_capacity; nothing else is touched"""
    case = request.getfixturevalue(case_name)
    d = case.dict.to_device(0)
    reads, want_offsets, want_runs = set_two(case)
    total = int(want_offsets[-1])
    for capacity in (0, 1, total - 1, total, total + 7):
        ro, buf, _ = device_runs(d, reads, capacity=capacity, tail=64, sentinel=0xC3)
        assert (ro == want_offsets).all(), capacity
        n = min(capacity, total)
        assert len(buf) == capacity + 64
        assert same_records(buf[:n], want_runs[:n]), capacity
        assert (buf[n:].view(np.uint8) == 0xC3).all(), capacity
        # the host call: the same rule on a host buffer
        host_ro = np.full(len(reads) + 1, 5, dtype=np.uint64)
        host_buf = np.full((capacity + 64) * 32, 0xC3, dtype=np.uint8)
        blob = np.frombuffer("".join(reads).encode(), dtype=np.uint8)
        offsets = np.zeros(len(reads) + 1, dtype=np.uint64)
        offsets[1:] = np.cumsum([len(r) for r in reads])
        from sshash_amd import _binding as B

        assert B._load().sshash_streaming_runs(d._h, blob.ctypes.data, offsets.ctypes.data, len(reads), host_ro.ctypes.data,
                                               host_buf.ctypes.data if capacity else None, capacity, None) == 0
        assert (host_ro == want_offsets).all(), capacity
        assert same_records(host_buf.view(RUN_DTYPE)[:n], want_runs[:n]) and (host_buf[n * 32:] == 0xC3).all(), capacity


@pytest.mark.parametrize("case_name", ["case_se_regular", "case_k63_canonical"])
def test_accounting(case_name, request, monkeypatch):
    """per read: runs = num_searches, k-mers in runs = num_positive_kmers of the per-read rows; the report is streaming_query's and is
    accumulated into; two launches are byte-identical; when the counters move out changes nothing; a stream of the caller's"""
    import torch

    case = request.getfixturevalue(case_name)
    d = case.dict.to_device(0)
    reads, want_offsets, want_runs = set_one(case)
    rows, _ = d.streaming_query_per_read(reads)
    total_report = np.array(report_row(d.streaming_query(reads)), dtype=np.uint64)
    ro, runs, report = d.streaming_runs(reads)
    assert (np.diff(ro) == rows[:, 4]).all()
    sums = np.zeros(len(reads), dtype=np.uint64)
    np.add.at(sums, np.repeat(np.arange(len(reads)), np.diff(ro).astype(np.int64)), lengths_of(runs))
    assert (sums == rows[:, 1]).all()
    assert report_row(report) == total_report.tolist()
    total = int(want_offsets[-1])
    side = torch.cuda.Stream(device=0)
    dro, druns, rep = device_runs(d, reads, capacity=total, report=[1, 2, 3, 4, 5, 6], launches=2, stream=side)
    assert (dro == want_offsets).all() and same_records(druns[:total], want_runs)
    assert (rep == 2 * total_report + np.arange(1, 7, dtype=np.uint64)).all()
    dro, druns, rep = device_runs(d, reads, capacity=total, report=[0] * 6, total_bases=0)  # total_bases not known to the caller
    assert (dro == want_offsets).all() and same_records(druns[:total], want_runs) and (rep == total_report).all()
    for at in ("1", "7", "300"):
        monkeypatch.setenv("SSHASH_AMD_TEST_HOOKS", "stream_move_out_every=" + at)
        rep = check_both(d, reads, want_offsets, want_runs, at)
        assert report_row(rep) == total_report.tolist(), at
        _, _, rep = device_runs(d, reads, capacity=total, report=[0] * 6)
        assert (rep == total_report).all(), at
    monkeypatch.delenv("SSHASH_AMD_TEST_HOOKS")
    # across pieces: the host call cuts its batch, a piece's offsets are local until they are stitched
    for piece in ("300", "257"):
        monkeypatch.setenv("SSHASH_AMD_TEST_HOOKS", "stream_piece_reads=" + piece)
        ro, runs, report = d.streaming_runs(reads)
        assert (ro == want_offsets).all() and same_records(runs, want_runs) and report_row(report) == total_report.tolist(), piece
    # five pieces of four reads, the third without a base: nothing is launched for it, its reads have no run and the stitching goes on behind it
    with_runs = [i for i in range(len(reads)) if want_offsets[i + 1] > want_offsets[i]][:16]
    batch = [reads[i] for i in with_runs[:8]] + [""] * 4 + [reads[i] for i in with_runs[8:]]
    batch_offsets, batch_runs = oracle_runs(case.oracle, batch)
    assert len(with_runs) == 16 and (np.diff(batch_offsets)[8:12] == 0).all() and batch_offsets[8] > 0 and batch_offsets[-1] > batch_offsets[12]
    monkeypatch.setenv("SSHASH_AMD_TEST_HOOKS", "stream_piece_reads=4")
    ro, runs, report = d.streaming_runs(batch)
    assert (ro == batch_offsets).all() and same_records(runs, batch_runs) and report == d.streaming_query(batch), "a piece of reads without a base"
    monkeypatch.delenv("SSHASH_AMD_TEST_HOOKS")
    # reads without any base, and no reads at all
    dro, druns, rep = device_runs(d, ["", "", ""], capacity=4, report=[1] * 6, total_bases=0)
    assert (dro == 0).all() and (druns.view(np.uint8) == 0x5A).all() and (rep == 1).all()
    d.streaming_runs_device(0, 0, 0, 0, 0, 0, 0)
    zero = torch.full((1,), -1, dtype=torch.int64, device="cuda:0")
    d.streaming_runs_device(0, 0, 0, 0, zero.data_ptr(), 0, 0)
    torch.cuda.synchronize()
    assert int(zero.item()) == 0


@pytest.mark.parametrize("case_name", ["case_se_regular", "case_se_canonical"])
def test_a_read_too_long_for_one_lane(case_name, request):
    """the host call sends a piece that holds a read above 2^16 bases through the position-parallel pipeline and the compaction behind
    it: the same records"""
    case = request.getfixturevalue(case_name)
    d = case.dict.to_device(0)
    g = genome()
    long_read = g[1234567:1234567 + 70000]
    shorts = genome_reads(g, 40, 300, seed=8) + synthetic_reads(case.sequences, case.k, 40, seed=3)
    reads = shorts[:30] + [long_read] + shorts[30:60] + ["", revcomp(long_read)] + shorts[60:]
    want_offsets, want_runs = oracle_runs(case.oracle, reads)
    assert int(want_offsets[31] - want_offsets[30]) >= 2 and int(want_offsets[63] - want_offsets[62]) >= 2 and int(lengths_of(want_runs).max()) > (1 << 15)
    ro, runs, report = d.streaming_runs(reads)
    assert (ro == want_offsets).all(), np.flatnonzero(ro != want_offsets)[:10]
    assert same_records(runs, want_runs), [i for i in range(len(runs)) if runs[i] != want_runs[i]][:5]
    assert report == d.streaming_query(reads)


@pytest.mark.parametrize("case_name,cut", [("case_se_regular", 40000), ("case_k63_regular", 40000)])
def test_a_run_of_more_than_2_to_15_kmers(case_name, cut, request):
    """one record like any other, through the DEVICE entry point (always the run kernel): a read cut from the longest string"""
    case = request.getfixturevalue(case_name)
    d = case.dict.to_device(0)
    s = max(case.sequences, key=len)
    assert len(s) > cut + 1000
    long_read = s[777:777 + cut]
    with_n = list(long_read)
    for at in (5000, 5001, 5002, 39000):
        with_n[at] = "N"
    reads = [s[:200], long_read, random_dna(np.random.default_rng(2), 90), revcomp(long_read), "", "".join(with_n), "N" * 34000 + s[:100]]
    want_offsets, want_runs = oracle_runs(case.oracle, reads)
    assert int(lengths_of(want_runs).max()) == cut - case.k + 1 > (1 << 15) and int(want_offsets[2] - want_offsets[1]) == 1
    check_both(d, reads, want_offsets, want_runs)


@pytest.mark.parametrize("fasta,k,m,canonical", [(SE_FASTA, 31, 13, 0), (SE_FASTA, 31, 13, 1)])
def test_runs_of_a_replica_without_the_table(fasta, k, m, canonical):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "gpu_runs_worker.py"), fasta, str(k), str(m), str(canonical), "3000"],
                       capture_output=True, text=True, timeout=900, env=dict(os.environ, SSHASH_AMD_SKTABLE="0"))
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    got = json.loads(p.stdout.strip().splitlines()[-1])
    assert got["ok"] and got["sk_slots"] == 0 and got["runs"] > 1000


@pytest.mark.parametrize("fasta,k,m,extra", [(SE_FASTA, 31, 13, []), (K63_FASTA, 63, 21, ["--canonical"])])
def test_cpp_facade_checker(fasta, k, m, extra):
    exe = os.path.join(ROOT, "tests", "cpp", "check_runs")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "sshash_amd", "csrc"), "tools"])
    p = subprocess.run([exe, fasta, str(k), str(m)] + extra, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "EVERYTHING OK!" in p.stdout
