"""GPU: the per-read streaming query -- for read r, the streaming_query_report the reference's state machine produces for that read
alone. Expected rows: the oracle's report of every read on its own (it is reset at every read, so the batch's six counters are the
column sums); compared for exact equality of all six columns of every row, and rows.sum(0) == the call's own report ==
Dictionary.streaming_query of the same reads."""
from __future__ import annotations

import gzip
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import FASTQ, K63_FASTA, ROOT, SE_FASTA
from gpu_per_read_worker import COLUMNS, device_rows, oracle_rows, random_dna, report_row, revcomp, synthetic_reads

pytestmark = pytest.mark.gpu

SEVEN = ["case_se_regular", "case_se_canonical", "case_skew_regular", "case_skew_canonical", "case_k63_canonical", "case_k63_regular",
         "case_small_k"]
_expected = {}


def _set_one(case):
    """the reads of the first set and the oracle's rows for them (made once per dictionary)"""
    if case.name not in _expected:
        reads = synthetic_reads(case.sequences, case.k, 3000, seed=17)
        _expected[case.name] = (reads, oracle_rows(case.oracle, reads))
    return _expected[case.name]


def _check(d, reads, want, what=""):
    rows, report = d.streaming_query_per_read(reads)
    assert rows.shape == (len(reads), 6) and rows.dtype == np.uint64
    wrong = np.flatnonzero((rows != want).any(1))
    assert wrong.size == 0, (what, wrong[:10], rows[wrong[:3]], want[wrong[:3]], [reads[i][:80] for i in wrong[:3]])
    assert (rows.sum(0) == report_row(report)).all(), what
    assert (report_row(report) == report_row(d.streaming_query(reads))).all(), what
    return rows


@pytest.mark.parametrize("case_name", SEVEN)
def test_rows_match_the_oracle_read_by_read(case_name, request):
    case = request.getfixturevalue(case_name)
    d = case.dict.to_device(0)
    reads, want = _set_one(case)
    n = len(reads)
    # what keeps this from passing on a trivial set, asserted on the ORACLE's rows
    assert (want[:, 5] > 0).sum() >= 0.20 * n, "reads with extensions"
    assert (want[:, 2] > 0).sum() >= 0.35 * n, "reads with negative k-mers"
    assert (want[:, 3] > 0).sum() >= 0.10 * n, "reads with invalid k-mers"
    assert len({tuple(r) for r in want.tolist()}) >= 400, "distinct rows"
    assert (want[:, 0] == 0).sum() >= 100, "reads without a k-mer"
    assert (want[:, 1] == want[:, 4] + want[:, 5]).all() and (want[:, 0] == want[:, 1] + want[:, 2] + want[:, 3]).all()
    assert (want.sum(0) == [case.oracle.streaming_query(reads)[c] for c in COLUMNS]).all()
    _check(d, reads, want)
    got, rep = device_rows(d, reads, prefill=-1, report=[0] * 6)
    assert (got == want).all() and (rep == want.sum(0)).all()


@pytest.mark.parametrize("case_name", ["case_se_regular", "case_se_canonical", "case_skew_regular", "case_k63_canonical", "case_k63_regular",
                                       "case_small_k", "case_m_equals_k"])
def test_rows_of_low_complexity_reads(case_name, request):
    """two-letter reads, homopolymers, short tandem repeats: ties between the strands, keys that never change (the reads of
    test_streaming_counters_on_low_complexity_reads, regenerated)"""
    case = request.getfixturevalue(case_name)
    d = case.dict.to_device(0)
    rng = np.random.default_rng(5)
    reads = synthetic_reads(case.sequences, case.k, 2000, seed=23)
    reads += ["".join(rng.choice(list("AC"), size=200)) for _ in range(50)] + ["A" * 300, "ACGT" * 60, ("A" * 40 + "C" * 40) * 3]
    _check(d, reads, oracle_rows(case.oracle, reads))


def _hand_made_reads(case):
    """one substitution at every distance from either end, runs starting at every alignment of the strings' words, whole strings, off
    a string's end into random bases and back, an N next to a substitution (the reads of
    test_streaming_runs_and_skips_against_hand_made_reads, regenerated)"""
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
def test_rows_of_hand_made_reads(case_name, request):
    case = request.getfixturevalue(case_name)
    d = case.dict.to_device(0)
    reads = _hand_made_reads(case)
    want = oracle_rows(case.oracle, reads)
    assert want[:, 5].sum() > 20 * want[:, 4].sum() > 0 and want[:, 2].sum() > 0 and want[:, 3].sum() > 0
    _check(d, reads, want)
    got, _ = device_rows(d, reads, prefill=123456789)
    assert (got == want).all()


@pytest.mark.parametrize("case_name", ["case_se_regular", "case_k63_canonical"])
def test_rows_do_not_depend_on_when_the_counters_move_out(case_name, request, monkeypatch):
    """SSHASH_AMD_TEST_HOOKS stream_move_out_every=<n>: the lanes' 32-bit counters go into the rows every n turns (added to what the
    row holds) instead of once at the end of the read"""
    case = request.getfixturevalue(case_name)
    d = case.dict.to_device(0)
    reads, want = _set_one(case)
    for at in ("1", "7", "300"):
        monkeypatch.setenv("SSHASH_AMD_TEST_HOOKS", "stream_move_out_every=" + at)
        _check(d, reads, want, at)
        got, rep = device_rows(d, reads, prefill=-1, report=[0] * 6)
        assert (got == want).all() and (rep == want.sum(0)).all(), at
    monkeypatch.delenv("SSHASH_AMD_TEST_HOOKS")
    _check(d, reads, want)


@pytest.mark.parametrize("case_name,cut", [("case_se_regular", 40000), ("case_se_canonical", 40000), ("case_k63_regular", 40000)])
def test_a_run_too_long_for_a_lane_counter(case_name, cut, request, monkeypatch):
    """one run of more than 2^15 extensions goes into the row at once, not through the lane's counter: a read cut from one string,
    forward and reverse-complemented, between ordinary reads, through the DEVICE entry point (always the run kernel)"""
    case = request.getfixturevalue(case_name)
    d = case.dict.to_device(0)
    s = max(case.sequences, key=len)
    assert len(s) > cut + 1000
    long_read = s[777:777 + cut]
    rng = np.random.default_rng(2)
    with_n = list(long_read)
    for at in (5000, 5001, 5002, 39000):  # invalid k-mers before and after a long run
        with_n[at] = "N"
    reads = [s[:200], long_read, random_dna(rng, 90), revcomp(long_read), "", "".join(with_n), s[300:500].lower(), "N" * 34000 + s[:100]]
    want = oracle_rows(case.oracle, reads)
    assert want[1, 5] == cut - case.k and want[1, 4] == 1 and want[3, 5] == cut - case.k  # one search, then extensions only
    assert want[5, 5] > (1 << 15) and want[7, 3] > (1 << 15)
    for hook in (None, "stream_move_out_every=3"):
        if hook:
            monkeypatch.setenv("SSHASH_AMD_TEST_HOOKS", hook)
        got, rep = device_rows(d, reads, prefill=-1, report=[1, 2, 3, 4, 5, 6])
        assert (got == want).all(), (hook, got, want)
        assert (rep == want.sum(0) + np.arange(1, 7, dtype=np.uint64)).all()
    monkeypatch.delenv("SSHASH_AMD_TEST_HOOKS")


@pytest.mark.parametrize("case_name", ["case_se_regular", "case_k63_regular"])
def test_reads_too_long_for_one_lane_take_the_position_parallel_pipeline(case_name, request):
    """the host entry point sends a piece holding a read above 2^16 bases through encode -> lookup -> classify: the same rows. One
    long read over many tiles with N's and substitutions in it, two long reads next to each other, short ones (and empty ones)
    around them, a long read last."""
    case = request.getfixturevalue(case_name)
    d = case.dict.to_device(0)
    k = case.k
    s = max(case.sequences, key=len)
    rng = np.random.default_rng(9)
    a = list(s[:100000])
    for at in rng.integers(0, len(a), 150):
        a[int(at)] = "ACGT"[int(rng.integers(0, 4))]
    for at in rng.integers(0, len(a), 60):
        a[int(at)] = "N"
    a = "".join(a)
    b = revcomp(s[20000:20000 + 70000])
    last = "N".join(case.sequences[int(i)] for i in rng.integers(0, len(case.sequences), 40))[:90000]
    while len(last) <= (1 << 16):
        last += "N" + s[:30000]
    shorts = synthetic_reads(case.sequences, k, 60, seed=3)
    reads = shorts[:20] + [a, b] + shorts[20:40] + ["", "ACGT"] + [s[5:5 + k], last[:70000].lower()] + shorts[40:] + [last]
    assert min(len(a), len(b), len(last)) > (1 << 16)
    want = oracle_rows(case.oracle, reads)
    assert want[20, 3] > 0 and want[20, 2] > 0 and want[20, 5] > 50000 and want[21, 5] > 50000 and want[-1, 0] == len(last) - k + 1
    _check(d, reads, want)


@pytest.mark.parametrize("case_name", ["case_se_canonical", "case_k63_canonical", "case_small_k"])
def test_rows_land_at_their_reads_across_pieces(case_name, request, monkeypatch):
    """SSHASH_AMD_TEST_HOOKS stream_piece_reads=<n>: the host call cuts its batch into pieces of n reads, run by several lanes side by
    side: row i is read i whatever piece it was in"""
    case = request.getfixturevalue(case_name)
    d = case.dict.to_device(0)
    reads, want = _set_one(case)
    assert len({tuple(r) for r in want.tolist()}) >= 400  # (a row in the wrong place shows)
    for piece in ("300", "257", "1"):
        some = slice(0, 200) if piece == "1" else slice(0, len(reads))
        monkeypatch.setenv("SSHASH_AMD_TEST_HOOKS", "stream_piece_reads=" + piece)
        _check(d, reads[some], want[some], piece)
    monkeypatch.delenv("SSHASH_AMD_TEST_HOOKS")


@pytest.mark.parametrize("env", [{"SSHASH_AMD_SKTABLE": "0", "SSHASH_AMD_DIRECTORY": "1"}, {"SSHASH_AMD_SKTABLE": "0", "SSHASH_AMD_DIRECTORY": "0"}],
                         ids=["directory", "mphf"])
@pytest.mark.parametrize("fasta,k,m,canonical", [(SE_FASTA, 31, 13, 0), (K63_FASTA, 63, 25, 1)])
def test_rows_of_a_replica_without_the_table(fasta, k, m, canonical, env):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "gpu_per_read_worker.py"), fasta, str(k), str(m), str(canonical), "1500"],
                       capture_output=True, text=True, timeout=900, env=dict(os.environ, **env))
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    got = json.loads(p.stdout.strip().splitlines()[-1])
    assert got["ok"] and got["sk_slots"] == 0 and (env["SSHASH_AMD_DIRECTORY"] == "1") == bool(got["directory_sectors"])
    assert got["totals"][5] > 0 and got["totals"][2] > 0


def test_device_entry_point_overwrites_rows_and_accumulates_the_report(case_se_regular):
    import torch

    case = case_se_regular
    d = case.dict.to_device(0)
    reads, want = _set_one(case)
    total = want.sum(0)
    for prefill in (-1, 0x0123456789ABCDEF, 0):
        got, rep = device_rows(d, reads, prefill=prefill, report=[10, 20, 30, 40, 50, 60])
        assert (got == want).all(), prefill
        assert (rep == total + np.array([10, 20, 30, 40, 50, 60], dtype=np.uint64)).all()
    got, rep = device_rows(d, reads, prefill=-1, report=None)  # report == NULL
    assert (got == want).all() and rep is None
    got, rep = device_rows(d, reads, prefill=-1, report=[0] * 6, total_bases=0)  # total_bases not known to the caller
    assert (got == want).all() and (rep == total).all()
    side = torch.cuda.Stream(device=0)
    got, rep = device_rows(d, reads, prefill=-1, report=[0] * 6, stream=side, launches=2)  # (device_rows compares the launches)
    assert (got == want).all() and (rep == 2 * total).all()
    # reads without any base: every row is written all the same; no reads: nothing is
    got, rep = device_rows(d, ["", "", ""], prefill=-1, report=[1] * 6, total_bases=0)
    assert (got == 0).all() and (rep == 1).all()
    d.streaming_query_per_read_device(0, 0, 0, 0, 0)
    # through the C++-style raw call with rows only shorter than k
    got, rep = device_rows(d, ["ACGT", "A" * (case.k - 1), ""], prefill=-1, report=[0] * 6)
    assert (got == 0).all() and (rep == 0).all()


def _collect(d, path, n, **kw):
    """the file query with a callback: the batches cover [0, n) exactly once and in order -> (rows, report)"""
    blocks, expect = [], [0]

    def take(first, rows):
        assert first == expect[0] and rows.ndim == 2 and rows.shape[1] == 6 and rows.dtype == np.uint64 and rows.shape[0] > 0
        expect[0] += rows.shape[0]
        blocks.append(rows)

    report = d.streaming_query_from_file(str(path), per_read=take, **kw)
    assert expect[0] == n, (expect[0], n)
    return (np.concatenate(blocks) if blocks else np.zeros((0, 6), dtype=np.uint64)), report


@pytest.mark.parametrize("case_name", ["case_se_regular", "case_k63_canonical"])
def test_query_files_give_a_row_per_record(case_name, request, tmp_path, monkeypatch):
    """a FASTQ of the first set's non-empty reads, those shorter than k included (they keep their rows: all zero): plain, gzip, plain
    with small pieces asked for, and the same reads as a single-line FASTA; in one batch and in many; a callback that returns 3 on its
    second call stops the query and is not called again"""
    import sshash_amd

    case = request.getfixturevalue(case_name)
    d = case.dict.to_device(0)
    all_reads, all_want = _set_one(case)
    keep = [i for i, r in enumerate(all_reads) if r]
    reads, want = [all_reads[i] for i in keep], all_want[keep]
    assert (want[:, 0] == 0).sum() >= 100 and min(len(r) for r in reads) < case.k
    fastq = "".join(f"@{i}\n{r}\n+\n{'I' * len(r)}\n" for i, r in enumerate(reads)).encode()
    fasta = "".join(f">{i}\n{r}\n" for i, r in enumerate(reads)).encode()
    (tmp_path / "q.fastq").write_bytes(fastq)
    (tmp_path / "q.fa").write_bytes(fasta)
    with gzip.open(tmp_path / "q.fastq.gz", "wb") as f:
        f.write(fastq)
    in_memory = _check(d, reads, want)
    for name, hooks in (("q.fastq", None), ("q.fastq.gz", None), ("q.fastq", "fastq_piece_bytes=4096"), ("q.fa", None),
                        ("q.fastq", "query_batch_bases=20000"), ("q.fa", "query_batch_bases=1"), ("q.fastq.gz", "query_batch_bases=77777,stream_piece_reads=100")):
        if hooks:
            monkeypatch.setenv("SSHASH_AMD_TEST_HOOKS", hooks)
        rows, report = _collect(d, tmp_path / name, len(reads))
        monkeypatch.delenv("SSHASH_AMD_TEST_HOOKS", raising=False)
        assert (rows == in_memory).all(), (name, hooks, np.flatnonzero((rows != in_memory).any(1))[:10])
        assert (report_row(report) == want.sum(0)).all(), (name, hooks)
        assert (report_row(d.streaming_query_from_file(str(tmp_path / name))) == want.sum(0)).all()  # (the totals drop nothing but zeros)
    # multiline FASTA: a record is a non-empty segment, headers and all
    (tmp_path / "m.fa").write_text("".join(f">{i}\n{r[:50]}\n{r[50:]}\n\n" if len(r) > 50 else f">{i}\n{r}\n\n" for i, r in enumerate(reads[:300])))
    segments = [f">{i}{r}" for i, r in enumerate(reads[:300])]
    rows, report = _collect(d, tmp_path / "m.fa", 300, multiline=True)
    assert (rows == oracle_rows(case.oracle, segments)).all()
    # a callback that wants no more
    calls = []

    def stop_at_second(first, rows):
        calls.append(first)
        return 3 if len(calls) == 2 else None

    monkeypatch.setenv("SSHASH_AMD_TEST_HOOKS", "query_batch_bases=20000")
    with pytest.raises(sshash_amd.SSHashError) as e:
        d.streaming_query_from_file(str(tmp_path / "q.fastq"), per_read=stop_at_second)
    assert e.value.status == 1 and "3" in str(e.value) and len(calls) == 2 and calls[0] == 0 and calls[1] > 0

    def broken(first, rows):
        raise KeyError("mine")

    with pytest.raises(KeyError):
        d.streaming_query_from_file(str(tmp_path / "q.fastq"), per_read=broken)
    monkeypatch.delenv("SSHASH_AMD_TEST_HOOKS")


def test_golden_fastq_known_answer(case_se_regular):
    """SRR5833294.10K has no positive k-mer in the Salmonella dictionaries: it serves as the known answer "10 000 rows, each with
    46 k-mers" (reads of 76 bases, k = 31), 459 143 negative and 857 invalid of 460 000 in all"""
    d = case_se_regular.dict.to_device(0)
    rows, report = _collect(d, FASTQ, 10000)
    assert (rows[:, 0] == 46).all() and (rows[:, 1] == 0).all() and (rows[:, 0] == rows[:, 2] + rows[:, 3]).all()
    assert rows.sum(0).tolist() == [460000, 0, 459143, 857, 0, 0] == report_row(report).tolist()


@pytest.mark.parametrize("fasta,k,m,extra", [(SE_FASTA, 31, 13, []), (K63_FASTA, 63, 21, ["--canonical"])])
def test_cpp_facade_checker(fasta, k, m, extra, tmp_path):
    exe = os.path.join(ROOT, "tests", "cpp", "check_per_read")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "sshash_amd", "csrc"), "tools"])
    p = subprocess.run([exe, fasta, str(k), str(m)] + extra, capture_output=True, text=True, timeout=600, env=dict(os.environ, TMPDIR=str(tmp_path)))
    assert p.returncode == 0, p.stdout + p.stderr
    assert "EVERYTHING OK!" in p.stdout
