#!/usr/bin/env python
"""Worker of tests/test_gpu_runs_segments.py: one process = one dictionary, one setting of SSHASH_AMD_SKTABLE and one case. The run records
of reads cut into segments of S k-mers (Dictionary.set_read_segments) must be byte for byte those of the uncut reads: run_offsets and
runs.tobytes(), through the host call, the device call at every capacity, and the file call. Expected values come from the run rule over
the CPU oracle's per-k-mer streaming results, and independently from the same calls under SEGMENTS_OFF. Before anything runs on the GPU
the worker asserts, from the oracle's per-k-mer results, that for every S of {1, 2, 7, 64} seams fall inside forward and backward runs,
on a run's first k-mer, behind its last, on a negative and on an invalid k-mer, and that a run spans three whole segments and more. That
a segmented launch really happened is read from the counter of read_segments(). Prints one JSON line; any mismatch is an assertion error.

    python tests/gpu_runs_segments_worker.py <fasta> <k> <m> <canonical 0|1> <scratch directory> <case> [S]
    case: segments (needs S) | long | file | counters"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import numpy as np

from gpu_per_read_worker import COLUMNS, report_row
from gpu_runs_worker import BACKWARD, RUN_DTYPE, device_runs, oracle_runs, same_records
from gpu_segments_worker import ALL_S, S_MAX, kinds_of, launches, long_read_of, make_reads, oracle_for, per_kmer

SENTINEL = 0x5A


def the_reads(sequences, k):
    """the reads of the segments test -- a few hundred, every kind of seam in them (kinds_of) --, and behind them, LAST, a read that follows
    one string for more than 4 * 64 + k k-mers: the empty entries of the segment table lie behind the segments of a long read"""
    reads = make_reads(sequences, k)
    long_seqs = sorted((s for s in sequences if len(s) >= 4 * S_MAX + 2 * k + 40), key=len)
    assert long_seqs
    reads.append(long_seqs[-1][:1200])
    assert len(reads[-1]) - k + 1 >= 4 * S_MAX + k
    return reads


def chains(kinds, S):
    """how many runs hold three whole segments of S k-mers and more: extensions from a seam to the seam after the next two"""
    n = 0
    for kind in kinds:
        for j in range(S, kind.size - 3 * S + 1, S):
            n += bool((kind[j:j + 3 * S] == 3).all())
    return n


def truth(d, reads, k):
    """-> (run_offsets, records, the six counters) out of the oracle, the reads' kinds asserted"""
    oracle = oracle_for(d)
    per = [per_kmer(oracle, r, k) for r in reads]
    kinds, oris = [p[0] for p in per], [p[1] for p in per]
    found = kinds_of(reads, kinds, oris, k)
    for S in ALL_S:
        assert chains(kinds, S) > 0, ("no run spans three whole segments", S)
    want_offsets, want_runs = oracle_runs(oracle, reads)
    rep = oracle.streaming_query(reads)
    totals = np.array([rep[c] for c in COLUMNS], dtype=np.uint64)
    assert int(want_offsets[-1]) == int(totals[4]) and int((want_runs["num_kmers"] & np.uint32(BACKWARD - 1)).sum()) == int(totals[1])
    assert (want_runs["num_kmers"] & BACKWARD).any() and not (want_runs["num_kmers"] & BACKWARD).all()
    return want_offsets, want_runs, totals, found


def host_same(d, reads, want_offsets, want_runs, want_totals, what):
    ro, runs, report = d.streaming_runs(reads)
    assert ro.dtype == np.uint64 and ro.tobytes() == want_offsets.tobytes(), (what, "host run_offsets", np.flatnonzero(ro != want_offsets)[:10])
    assert same_records(runs, want_runs), (what, "host records", [i for i in range(min(len(runs), len(want_runs))) if runs[i] != want_runs[i]][:5])
    if want_totals is not None:
        assert (report_row(report) == want_totals).all(), (what, "host report", report_row(report), want_totals)


def device_same(d, reads, capacity, want_offsets, want_runs, what, report=None, want_report=None):
    ro, buffer, rep = device_runs(d, reads, capacity=capacity, report=report, tail=3, sentinel=SENTINEL)
    kept = min(capacity, int(want_offsets[-1]))
    assert ro.tobytes() == want_offsets.tobytes(), (what, capacity, "device run_offsets", np.flatnonzero(ro != want_offsets)[:10])
    assert buffer[:kept].tobytes() == want_runs[:kept].tobytes(), (what, capacity, "device records", [i for i in range(kept) if buffer[i] != want_runs[i]][:5])
    assert (buffer[kept:].view(np.uint8) == SENTINEL).all(), (what, capacity, "written at or behind the capacity")
    if want_report is not None:
        assert (rep == want_report).all(), (what, capacity, "device report", rep, want_report)


def case_segments(d, sequences, k, S):
    import sshash_amd

    reads = the_reads(sequences, k)
    want_offsets, want_runs, want_totals, found = truth(d, reads, k)
    total = int(want_offsets[-1])
    assert total > len(reads) // 2  # (most reads hit, several more than once)
    capacities = (0, 1, total - 1, total, total + 3)
    start = np.arange(1, 7, dtype=np.uint64) * np.uint64(1000003)
    d.to_device(0)
    st = d.device_stats(0)
    # ---- SEGMENTS_OFF: the second truth ----
    d.set_read_segments(sshash_amd.SEGMENTS_OFF, device_calls=True)
    host_same(d, reads, want_offsets, want_runs, want_totals, "OFF")
    off_ro, off_runs, _ = d.streaming_runs(reads)
    device_same(d, reads, total, off_ro, off_runs, "OFF", report=[0] * 6, want_report=want_totals)
    assert launches(d) == 0, "SEGMENTS_OFF launched over segments"
    # ---- S, host call ----
    d.set_read_segments(S, device_calls=True)
    host_same(d, reads, want_offsets, want_runs, want_totals, f"S = {S}")
    n_host = launches(d)
    assert n_host >= 1, "the host call did not launch over segments"
    # ---- S, device call: every capacity, guard records behind it, one launch counted per call ----
    for capacity in capacities:
        before = launches(d)
        device_same(d, reads, capacity, want_offsets, want_runs, f"S = {S}", report=[0] * 6, want_report=want_totals)
        assert launches(d) == before + 1, "a segmented device call counts one launch"
    device_same(d, reads, total, want_offsets, want_runs, f"S = {S}, a report that holds values", report=start, want_report=want_totals + start)
    device_same(d, reads, total, want_offsets, want_runs, f"S = {S}, a NULL report")
    device_same(d, reads, 0, want_offsets, want_runs, f"S = {S}, counting, a NULL report")
    # ---- geometry: pieces inside the batch (host), the counters moved out every turn ----
    for hook in ("stream_piece_reads=37", "stream_move_out_every=1"):
        os.environ["SSHASH_AMD_TEST_HOOKS"] = hook
        host_same(d, reads, want_offsets, want_runs, want_totals, f"S = {S}, {hook}")
        device_same(d, reads, total, want_offsets, want_runs, f"S = {S}, {hook}", report=[0] * 6, want_report=want_totals)
    del os.environ["SSHASH_AMD_TEST_HOOKS"]
    # ---- no reads, reads without a base ----
    ro, _, _ = device_runs(d, ["", "", ""], capacity=0, total_bases=0)
    assert not ro.any()
    return {"ok": True, "S": S, "reads": len(reads), "runs": total, "segmented_launches": launches(d), "sk_slots": st["sk_slots"],
            "seams_in_runs": found[f"seam_in_forward_run@{S}"] + found[f"seam_in_backward_run@{S}"]}


def case_long(d, sequences, k):
    """one read above 2^16 bases at the default S through the host and the device call, against SEGMENTS_OFF"""
    import sshash_amd

    long_read = long_read_of(sequences, 70000)
    assert len(long_read) > (1 << 16)
    few = make_reads(sequences, k)[:40]
    batch = few[:20] + [long_read, ""] + few[20:]
    d.to_device(0)
    assert d.read_segments()["kmers"] == sshash_amd.SEGMENTS_OFF, "a new dictionary does not segment"
    d.set_read_segments(sshash_amd.SEGMENTS_OFF, device_calls=True)
    want_ro, want_runs, want_report = d.streaming_runs(batch)  # (the per-k-mer pipeline for the long read's piece)
    total = int(want_ro[-1])
    device_same(d, batch, total, want_ro, want_runs, "OFF, the device call: one lane walks the long read")
    assert launches(d) == 0
    mine = want_runs[int(want_ro[20]):int(want_ro[21])]
    assert mine.size > 10 and int((mine["num_kmers"] & np.uint32(BACKWARD - 1)).max()) > 1000, "the long read has long runs"
    d.set_read_segments()  # the default S, host calls only
    S = d.read_segments()["kmers"]
    assert 1 < S < len(long_read) // 4
    host_same(d, batch, want_ro, want_runs, report_row(want_report), "the default S, host call")
    before = launches(d)
    assert before >= 1
    device_same(d, batch, total, want_ro, want_runs, "device_calls = 0")
    assert launches(d) == before
    d.set_read_segments(device_calls=True)
    device_same(d, batch, total, want_ro, want_runs, "the default S, device call", report=[0] * 6, want_report=report_row(want_report))
    device_same(d, batch, total // 2, want_ro, want_runs, "the default S, device call, half the room")
    assert launches(d) == before + 2
    return {"ok": True, "S": S, "bases": len(long_read), "runs": total, "segmented_launches": launches(d)}


def case_file(d, sequences, k, scratch):
    """a multiline FASTA with a record of ~3 kb, and a FASTQ, in batches that seam inside the file, at S = 7 and with the segments off"""
    import sshash_amd

    s = max(sequences, key=len)[:3000]
    assert len(s) >= 2500
    pool = [q for q in sequences if len(q) >= 400]
    others = [pool[i][:200 + 17 * i] for i in range(1, 9)]  # (more than 1500 bases together: the batches below seam between them)
    assert all(len(o) == 200 + 17 * (i + 1) for i, o in enumerate(others))
    fasta = os.path.join(scratch, f"runs_multiline_k{k}_{int(d.canonical())}.fa")
    with open(fasta, "w") as f:
        f.write(">short0\n" + others[0] + "\n\n>long\n" + "".join(s[a:a + 60] + "\n" for a in range(0, len(s), 60)))
        for i, o in enumerate(others[1:]):
            f.write(f"\n>short{i + 1}\n" + o + "\n")
    records = [">short0" + others[0], ">long" + s] + [f">short{i + 1}" + o for i, o in enumerate(others[1:])]  # (multiline: a record is a non-empty segment of the file, header and all)
    reads = [r for r in make_reads(sequences, k)[:150] if r] + ["ACGT", sequences[0][:k - 1]]
    fastq = os.path.join(scratch, f"runs_k{k}_{int(d.canonical())}.fastq")
    with open(fastq, "w") as f:
        for i, r in enumerate(reads):
            f.write(f"@r{i}\n{r}\n+\n{'I' * len(r)}\n")
    d.to_device(0)
    out = {}
    for name, path, multiline, parsed in (("fasta", fasta, True, records), ("fastq", fastq, False, reads)):
        d.set_read_segments(sshash_amd.SEGMENTS_OFF)
        want_ro, want_runs, want_report = d.streaming_runs(parsed)
        assert int(want_ro[-1]) > len(parsed) // 2
        for S in (sshash_amd.SEGMENTS_OFF, 7):
            d.set_read_segments(S)
            before = launches(d)
            os.environ["SSHASH_AMD_TEST_HOOKS"] = "query_batch_bases=1500"
            ro, runs, report = d.streaming_runs_from_file(path, multiline=multiline)
            batches = []

            def keep(first, offsets, block):
                assert offsets.dtype == np.uint64 and offsets[0] == 0 and block.dtype == RUN_DTYPE and int(offsets[-1]) == block.size
                batches.append((first, offsets.size - 1))
                lo = int(want_ro[first])
                assert (offsets + np.uint64(lo) == want_ro[first:first + offsets.size]).all(), (name, S, "a batch's offsets", first)
                assert block.tobytes() == want_runs[lo:lo + block.size].tobytes(), (name, S, "a batch's records", first)

            report2 = d.streaming_runs_from_file(path, multiline=multiline, per_batch=keep)
            calls = []

            def stop(first, offsets, block):
                calls.append(first)
                return 7

            try:
                d.streaming_runs_from_file(path, multiline=multiline, per_batch=stop)
                raise AssertionError("a callback that returned 7 did not stop the call")
            except sshash_amd.SSHashError as e:
                assert e.status == 1 and "7" in str(e) and calls == [0]
            del os.environ["SSHASH_AMD_TEST_HOOKS"]
            assert ro.tobytes() == want_ro.tobytes() and same_records(runs, want_runs), (name, S, "the stitched file call")
            assert report == want_report and report2 == want_report, (name, S)
            assert len(batches) >= 3 and batches[0][0] == 0 and sum(n for _, n in batches) == len(parsed), "batches seam inside the file, in file order"
            assert all(batches[i][0] + batches[i][1] == batches[i + 1][0] for i in range(len(batches) - 1))
            assert (launches(d) > before) == (S == 7), (name, S, "segmented launches")
        out[name] = int(want_ro[-1])
    return {"ok": True, "runs": out, "segmented_launches": launches(d)}


def case_counters(fasta, k, m, canonical, d, sequences):
    """where the counter does not move: device_calls = 0 (device call), and a minimizer shard whatever is set"""
    import sshash_amd

    reads = the_reads(sequences, k)
    d.to_device(0)
    d.set_read_segments(sshash_amd.SEGMENTS_OFF)
    want_ro, want_runs, _ = d.streaming_runs(reads)
    total = int(want_ro[-1])
    d.set_read_segments(7, device_calls=False)
    device_same(d, reads, total, want_ro, want_runs, "device_calls = 0")
    assert launches(d) == 0, "device_calls = 0 launched over segments"
    d.streaming_runs(reads)
    assert launches(d) >= 1
    shard = sshash_amd.Dictionary.build(fasta, k=k, m=m, canonical=canonical, num_threads=4, num_shards=2, shard_id=0).to_device(0)
    shard.set_read_segments(sshash_amd.SEGMENTS_OFF)
    off_ro, off_runs, _ = shard.streaming_runs(reads)
    dro, dbuf, _ = device_runs(shard, reads, capacity=int(off_ro[-1]) + 64, tail=0)
    shard.set_read_segments(7, device_calls=True)
    ro, runs, _ = shard.streaming_runs(reads)
    assert ro.tobytes() == off_ro.tobytes() and same_records(runs, off_runs), "a shard's host call: S = 7 against OFF"
    dro2, dbuf2, _ = device_runs(shard, reads, capacity=int(off_ro[-1]) + 64, tail=0)
    assert dro2.tobytes() == dro.tobytes() and dbuf2.tobytes() == dbuf.tobytes(), "a shard's device call: S = 7 against OFF"
    assert launches(shard) == 0, "a minimizer shard launched over segments"
    return {"ok": True, "segmented_launches": launches(d), "shard_runs": int(off_ro[-1])}


def main():
    import sshash_amd
    from oracle.ground_truth import read_fasta_sequences

    fasta, k, m, canonical, scratch, case = sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), bool(int(sys.argv[4])), sys.argv[5], sys.argv[6]
    sequences = read_fasta_sequences(fasta, k)
    d = sshash_amd.Dictionary.build(fasta, k=k, m=m, canonical=canonical, num_threads=4)
    if case == "segments":
        out = case_segments(d, sequences, k, int(sys.argv[7]))
    elif case == "long":
        out = case_long(d, sequences, k)
    elif case == "file":
        out = case_file(d, sequences, k, scratch)
    elif case == "counters":
        out = case_counters(fasta, k, m, canonical, d, sequences)
    else:
        raise SystemExit("unknown case " + case)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
