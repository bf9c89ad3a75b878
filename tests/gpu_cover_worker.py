#!/usr/bin/env python
"""Worker of tests/test_gpu_streaming_cover.py: one process = one dictionary and one setting of the environment switches that decide
what a replica holds (read once per process: SSHASH_AMD_SKTABLE=0 is a replica without the super-k-mer table, whose run kernel takes
the complete seed() path). Everything the streaming cover promises, against ground truth that shares no code with it: the bitmap built
in numpy from the kmer_id values of streaming_lookup over the same reads, and from the CPU oracle's point lookups of every k-mer of
every read. Prints one JSON line; any mismatch is an assertion error.

    python tests/gpu_cover_worker.py <fasta> <k> <m> <canonical 0|1> <scratch directory>"""
import gzip
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import numpy as np

from gpu_per_read_worker import random_dna, report_row, revcomp, synthetic_reads

INVALID = np.uint64(0xFFFFFFFFFFFFFFFF)
BACKWARD = 0x80000000
FASTQ = os.path.join(ROOT, "tests", "golden", "SRR5833294.10K.fastq.gz")
GUARD = 0x5A5A5A5A5A5A5A5A


def bitmap_of(ids, words):
    """numpy: the bitmap holding the ids that are not INVALID (id i = bit i & 63 of word i >> 6)"""
    ids = np.asarray(ids, dtype=np.uint64)
    ids = ids[ids != INVALID]
    cover = np.zeros(words, dtype=np.uint64)
    np.bitwise_or.at(cover, (ids >> np.uint64(6)).astype(np.int64), np.uint64(1) << (ids & np.uint64(63)))
    return cover


def popcount(cover):
    return int(np.unpackbits(cover.view(np.uint8)).sum())


def truth_from_lookup(d, reads):
    per_read, _ = d.streaming_lookup(reads)
    return bitmap_of(np.concatenate([p.kmer_id for p in per_read] + [np.zeros(0, dtype=np.uint64)]), d.cover_words())


def truth_from_oracle(oracle, reads, k, words):
    """the point lookup (either strand) of every k-mer of every read that holds nothing but A, C, G, T in either case"""
    ok = np.zeros(256, dtype=bool)
    ok[list(b"ACGTacgt")] = True
    kmers = []
    for r in reads:
        b = np.frombuffer(r.encode("ascii", "replace") if isinstance(r, str) else bytes(r), dtype=np.uint8)
        if b.size < k:
            continue
        windows = np.lib.stride_tricks.sliding_window_view(b, k)
        kmers.append(windows[ok[windows].all(axis=1)] & np.uint8(0xDF))  # (upper case)
    if not kmers:
        return np.zeros(words, dtype=np.uint64)
    res = oracle.lookup_ascii(np.ascontiguousarray(np.concatenate(kmers)).reshape(-1), True)
    return bitmap_of(res["kmer_id"], words)


def device_cover(d, reads, before=None, report=None, stream=None, total_bases=None):
    """the device entry point on device 0 into a bitmap that holds `before` (None: zeros), with a guard word behind its last word
    -> (bitmap, report or None); asserts that the guard word is untouched"""
    import torch

    dev = torch.device("cuda", 0)
    words = d.cover_words()
    blob = "".join(reads).encode()
    offsets = np.zeros(len(reads) + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum([len(r) for r in reads])
    d_bases = torch.frombuffer(bytearray(blob or b"\0"), dtype=torch.uint8).to(dev)
    d_off = torch.from_numpy(offsets.view(np.int64)).to(dev)
    host = np.full(words + 1, GUARD, dtype=np.uint64)
    host[:words] = 0 if before is None else before
    d_cover = torch.from_numpy(host.view(np.int64).copy()).to(dev)
    d_report = None if report is None else torch.from_numpy(np.asarray(report, dtype=np.uint64).view(np.int64).copy()).to(dev)
    torch.cuda.synchronize()  # (the copies run on torch's stream, the query may run on another)
    d.streaming_cover_device(0, d_bases.data_ptr(), d_off.data_ptr(), len(reads), d_cover.data_ptr(), d_report=0 if d_report is None else d_report.data_ptr(),
                             stream=0 if stream is None else stream.cuda_stream, total_bases=len(blob) if total_bases is None else total_bases)
    (stream or torch.cuda.current_stream(dev)).synchronize()
    torch.cuda.synchronize()
    got = d_cover.cpu().numpy().view(np.uint64)
    assert int(got[words]) == GUARD, "the word behind the bitmap was written"
    return got[:words].copy(), None if d_report is None else d_report.cpu().numpy().view(np.uint64)


def device_string_counts(d, cover):
    import torch

    dev = torch.device("cuda", 0)
    d_cover = torch.from_numpy(cover.view(np.int64).copy()).to(dev)
    d_counts = torch.full((d.num_strings() + 2,), -3, dtype=torch.int64, device=dev)  # counts, the total, a guard
    torch.cuda.synchronize()
    d.cover_string_counts_device(0, d_cover.data_ptr(), d_counts.data_ptr(), d_counts.data_ptr() + 8 * d.num_strings())
    torch.cuda.synchronize()
    out = d_counts.cpu().numpy()
    assert out[-1] == -3, "the word behind the total was written"
    return out[:-2].view(np.uint64), int(out[-2])


def same(got, want, what):
    assert got.dtype == np.uint64 and got.shape == want.shape, what
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (what, "words", bad[:5].tolist(), [hex(int(got[i])) for i in bad[:5]], [hex(int(want[i])) for i in bad[:5]])


def make_reads(d, sequences, k):
    """every kind of read the cover form of the kernel has a branch for; which kinds are really there is asserted from the runs"""
    rng = np.random.default_rng(23)
    reads = synthetic_reads(sequences, k, 1500, seed=29)  # substitutions that cut runs, N, lower case, random reads, "", k - 1 bases, N's
    by_length = sorted(range(len(sequences)), key=lambda i: len(sequences[i]))
    whole = [i for i in by_length if len(sequences[i]) <= 6000]
    for i in whole[:3] + whole[len(whole) // 2:len(whole) // 2 + 3] + whole[-3:]:  # whole strings and their reverse complements
        reads += [sequences[i], revcomp(sequences[i])]
    first, last = sequences[0], sequences[-1]
    reads += [first[:k + 130], revcomp(first[:k + 70]), last[-(k + 130):], revcomp(last[-(k + 70):])]  # k-mer id 0 and id num_kmers - 1
    long_seqs = [s for s in sequences if len(s) >= 3 * k + 300]
    for j in range(60):
        s = long_seqs[int(rng.integers(0, len(long_seqs)))]
        a = int(rng.integers(0, len(s) - (2 * k + 200)))
        reads.append(s[a:a + k])                              # a run of one k-mer
        reads.append(revcomp(s[a + 7:a + 7 + k]))
        reads.append(s[a:a + k + int(rng.integers(1, 20))])   # a short run: as a rule inside one word
        reads.append(revcomp(s[a + 3:a + k + 190]))           # a run of 64 k-mers and more, backward in a regular dictionary
        cut = list(s[a:a + 2 * k + 150])
        for at in (k + 3, k + 4 + int(rng.integers(0, 100))):
            cut[at] = "ACGT"[("ACGT".index(cut[at].upper()) + 1 + j % 3) % 4]
        reads.append("".join(cut))                            # substitutions that cut runs
    s = long_seqs[0]
    n_read = list(s[10:10 + 2 * k + 60])
    n_read[k + 9] = "N"
    reads += ["".join(n_read), "N" * 40, "A" * (k - 1), "", random_dna(rng, 200), random_dna(rng, k)]
    hot = s[40:40 + k + 100]
    return reads, [hot] * 4096  # the same read 4096 times: many lanes OR into the same words


def runs_cover(d, reads, k):
    """the bitmap out of streaming_runs + expand_runs, and the runs themselves"""
    import sshash_amd

    run_offsets, runs, _ = d.streaming_runs(reads)
    back = sshash_amd.expand_runs(run_offsets, runs, [len(r) for r in reads], k)
    return bitmap_of(np.concatenate([b.kmer_id for b in back] + [np.zeros(0, dtype=np.uint64)]), d.cover_words()), runs


def main():
    import torch

    import sshash_amd
    from oracle import oracle as O
    from oracle.ground_truth import read_fasta_sequences

    fasta, k, m, canonical, scratch = sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), bool(int(sys.argv[4])), sys.argv[5]
    d = sshash_amd.Dictionary.build(fasta, k=k, m=m, canonical=canonical, num_threads=4).to_device(0)
    st = d.device_stats(0)
    sequences = read_fasta_sequences(fasta, k)
    words, n_kmers = d.cover_words(), d.num_kmers()
    assert words == (n_kmers + 63) // 64
    reads, repeated = make_reads(d, sequences, k)
    everything = reads + repeated

    # ---- ground truth, twice; what the reads exercise ----
    want = truth_from_lookup(d, reads)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "w.sshash")
        d.save(path)
        oracle = O.OracleIndex(path)
        same(truth_from_oracle(oracle, reads, k, words), want, "the oracle's point lookups against streaming_lookup")
    from_runs, runs = runs_cover(d, reads, k)
    same(from_runs, want, "streaming_runs + expand_runs against streaming_lookup")
    covered = popcount(want)
    assert 0 < covered < n_kmers, "the expected bitmap must hold set and clear bits"
    n = (runs["num_kmers"] & 0x7FFFFFFF).astype(np.uint64)
    backward = (runs["num_kmers"] & BACKWARD) != 0
    lo = np.where(backward, runs["kmer_id"] + np.uint64(1) - n, runs["kmer_id"])
    hi = lo + n
    one_word = (lo >> np.uint64(6)) == ((hi - np.uint64(1)) >> np.uint64(6))
    kinds = {"backward": int(backward.sum()), "forward": int((~backward).sum()), "runs_of_one": int((n == 1).sum()), "runs_of_64_and_more": int((n >= 64).sum()),
             "runs_inside_one_word": int((one_word & (n > 1)).sum()), "runs_over_three_words_and_more": int((((hi - np.uint64(1)) >> np.uint64(6)) - (lo >> np.uint64(6)) >= 2).sum()),
             "covers_id_0": int((lo == 0).sum()), "covers_last_id": int((hi == np.uint64(n_kmers)).sum())}
    assert all(v > 0 for v in kinds.values()), kinds
    rows, _ = d.streaming_query_per_read(reads)
    lengths = np.array([len(r) for r in reads])
    strings = set(sequences)
    kinds.update({"reads_with_N": sum("N" in r for r in reads), "reads_shorter_than_k": int((lengths < k).sum()), "empty_reads": int((lengths == 0).sum()),
                  "reads_without_a_hit": int(((rows[:, 0] > 0) & (rows[:, 1] == 0)).sum()), "reads_with_cut_runs": int((rows[:, 4] >= 2).sum()),
                  "whole_strings": len(set(reads) & strings), "reverse_complements_of_whole_strings": len({revcomp(r) for r in reads if r} & strings)})
    assert all(v > 0 for v in kinds.values()), kinds

    # ---- the cover, host and device; the report ----
    want_report = report_row(d.streaming_query(reads))
    got, rep = d.streaming_cover(reads)
    same(got, want, "host call")
    assert (report_row(rep) == want_report).all(), ("host report", report_row(rep), want_report)
    got, rep = device_cover(d, reads, report=[0] * 6)
    same(got, want, "device call")
    assert (rep == want_report).all(), ("device report", rep, want_report)
    if n_kmers % 64:
        assert int(got[-1]) >> (n_kmers % 64) == 0, "bits at or above num_kmers"
    got, rep = device_cover(d, reads, report=[1, 2, 3, 4, 5, 6], stream=torch.cuda.Stream(device=0), total_bases=0)  # a stream of the caller's; total_bases unknown
    same(got, want, "device call on a side stream")
    assert (rep == want_report + np.arange(1, 7, dtype=np.uint64)).all(), "the report is accumulated into"
    got, rep = device_cover(d, reads)  # a NULL report
    same(got, want, "device call without a report")

    # ---- the same read 4096 times ----
    want_hot = truth_from_lookup(d, repeated[:1])
    assert popcount(want_hot) == 101
    got, _ = device_cover(d, repeated)
    same(got, want_hot, "one read 4096 times, device call")
    got, _ = d.streaming_cover(everything)
    same(got, want | want_hot, "all reads and the repeated one, host call")

    # ---- accumulation and bounds ----
    rng = np.random.default_rng(5)
    before = bitmap_of(rng.integers(0, n_kmers, n_kmers // 50).astype(np.uint64), words)
    assert (before & ~want).any() and (want & ~before).any()
    got, _ = device_cover(d, reads, before=before)
    same(got, want | before, "bits set before the device call")
    mine = before.copy()
    got, _ = d.streaming_cover(reads, cover=mine)
    assert got is mine
    same(mine, want | before, "bits set before the host call")
    half = len(reads) // 2
    want_a, want_b = truth_from_lookup(d, reads[:half]), truth_from_lookup(d, reads[half:])
    assert (want_a & ~want_b).any() and (want_b & ~want_a).any()
    same(want_a | want_b, want, "the two halves' truth")
    got, _ = device_cover(d, reads[:half])
    same(got, want_a, "first batch, device call")
    got, _ = device_cover(d, reads[half:], before=got)
    same(got, want, "two batches into one bitmap, device call")
    two, _ = d.streaming_cover(reads[:half])
    d.streaming_cover(reads[half:], cover=two)
    same(two, want, "two batches into one bitmap, host call")
    # no reads at all, and reads without a base
    d.streaming_cover_device(0, 0, 0, 0, 0)
    got, rep = device_cover(d, ["", "", ""], before=before, report=[1] * 6, total_bases=0)
    same(got, before, "reads without a base")
    assert (rep == 1).all()

    # ---- geometry independence: the test hooks of the run kernel and of the host call's pieces ----
    for hook in ("stream_move_out_every=1", "stream_move_out_every=7", "stream_move_out_every=300", "stream_piece_reads=300", "stream_piece_reads=257"):
        os.environ["SSHASH_AMD_TEST_HOOKS"] = hook
        got, rep = d.streaming_cover(reads)
        assert got.tobytes() == want.tobytes() and (report_row(rep) == want_report).all(), hook
        got, rep = device_cover(d, reads, report=[0] * 6)
        assert got.tobytes() == want.tobytes() and (rep == want_report).all(), hook
    del os.environ["SSHASH_AMD_TEST_HOOKS"]

    # ---- a read above 2^16 bases: the host call's position-parallel route against the same bases cut into short reads ----
    parts, size = [], 0
    order = np.random.default_rng(9).permutation(len(sequences))
    while size <= 70000:  # (a small dictionary goes round more than once: a k-mer may come twice)
        for i in order:
            s = sequences[int(i)][:3000]
            parts.append(revcomp(s) if len(parts) % 3 == 1 else s)
            size += len(parts[-1])
            if size > 70000:
                break
    long_read = "".join(parts)
    assert len(long_read) > (1 << 16)
    step = 1000
    pieces = [long_read[a:a + step + k - 1] for a in range(0, len(long_read) - k + 1, step)]  # overlapping by k - 1: the same k-mers
    assert sum(len(p) - k + 1 for p in pieces) == len(long_read) - k + 1
    want_long, rep_pieces = d.streaming_cover(pieces + reads[:40])
    same(want_long, truth_from_lookup(d, pieces + reads[:40]), "the pieces of the long read")
    got, rep = d.streaming_cover(reads[:20] + [long_read, ""] + reads[20:40])
    same(got, want_long, "a batch that holds a read above 2^16 bases, host call")
    assert rep.num_positive_kmers == rep_pieces.num_positive_kmers and rep.num_kmers == rep_pieces.num_kmers
    assert popcount(want_long) > 10000
    got, _ = device_cover(d, [long_read])  # (the device call: one lane walks it)
    same(got, truth_from_lookup(d, pieces), "the long read, device call")

    # ---- query files ----
    with gzip.open(FASTQ, "rt") as f:
        fastq_reads = [line.strip() for i, line in enumerate(f) if i % 4 == 1]
    assert len(fastq_reads) == 10000
    want_fastq, want_fastq_report = d.streaming_cover(fastq_reads)
    got, rep = d.streaming_cover_from_file(FASTQ)
    same(got, want_fastq, "the FASTQ file against its parsed reads")
    assert rep == want_fastq_report, (rep, want_fastq_report)
    os.environ["SSHASH_AMD_TEST_HOOKS"] = "query_batch_bases=200000"  # (batch seams inside the file: the bitmap stays on the device across them)
    got, rep = d.streaming_cover_from_file(FASTQ)
    del os.environ["SSHASH_AMD_TEST_HOOKS"]
    same(got, want_fastq, "the FASTQ file in many batches")
    assert rep == want_fastq_report
    fasta_reads = [sequences[int(i)] for i in order[:400]]
    own = os.path.join(scratch, f"own_strings_k{k}_{int(canonical)}.fa")
    with open(own, "w") as f:
        for i, s in enumerate(fasta_reads):
            f.write(f">{i}\n{s}\n")
    want_fasta, want_fasta_report = d.streaming_cover(fasta_reads)
    assert popcount(want_fasta) == sum(len(s) - k + 1 for s in fasta_reads), "every k-mer of the dictionary's own strings is found"
    got, rep = d.streaming_cover_from_file(own, cover=before.copy())
    same(got, want_fasta | before, "the FASTA file against its parsed reads, into a bitmap that held bits")
    assert rep == want_fasta_report

    # ---- covered k-mers per string ----
    for name, cover in (("reads", want), ("fastq", want_fastq), ("fasta", want_fasta), ("long", want_long), ("zero", np.zeros(words, dtype=np.uint64)),
                        ("ones", np.full(words, ~np.uint64(0), dtype=np.uint64))):
        host_counts, host_total = d.cover_string_counts(cover)
        counts, total = device_string_counts(d, cover)
        same(counts, host_counts, "counts per string of " + name)
        valid = cover.copy()
        if n_kmers % 64:
            valid[-1] &= np.uint64((1 << (n_kmers % 64)) - 1)
        assert total == host_total == popcount(valid) == int(counts.sum()), (name, total, host_total, popcount(valid))
    counts, total = device_string_counts(d, want_fasta)
    sizes = d.string_size(np.sort(order[:400]).astype(np.uint64))
    assert (counts[np.sort(order[:400])] == sizes).all() and total == int(sizes.sum())

    print(json.dumps({"ok": True, "reads": len(reads), "covered": covered, "num_kmers": n_kmers, "sk_slots": st["sk_slots"], "kinds": kinds}))


if __name__ == "__main__":
    main()
