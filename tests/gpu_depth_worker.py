#!/usr/bin/env python
"""Worker of tests/test_gpu_streaming_depth.py: one process = one dictionary and one setting of the environment switches that decide
what a replica holds (SSHASH_AMD_SKTABLE=0: a replica without the super-k-mer table, whose run kernel takes the complete seed() path).
Everything the streaming depth promises, against ground truth that shares no code with it: numpy.bincount over the kmer_id values of
streaming_lookup over the same reads, and the same over the CPU oracle's point lookups of every k-mer of every read. The oracle's ids
also say, before anything runs on the GPU, that the reads hold every kind of run the kernel has a branch for. Prints one JSON line; any
mismatch is an assertion error.

    python tests/gpu_depth_worker.py <fasta> <k> <m> <canonical 0|1> <scratch directory> [shards]"""
import gzip
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import numpy as np

from gpu_cover_worker import make_reads
from gpu_per_read_worker import report_row, revcomp

INVALID = np.uint64(0xFFFFFFFFFFFFFFFF)
FASTQ = os.path.join(ROOT, "tests", "golden", "SRR5833294.10K.fastq.gz")
GUARD = 0x5A5A5A5A
SCAN_TILE, SUMS_PER_ROUND = 4096, 256  # a tile of the finish kernel; the tile sums one round of its middle launch takes


def depth_of(ids, n_kmers):
    """numpy: how often every id occurs among those that are not INVALID"""
    ids = np.asarray(ids, dtype=np.uint64)
    ids = ids[ids != INVALID]
    return np.bincount(ids.astype(np.int64), minlength=n_kmers).astype(np.uint32)


def truth_from_lookup(d, reads):
    per_read, _ = d.streaming_lookup(reads)
    return depth_of(np.concatenate([p.kmer_id for p in per_read] + [np.zeros(0, dtype=np.uint64)]), d.num_kmers())


def oracle_ids(oracle, reads, k):
    """per read the id of every k-mer by the oracle's point lookup (either strand); INVALID for a k-mer that holds anything but A, C, G,
    T in either case, and for one that is not in the dictionary"""
    ok = np.zeros(256, dtype=bool)
    ok[list(b"ACGTacgt")] = True
    out, kmers, where = [], [], []
    for i, r in enumerate(reads):
        b = np.frombuffer(r.encode("ascii", "replace") if isinstance(r, str) else bytes(r), dtype=np.uint8)
        out.append(np.full(max(0, b.size - k + 1), INVALID, dtype=np.uint64))
        if b.size < k:
            continue
        windows = np.lib.stride_tricks.sliding_window_view(b, k)
        valid = ok[windows].all(axis=1)
        kmers.append(windows[valid] & np.uint8(0xDF))  # (upper case)
        where.append((i, np.flatnonzero(valid)))
    if kmers:
        ids = oracle.lookup_ascii(np.ascontiguousarray(np.concatenate(kmers)).reshape(-1), True)["kmer_id"]
        at = 0
        for i, places in where:
            out[i][places] = ids[at:at + places.size]
            at += places.size
    return out


def runs_of(ids_per_read):
    """the stretches of consecutive ids along the reads -> (lo, n, backward, read) of each: what the kernel sees as runs. (A stretch
    that crosses from one string into the next counts as one here, and ids that go up and down by turns are cut at every turn; the kinds
    below only ask whether a kind of run is there at all.)"""
    flat = np.concatenate([np.append(ids, INVALID) for ids in ids_per_read])  # (an INVALID behind every read: no stretch goes on into the next)
    read = np.concatenate([np.full(ids.size + 1, r, dtype=np.int64) for r, ids in enumerate(ids_per_read)])
    hit = flat != INVALID
    step = np.zeros(flat.size, dtype=np.int8)  # how the id at j follows the id at j - 1: +1, -1, or not at all
    both = hit[1:] & hit[:-1]
    step[1:][both & (flat[1:] == flat[:-1] + np.uint64(1))] = 1
    step[1:][both & (flat[1:] + np.uint64(1) == flat[:-1])] = -1
    goes_on = step != 0
    goes_on[1:] &= ~((step[:-1] != 0) & (step[:-1] != step[1:]))
    first = np.flatnonzero(hit & ~goes_on)
    last = np.append(first[1:], flat.size)  # (one past; the places between a stretch and the next one's first are no hits)
    n = np.array([int(hit[a:b].sum()) for a, b in zip(first, last)], dtype=np.int64)
    backward = np.zeros(first.size, dtype=bool)
    more = n > 1
    backward[more] = step[first[more] + 1] < 0
    lo = np.where(backward, flat[first].astype(np.int64) - n + 1, flat[first].astype(np.int64))
    return lo, n, backward, read[first]


def upload(reads):
    import torch

    dev = torch.device("cuda", 0)
    blob = "".join(reads).encode()
    offsets = np.zeros(len(reads) + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum([len(r) for r in reads])
    return torch.frombuffer(bytearray(blob or b"\0"), dtype=torch.uint8).to(dev), torch.from_numpy(offsets.view(np.int64)).to(dev), len(blob)


def guarded(values, n, skew=0):
    """a device array of `skew` + n + 1 words of 32 bits: `skew` guard words, `values` (None: zeros), a guard word -> (tensor, pointer to
    the first value); skew = 1 puts the values at an address that is no multiple of 16"""
    import torch

    host = np.full(skew + n + 1, GUARD, dtype=np.uint32)
    host[skew:skew + n] = 0 if values is None else values
    t = torch.from_numpy(host.view(np.int32).copy()).to(torch.device("cuda", 0))
    return t, t.data_ptr() + 4 * skew


def unguard(t, n, skew, what):
    got = t.cpu().numpy().view(np.uint32)
    assert (got[:skew] == GUARD).all() and int(got[skew + n]) == GUARD, "a word outside the array was written: " + what
    return got[skew:skew + n].copy()


def device_finish(d, deltas, in_place, skew=0, stream=None):
    """sshash_depth_finish_device over `deltas` (host) -> depths; guard words around both arrays"""
    import torch

    n = d.num_kmers()
    t_in, p_in = guarded(deltas, n, skew)
    t_out, p_out = (t_in, p_in) if in_place else guarded(np.full(n, 0x77777777, dtype=np.uint32), n, skew)
    torch.cuda.synchronize()
    d.depth_finish_device(0, p_in, p_out, stream=0 if stream is None else stream.cuda_stream)
    (stream or torch.cuda.current_stream()).synchronize()
    torch.cuda.synchronize()
    if not in_place:
        assert (unguard(t_in, n, skew, "finish, input") == deltas).all(), "the deltas of an out-of-place finish were changed"
    return unguard(t_out, n, skew, "finish")


def device_depth(d, reads, before=None, report=None, stream=None, total_bases=None, in_place=True, skew=0):
    """the device entry points on device 0: the reads' deltas into an array that holds the deltas `before` (None: zeros), then the
    finish, in place or into a second array -> (depth, deltas, report or None); guard words around the arrays are asserted untouched"""
    import torch

    n = d.num_kmers()
    d_bases, d_off, n_bases = upload(reads)
    t, p = guarded(before, n, skew)
    d_report = None if report is None else torch.from_numpy(np.asarray(report, dtype=np.uint64).view(np.int64).copy()).to(torch.device("cuda", 0))
    torch.cuda.synchronize()  # (the copies run on torch's stream, the query may run on another)
    d.streaming_depth_device(0, d_bases.data_ptr(), d_off.data_ptr(), len(reads), p, d_report=0 if d_report is None else d_report.data_ptr(),
                             stream=0 if stream is None else stream.cuda_stream, total_bases=n_bases if total_bases is None else total_bases)
    (stream or torch.cuda.current_stream()).synchronize()
    torch.cuda.synchronize()
    deltas = unguard(t, n, skew, "the depth form of the run kernel")
    depth = device_finish(d, deltas, in_place, skew, stream)
    return depth, deltas, None if d_report is None else d_report.cpu().numpy().view(np.uint64)


def device_string_sums(d, depth):
    import torch

    dev = torch.device("cuda", 0)
    d_depth = torch.from_numpy(depth.view(np.int32).copy()).to(dev)
    d_sums = torch.full((d.num_strings() + 2,), -3, dtype=torch.int64, device=dev)  # sums, the total, a guard
    torch.cuda.synchronize()
    d.depth_string_sums_device(0, d_depth.data_ptr(), d_sums.data_ptr(), d_sums.data_ptr() + 8 * d.num_strings())
    torch.cuda.synchronize()
    out = d_sums.cpu().numpy()
    assert out[-1] == -3, "the word behind the total was written"
    return out[:-2].view(np.uint64), int(out[-2].view(np.uint64))


def same(got, want, what):
    assert got.dtype == np.uint32 and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (what, "ids", bad[:5].tolist(), got[bad[:5]].tolist(), want[bad[:5]].tolist())


def shards_main(fasta, k, m, canonical):
    """two minimizer shards: each counts the k-mers it owns under the ids of the whole index; their arrays added are the whole index's"""
    import sshash_amd
    from oracle.ground_truth import read_fasta_sequences

    sequences = read_fasta_sequences(fasta, k)
    whole = sshash_amd.Dictionary.build(fasta, k=k, m=m, canonical=canonical, num_threads=4).to_device(0)
    reads, repeated = make_reads(whole, sequences, k)
    reads = reads[::3] + repeated[:64]
    want = truth_from_lookup(whole, reads)
    got, rep = whole.streaming_depth(reads)
    same(got, want, "the whole index")
    total = np.zeros(whole.num_kmers(), dtype=np.uint32)
    positive, parts = 0, []
    for r in range(2):
        shard = sshash_amd.Dictionary.build(fasta, k=k, m=m, canonical=canonical, num_threads=4, num_shards=2, shard_id=r).to_device(0)
        assert shard.num_kmers() == whole.num_kmers()
        part, shard_rep = shard.streaming_depth(reads)
        assert int(part.sum(dtype=np.uint64)) == shard_rep.num_positive_kmers > 0
        try:  # (the run kernel would follow an owned k-mer's run through k-mers of the other shard: the device call refuses)
            shard.streaming_depth_device(0, 0, 0, 1, 0)
            raise AssertionError("the device call on a minimizer shard did not refuse")
        except sshash_amd.SSHashError as e:
            assert e.status == 1, e
        shard.streaming_depth(reads, depth=total)  # (added into)
        positive += shard_rep.num_positive_kmers
        parts.append(part)
    assert ((parts[0] != 0) & (parts[1] == 0)).any() and ((parts[1] != 0) & (parts[0] == 0)).any(), "both shards own k-mers of the reads"
    same(total, want, "the shards' arrays added")
    assert positive == rep.num_positive_kmers
    print(json.dumps({"ok": True, "shards": 2, "positive": positive, "num_kmers": whole.num_kmers()}))


def main():
    import torch

    import sshash_amd
    from oracle import oracle as O
    from oracle.ground_truth import read_fasta_sequences

    fasta, k, m, canonical, scratch = sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), bool(int(sys.argv[4])), sys.argv[5]
    if len(sys.argv) > 6 and sys.argv[6] == "shards":
        return shards_main(fasta, k, m, canonical)
    d = sshash_amd.Dictionary.build(fasta, k=k, m=m, canonical=canonical, num_threads=4)
    sequences = read_fasta_sequences(fasta, k)
    n_kmers = d.num_kmers()
    reads, repeated = make_reads(d, sequences, k)
    everything = reads + repeated

    # ---- on the CPU, before anything runs on the GPU: the oracle's depth, and that the reads hold every kind of run ----
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "w.sshash")
        d.save(path)
        oracle = O.OracleIndex(path)
        ids_per_read = oracle_ids(oracle, reads, k)
        hot_ids = oracle_ids(oracle, repeated[:1], k)[0]
    want_oracle = depth_of(np.concatenate(ids_per_read), n_kmers)
    want_hot = depth_of(hot_ids, n_kmers) * np.uint32(len(repeated))
    lo, n, backward, read_of_run = runs_of(ids_per_read)
    lengths = np.array([len(r) for r in reads])
    hits = np.array([int((ids != INVALID).sum()) for ids in ids_per_read])
    runs_per_read = np.bincount(read_of_run, minlength=len(reads))
    kinds = {"backward": int(backward.sum()), "forward": int((~backward & (n > 1)).sum()), "runs_of_one": int((n == 1).sum()),
             "runs_of_64_and_more": int((n >= 64).sum()), "runs_from_id_0": int((lo == 0).sum()),
             "runs_to_the_last_id": int((lo + n == n_kmers).sum()),  # (the -1 that is dropped)
             "reads_with_N": sum("N" in r for r in reads), "reads_shorter_than_k": int((lengths < k).sum()), "empty_reads": int((lengths == 0).sum()),
             "reads_without_a_hit": int(((lengths >= k) & (hits == 0)).sum()), "reads_with_cut_runs": int((runs_per_read >= 2).sum()),
             "ids_never_held": int((want_oracle == 0).sum()), "ids_held_once": int((want_oracle == 1).sum()), "ids_held_twice_and_more": int((want_oracle >= 2).sum()),
             "ids_held_4096_times_and_more": int((want_hot >= 4096).sum())}
    assert all(v > 0 for v in kinds.values()), kinds
    assert len(repeated) == 4096 and len(set(repeated)) == 1 and kinds["ids_held_4096_times_and_more"] == 101
    finish_rounds = -(-(-(-n_kmers // SCAN_TILE)) // SUMS_PER_ROUND)  # rounds of the finish's middle launch: the caller says how many it expects
    assert n_kmers % SCAN_TILE and n_kmers % 16, "a last tile, and a last lane, that are not full"

    # ---- the same truth from streaming_lookup on the GPU ----
    d.to_device(0)
    st = d.device_stats(0)
    want = truth_from_lookup(d, reads)
    same(want, want_oracle, "streaming_lookup against the oracle's point lookups")
    same(truth_from_lookup(d, repeated[:1]) * np.uint32(4096), want_hot, "the repeated read")

    # ---- the depth, host and device; the report; the cover ----
    want_report = report_row(d.streaming_query(reads))
    got, rep = d.streaming_depth(reads)
    same(got, want, "host call")
    assert (report_row(rep) == want_report).all(), ("host report", report_row(rep), want_report)
    assert int(got.sum(dtype=np.uint64)) == rep.num_positive_kmers
    cover, _ = d.streaming_cover(reads)
    assert (sshash_amd.cover_to_ids(cover) == np.flatnonzero(got).astype(np.uint64)).all(), "(depth != 0) against the bits of streaming_cover"
    got, deltas, rep = device_depth(d, reads, report=[0] * 6, in_place=True)
    same(got, want, "device call, finished in place")
    assert (rep == want_report).all(), ("device report", rep, want_report)
    assert (deltas != 0).sum() <= 2 * int(want_report[4]), "at most two deltas a run"
    same(np.cumsum(deltas, dtype=np.uint32), want, "the deltas' prefix sum in numpy")
    got, _, rep = device_depth(d, reads, report=[1, 2, 3, 4, 5, 6], stream=torch.cuda.Stream(device=0), total_bases=0, in_place=False)
    same(got, want, "device call on a side stream, finished out of place")
    assert (rep == want_report + np.arange(1, 7, dtype=np.uint64)).all(), "the report is accumulated into"
    got, _, _ = device_depth(d, reads, in_place=True, skew=1)  # a NULL report; arrays at an address that is no multiple of 16
    same(got, want, "device call, arrays not 16-byte aligned, in place")
    got, _, _ = device_depth(d, reads, in_place=False, skew=3)
    same(got, want, "device call, arrays not 16-byte aligned, out of place")

    # ---- the same read 4096 times: many lanes add to the same two words ----
    got, deltas, _ = device_depth(d, repeated)
    same(got, want_hot, "one read 4096 times, device call")
    assert sorted(deltas[deltas != 0].tolist()) == sorted([4096, (1 << 32) - 4096])
    got, rep = d.streaming_depth(everything)
    same(got, want + want_hot, "all reads and the repeated one, host call")
    assert int(got.sum(dtype=np.uint64)) == rep.num_positive_kmers

    # ---- accumulation and bounds ----
    rng = np.random.default_rng(5)
    before = rng.integers(0, 1 << 32, n_kmers, dtype=np.uint64).astype(np.uint32)
    before[rng.random(n_kmers) < 0.5] = 0
    mine = before.copy()
    got, _ = d.streaming_depth(reads, depth=mine)
    assert got is mine
    same(mine, before + want, "a host array that held values keeps them added (modulo 2^32)")
    half = len(reads) // 2
    want_a, want_b = truth_from_lookup(d, reads[:half]), truth_from_lookup(d, reads[half:])
    assert (want_a != 0).any() and (want_b != 0).any()
    same(want_a + want_b, want, "the two halves' truth")
    got_a, deltas_a, _ = device_depth(d, reads[:half])
    same(got_a, want_a, "first batch, device call")
    got, _, _ = device_depth(d, reads[half:], before=deltas_a)
    same(got, want, "two batches into one delta array, device call")
    two, _ = d.streaming_depth(reads[:half])
    d.streaming_depth(reads[half:], depth=two)
    same(two, want, "two batches into one array, host call")
    # no reads at all, and reads without a base
    d.streaming_depth_device(0, 0, 0, 0, 0)
    got, deltas, rep = device_depth(d, ["", "", ""], before=deltas_a, report=[1] * 6, total_bases=0)
    assert (deltas == deltas_a).all(), "reads without a base"
    same(got, want_a, "reads without a base, finished")
    assert (rep == 1).all()

    # ---- geometry independence: the test hooks of the run kernel and of the host call's pieces ----
    for hook in ("stream_move_out_every=1", "stream_move_out_every=7", "stream_move_out_every=300", "stream_piece_reads=300", "stream_piece_reads=257"):
        os.environ["SSHASH_AMD_TEST_HOOKS"] = hook
        got, rep = d.streaming_depth(reads)
        assert got.tobytes() == want.tobytes() and (report_row(rep) == want_report).all(), hook
        got, _, rep = device_depth(d, reads, report=[0] * 6)
        assert got.tobytes() == want.tobytes() and (rep == want_report).all(), hook
    del os.environ["SSHASH_AMD_TEST_HOOKS"]

    # ---- a read above 2^16 bases: the host call's position-parallel route against the same bases cut into short reads ----
    parts, size = [], 0
    order = np.random.default_rng(9).permutation(len(sequences))
    while size <= 70000:  # (strings come more than once, on either strand: depths of two and more, ids that go up, down and up again)
        for i in order[:12]:
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
    want_long = truth_from_lookup(d, pieces + reads[:40])
    assert (want_long >= 2).any() and (want_long == 1).any()
    got, rep_pieces = d.streaming_depth(pieces + reads[:40])
    same(got, want_long, "the pieces of the long read, host call")
    got, rep = d.streaming_depth(reads[:20] + [long_read, ""] + reads[20:40])
    same(got, want_long, "a batch that holds a read above 2^16 bases, host call")
    assert rep.num_positive_kmers == rep_pieces.num_positive_kmers == int(want_long.sum(dtype=np.uint64)) and rep.num_kmers == rep_pieces.num_kmers
    got, _, _ = device_depth(d, [long_read])  # (the device call: one lane walks it)
    same(got, truth_from_lookup(d, pieces), "the long read, device call")

    # ---- query files ----
    with gzip.open(FASTQ, "rt") as f:
        fastq_reads = [line.strip() for i, line in enumerate(f) if i % 4 == 1]
    assert len(fastq_reads) == 10000
    want_fastq = truth_from_lookup(d, fastq_reads)
    got, want_fastq_report = d.streaming_depth(fastq_reads)
    same(got, want_fastq, "the FASTQ file's parsed reads")
    os.environ["SSHASH_AMD_TEST_HOOKS"] = "query_batch_bases=200000"  # (batch seams inside the file: the deltas stay on the device across them)
    got, rep = d.streaming_depth_from_file(FASTQ)
    del os.environ["SSHASH_AMD_TEST_HOOKS"]
    same(got, want_fastq, "the FASTQ file in many batches")
    assert rep == want_fastq_report, (rep, want_fastq_report)
    fasta_reads = [sequences[int(i)] for i in order[:400]]
    own = os.path.join(scratch, f"own_strings_k{k}_{int(canonical)}.fa")
    with open(own, "w") as f:
        for i, s in enumerate(fasta_reads):
            f.write(f">{i}\n{s}\n")
    want_fasta = truth_from_lookup(d, fasta_reads)
    assert int(want_fasta.sum(dtype=np.uint64)) == sum(len(s) - k + 1 for s in fasta_reads), "every k-mer of the dictionary's own strings is found"
    got, rep = d.streaming_depth_from_file(own, depth=before.copy())
    same(got, want_fasta + before, "the FASTA file against its parsed reads, into an array that held values")
    assert rep.num_positive_kmers == int(want_fasta.sum(dtype=np.uint64))

    # ---- the finish alone, on deltas of the test's own ----
    wrap = np.zeros(n_kmers, dtype=np.uint32)
    wrap[0], wrap[1] = 0xFFFFFFF0, 0x20
    got = device_finish(d, wrap, in_place=True)
    assert got[0] == 0xFFFFFFF0 and got[1] == 0x10 and (got[1:] == 0x10).all(), "the intermediate value wraps, the result is exact"
    ends = np.zeros(n_kmers, dtype=np.uint32)
    ends[0], ends[-1] = 1, 0xFFFFFFFF
    got = device_finish(d, ends, in_place=False)
    assert (got[:-1] == 1).all() and got[-1] == 0, "+1 in the first word, -1 in the last"
    noise = np.random.default_rng(31).integers(0, 1 << 32, n_kmers, dtype=np.uint64).astype(np.uint32)
    for in_place, skew in ((True, 0), (False, 0), (True, 1), (False, 2)):
        same(device_finish(d, noise, in_place, skew), np.cumsum(noise, dtype=np.uint32), f"random deltas, in place {in_place}, skew {skew}")

    # ---- depth per string ----
    for name, depth in (("reads", want), ("repeated", want + want_hot), ("noise", noise), ("zero", np.zeros(n_kmers, dtype=np.uint32)),
                        ("all ones", np.full(n_kmers, 0xFFFFFFFF, dtype=np.uint32))):
        host_sums, host_total = d.depth_string_sums(depth)
        sums, total = device_string_sums(d, depth)
        assert sums.shape == host_sums.shape and (sums == host_sums).all(), ("sums per string of " + name, np.flatnonzero(sums != host_sums)[:5])
        assert total == host_total == int(depth.sum(dtype=np.uint64)), (name, total, host_total)

    print(json.dumps({"ok": True, "reads": len(reads), "positive": int(want.sum(dtype=np.uint64)), "held": int((want != 0).sum()), "num_kmers": n_kmers,
                      "sk_slots": st["sk_slots"], "finish_rounds": finish_rounds, "kinds": kinds}))


if __name__ == "__main__":
    main()
