#!/usr/bin/env python
"""Worker of tests/test_gpu_streaming_sums.py: one process = one dictionary and one setting of the environment switch that decides
whether a replica holds the super-k-mer table (SSHASH_AMD_SKTABLE=0: the run kernel takes the complete seed() path). Everything the
streaming sums promise -- per read, the sum of a value per k-mer over the read's positive k-mers, and their number -- against ground
truth that shares no code with the kernel: values[ids].sum() and (ids valid).sum() per read over the kmer_id values of
streaming_lookup, and the same over the CPU oracle's point lookups of every k-mer of every read. All comparisons are exact. The
oracle's ids also say, before anything runs on the GPU, that the reads hold every kind of read and of run the kernel has a branch for.
Prints one JSON line; any mismatch is an assertion error.

    python tests/gpu_sums_worker.py <k31|k63> <canonical 0|1> <scratch directory> [shards|weighted]"""
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import numpy as np

from gpu_depth_worker import oracle_ids, upload
from gpu_per_read_worker import random_dna, report_row, revcomp

INVALID = np.uint64(0xFFFFFFFFFFFFFFFF)
GUARD = 0x5A5A5A5A5A5A5A5A
GARBAGE = 0x7777777777777777
SCAN_TILE = 4096
ALL_ONES = 0xFFFFFFFF


def dictionary_input(which, canonical, scratch):
    """-> (fasta, sequences, k, m). k31: conftest.skewed_sequences(31, 11) and one random string of 10,000 bases, whose ids cross two
    tiles of the scan; k63: the 24 strings of the golden k = 63 file."""
    from conftest import K63_FASTA, skewed_sequences
    from oracle.ground_truth import read_fasta_sequences

    if which == "k63":
        return K63_FASTA, read_fasta_sequences(K63_FASTA, 63), 63, 25
    sequences = skewed_sequences(31, 11, seed=5 if canonical else 3) + [random_dna(np.random.default_rng(41), 10000)]
    fasta = os.path.join(scratch, f"sums_k31_{int(canonical)}.fa")
    with open(fasta, "w") as f:
        for s in sequences:
            f.write(">\n" + s + "\n")
    return fasta, sequences, 31, 11


def substitute(rng, s, places):
    s = list(s)
    for at in places:
        s[at] = "ACGT"[("ACGT".index(s[at].upper()) + 1 + int(rng.integers(0, 3))) % 4]
    return "".join(s)


def whole_long_string(sequences):
    """the longest string that one lane still walks in a host call (the one read above 2^16 bases is made on purpose)"""
    return max((s for s in sequences if len(s) <= 60000), key=len)


def make_reads(sequences, k):
    """-> (reads, index of the read above 2^16 bases); some 2,000 reads of every kind the issue lists"""
    rng = np.random.default_rng(23)
    lengths = np.array([len(s) for s in sequences])
    weights = (lengths - k + 1) / (lengths - k + 1).sum()
    reads = []
    for j in range(1500):  # samples of 100 .. 300 bases (shorter where the string is), either strand
        s = sequences[int(rng.choice(len(sequences), p=weights))]
        n = min(len(s), int(rng.integers(100, 301)))
        a = int(rng.integers(0, len(s) - n + 1))
        r = s[a:a + n]
        if j % 2:
            r = revcomp(r)
        if j % 5 == 0 and n > k + 2:  # substitutions that cut runs
            r = substitute(rng, r, sorted(set(int(x) for x in rng.integers(0, n, 2))))
        if j % 50 == 7:
            r = r[:n // 2] + "N" + r[n // 2 + 1:]
        if j % 50 == 8:
            r = r.lower()
        reads.append(r)
    longest = whole_long_string(sequences)
    reads += [longest, revcomp(longest)]  # a whole long string as one read
    first, last = sequences[0], sequences[-1]
    reads += [first[:k + 130], revcomp(first[:k + 70]), last[-(k + 130):], revcomp(last[-(k + 70):])]  # k-mer id 0 and id num_kmers - 1
    for j in range(60):  # reads of exactly k bases
        s = sequences[int(rng.choice(len(sequences), p=weights))]
        a = int(rng.integers(0, len(s) - k + 1))
        reads.append(s[a:a + k] if j % 2 else revcomp(s[a:a + k]))
    for j in range(150):
        reads.append(random_dna(rng, int(rng.integers(0, k))))  # shorter than k
    reads += ["", "", "N" * 40, "A" * (k - 1)]
    for j in range(250):
        reads.append(random_dna(rng, int(rng.integers(k, 300))))  # random: no hit
    parts, size, j = [], 0, 0
    order = np.argsort(-lengths)
    while size <= (1 << 16) + 1000:  # whole strings joined by N, either strand, until the read is above 2^16 bases
        s = sequences[int(order[j % len(order)])]
        parts.append(revcomp(s) if (j // len(order) + j) % 2 else s)
        size += len(parts[-1]) + 1
        j += 1
    long_at = len(reads) // 2
    reads.insert(long_at, "N".join(parts))
    return reads, long_at


def flat_ids(ids_per_read):
    read = np.concatenate([np.full(ids.size, r, dtype=np.int64) for r, ids in enumerate(ids_per_read)] + [np.zeros(0, dtype=np.int64)])
    ids = np.concatenate(list(ids_per_read) + [np.zeros(0, dtype=np.uint64)])
    hit = ids != INVALID
    return read[hit], ids[hit].astype(np.int64)


def rows_of(flat, n_reads, values, at_least=0):
    """numpy: per read (sum of the value of every hit, number of hits)"""
    import sshash_amd

    read, ids = flat
    v = values.astype(np.uint64) if at_least == 0 else (values >= np.uint32(at_least)).astype(np.uint64)
    out = np.zeros(n_reads, dtype=sshash_amd.READ_SUM_DTYPE)
    np.add.at(out["sum"], read, v[ids])
    np.add.at(out["positive_kmers"], read, np.uint64(1))
    return out


def same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    bad = np.flatnonzero((got["sum"] != want["sum"]) | (got["positive_kmers"] != want["positive_kmers"]))
    assert bad.size == 0, (what, "reads", bad[:5].tolist(), got[bad[:5]].tolist(), want[bad[:5]].tolist())


def device_prefix(d, values, at_least=0, stream=None):
    """sshash_value_prefix_device over `values` (host) -> (device tensor that holds a guard word, the prefix, a guard word; pointer to the
    prefix); the prefix is compared with numpy.cumsum in 64 bits, the guards and the values are asserted untouched"""
    import torch

    dev = torch.device("cuda", 0)
    n = d.num_kmers()
    host = np.full(n + 3, GUARD, dtype=np.uint64)
    host[1:n + 2] = GARBAGE
    t = torch.from_numpy(host.view(np.int64).copy()).to(dev)
    guarded_values = np.full(n + 2, 0x5A5A5A5A, dtype=np.uint32)
    guarded_values[1:n + 1] = values
    d_values = torch.from_numpy(guarded_values.view(np.int32).copy()).to(dev)
    torch.cuda.synchronize()
    d.value_prefix_device(0, d_values.data_ptr() + 4, t.data_ptr() + 8, at_least=at_least, stream=0 if stream is None else stream.cuda_stream)
    (stream or torch.cuda.current_stream()).synchronize()
    torch.cuda.synchronize()
    got = t.cpu().numpy().view(np.uint64)
    assert int(got[0]) == GUARD and int(got[n + 2]) == GUARD, "a word outside the prefix was written"
    assert (d_values.cpu().numpy().view(np.uint32) == guarded_values).all(), "the values were changed"
    v = values.astype(np.uint64) if at_least == 0 else (values >= np.uint32(at_least)).astype(np.uint64)
    want = np.zeros(n + 1, dtype=np.uint64)
    np.cumsum(v, dtype=np.uint64, out=want[1:])
    bad = np.flatnonzero(got[1:n + 2] != want)
    assert bad.size == 0, ("prefix", at_least, bad[:5].tolist(), got[1:n + 2][bad[:5]].tolist(), want[bad[:5]].tolist())
    assert int(got[1]) == 0 and int(got[n + 1]) == int(v.sum(dtype=np.uint64)), "word 0 and the total"
    return t, t.data_ptr() + 8


def device_sums(d, reads, p_prefix, report=None, stream=None, total_bases=None):
    """the device entry point on device 0 over rows that held garbage, at an address that is a multiple of 8 and not of 16, a guard word
    on either side -> (rows, report or None)"""
    import torch

    import sshash_amd

    dev = torch.device("cuda", 0)
    n = len(reads)
    d_bases, d_off, n_bases = upload(reads)
    host = np.full(2 * n + 2, GARBAGE, dtype=np.uint64)
    host[0] = host[-1] = GUARD
    t = torch.from_numpy(host.view(np.int64).copy()).to(dev)
    p = t.data_ptr() + 8
    assert p % 8 == 0 and p % 16 != 0
    d_report = None if report is None else torch.from_numpy(np.asarray(report, dtype=np.uint64).view(np.int64).copy()).to(dev)
    torch.cuda.synchronize()  # (the copies run on torch's stream, the query may run on another)
    d.streaming_sums_device(0, d_bases.data_ptr(), d_off.data_ptr(), n, p_prefix, p, d_report=0 if d_report is None else d_report.data_ptr(),
                            stream=0 if stream is None else stream.cuda_stream, total_bases=n_bases if total_bases is None else total_bases)
    (stream or torch.cuda.current_stream()).synchronize()
    torch.cuda.synchronize()
    got = t.cpu().numpy().view(np.uint64)
    assert int(got[0]) == GUARD and int(got[-1]) == GUARD, "a word outside sums[0 .. num_reads) was written"
    rows = got[1:-1].copy().view(sshash_amd.READ_SUM_DTYPE)
    return rows, None if d_report is None else d_report.cpu().numpy().view(np.uint64)


def build(which, canonical, scratch, **kw):
    import sshash_amd

    fasta, sequences, k, m = dictionary_input(which, canonical, scratch)
    return sshash_amd.Dictionary.build(fasta, k=k, m=m, canonical=canonical, num_threads=4, **kw), sequences, k


def shards_main(which, canonical, scratch):
    """two minimizer shards: each adds the k-mers it owns, so the shards' rows added together are the rows of the whole index"""
    import sshash_amd

    whole, sequences, k = build(which, canonical, scratch)
    whole.to_device(0)
    reads, _ = make_reads(sequences, k)
    values = np.random.default_rng(7).integers(0, 1000, whole.num_kmers()).astype(np.uint32)
    per_read, _ = whole.streaming_lookup(reads)
    want = rows_of(flat_ids([p.kmer_id for p in per_read]), len(reads), values)
    got, rep = whole.streaming_sums(reads, values)
    same(got, want, "the whole index")
    total = np.zeros(len(reads), dtype=sshash_amd.READ_SUM_DTYPE)
    parts = []
    for r in range(2):
        shard, _, _ = build(which, canonical, scratch, num_shards=2, shard_id=r)
        shard.to_device(0)
        assert shard.num_kmers() == whole.num_kmers()
        part, shard_rep = shard.streaming_sums(reads, values)
        assert int(part["positive_kmers"].sum(dtype=np.uint64)) == shard_rep.num_positive_kmers > 0
        try:  # (the run kernel would follow an owned k-mer's run through k-mers of the other shard: the device call refuses)
            shard.streaming_sums_device(0, 8, 8, 1, 8, 8)
            raise AssertionError("the device call on a minimizer shard did not refuse")
        except sshash_amd.SSHashError as e:
            assert e.status == 1 and "minimizer shard" in str(e), e
        total["sum"] += part["sum"]
        total["positive_kmers"] += part["positive_kmers"]
        parts.append(part)
    only_0 = (parts[0]["positive_kmers"] != 0) & (parts[1]["positive_kmers"] == 0)
    only_1 = (parts[1]["positive_kmers"] != 0) & (parts[0]["positive_kmers"] == 0)
    both = (parts[0]["positive_kmers"] != 0) & (parts[1]["positive_kmers"] != 0)
    assert both.any() and (only_0.any() or only_1.any()), "reads whose k-mers lie in both shards, and reads of one shard alone"
    same(total, want, "the shards' rows added")
    print(json.dumps({"ok": True, "shards": 2, "positive": int(rep.num_positive_kmers), "num_kmers": whole.num_kmers()}))


def weighted_main(which, canonical, scratch):
    """a depth array -> write_weighted_fasta -> a weighted build: streaming_sums without values reads the weights, which are the depths"""
    import sshash_amd

    d, sequences, k = build(which, canonical, scratch)
    d.to_device(0)
    reads, _ = make_reads(sequences, k)
    try:
        d.streaming_sums(reads)
        raise AssertionError("values=None on a dictionary without weights did not raise")
    except ValueError:
        pass
    depth, _ = d.streaming_depth(reads)
    assert (depth >= 2).any() and np.unique(depth).size > 2  # (the read of whole strings holds every k-mer: no zero among them)
    path = os.path.join(scratch, "sums_weighted.fa")
    sshash_amd.write_weighted_fasta(d, depth, path)
    w = sshash_amd.Dictionary.build(path, k=d.k(), m=d.m(), canonical=d.canonical(), weighted=True).to_device(0)
    assert w.weighted() and w.num_kmers() == d.num_kmers()
    by_weights, rep_w = w.streaming_sums(reads)
    by_depth, rep_d = w.streaming_sums(reads, depth)
    same(by_weights, by_depth, "the weights of the weighted build against the depth array they were written from")
    per_read, _ = w.streaming_lookup(reads)
    same(by_depth, rows_of(flat_ids([p.kmer_id for p in per_read]), len(reads), depth), "the depth array against the truth")
    assert rep_w == rep_d and int(by_weights["sum"].sum(dtype=np.uint64)) > rep_w.num_positive_kmers > 0
    solid, _ = w.streaming_sums(reads, at_least=2)
    same(solid, rows_of(flat_ids([p.kmer_id for p in per_read]), len(reads), depth, 2), "solid k-mers out of the weights")
    print(json.dumps({"ok": True, "weighted": True, "positive": int(rep_w.num_positive_kmers), "num_kmers": w.num_kmers()}))


def main():
    import torch

    import sshash_amd
    from oracle import oracle as O

    which, canonical, scratch = sys.argv[1], bool(int(sys.argv[2])), sys.argv[3]
    mode = sys.argv[4] if len(sys.argv) > 4 else ""
    if mode == "shards":
        return shards_main(which, canonical, scratch)
    if mode == "weighted":
        return weighted_main(which, canonical, scratch)
    d, sequences, k = build(which, canonical, scratch)
    n_kmers = d.num_kmers()
    reads, long_at = make_reads(sequences, k)
    n = len(reads)
    short_reads = reads[:long_at] + reads[long_at + 1:]
    lengths = np.array([len(r) for r in reads])

    # ---- on the CPU, before anything runs on the GPU: the oracle's ids, and that the reads hold every kind the kernel has a branch for ----
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "w.sshash")
        d.save(path)
        oracle_per_read = oracle_ids(O.OracleIndex(path), reads, k)
    hits = np.array([int((ids != INVALID).sum()) for ids in oracle_per_read])
    flat_all = np.concatenate([np.append(ids, INVALID) for ids in oracle_per_read])
    both = (flat_all[1:] != INVALID) & (flat_all[:-1] != INVALID)
    up = both & (flat_all[1:] == flat_all[:-1] + np.uint64(1))
    down = both & (flat_all[1:] + np.uint64(1) == flat_all[:-1])
    valid = flat_all[flat_all != INVALID].astype(np.int64)
    longest = len(whole_long_string(sequences))
    cut = 0  # reads where a hit follows a miss that follows a hit: a run was cut
    for ids in oracle_per_read[:1500]:
        h = np.flatnonzero(ids != INVALID)
        cut += bool(h.size and (np.diff(h) > 1).any())
    kinds = {"forward_steps": int(up.sum()), "backward_steps": int(down.sum()), "id_0": int((valid == 0).sum()), "last_id": int((valid == n_kmers - 1).sum()),
             "reads_of_k_bases_found": int(((lengths == k) & (hits == 1)).sum()), "reads_with_cut_runs": cut,
             "reads_with_N": sum("N" in r for r in reads), "reads_shorter_than_k": int((lengths < k).sum()), "empty_reads": int((lengths == 0).sum()),
             "reads_without_a_hit": int(((lengths >= k) & (hits == 0)).sum()), "whole_long_string": int((hits == longest - k + 1).sum()),
             "reads_above_2_16": int((lengths > (1 << 16)).sum())}
    assert all(v > 0 for v in kinds.values()), kinds
    assert kinds["reads_above_2_16"] == 1 and lengths[long_at] > (1 << 16) and 1800 <= n <= 2200, (kinds, n)
    if which == "k31":  # the whole long string: one run of ids over two tile boundaries of the scan
        assert longest - k + 1 > 2 * SCAN_TILE and n_kmers % SCAN_TILE
    flat = flat_ids(oracle_per_read)

    # ---- the same truth from streaming_lookup on the GPU ----
    d.to_device(0)
    st = d.device_stats(0)
    per_read, _ = d.streaming_lookup(reads)
    assert all((p.kmer_id == o).all() for p, o in zip(per_read, oracle_per_read)), "streaming_lookup against the oracle's point lookups"
    want_report = report_row(d.streaming_query(reads))
    want_short_report = report_row(d.streaming_query(short_reads))
    per_read_rows, _ = d.streaming_query_per_read(reads)

    rng = np.random.default_rng(7)
    random_values = rng.integers(0, 1000, n_kmers).astype(np.uint32)
    cases = [("random", random_values, 0), ("all ones", np.full(n_kmers, ALL_ONES, dtype=np.uint32), 0), ("ones", np.ones(n_kmers, dtype=np.uint32), 0),
             ("at least 1", random_values, 1), ("at least 500", random_values, 500), ("at least all ones", random_values, ALL_ONES)]
    drop = lambda rows: np.concatenate([rows[:long_at], rows[long_at + 1:]])
    for name, values, at_least in cases:
        want = rows_of(flat, n, values, at_least)
        assert (want["positive_kmers"] == per_read_rows[:, 1]).all(), "positive_kmers against column 1 of streaming_query_per_read"
        if name == "all ones":
            assert int(want["sum"].max()) > (1 << 32)
        if name == "ones":
            assert (want["sum"] == want["positive_kmers"]).all()
        # the host call: with the long read its piece takes the per-k-mer route (segments are off), without it the run kernel
        got, rep = d.streaming_sums(reads, values, at_least)
        same(got, want, name + ": host call, per-k-mer route")
        assert (report_row(rep) == want_report).all(), (name, report_row(rep), want_report)
        got, rep = d.streaming_sums(short_reads, values, at_least)
        same(got, drop(want), name + ": host call, run kernel")
        assert (report_row(rep) == want_short_report).all(), (name, report_row(rep), want_short_report)
        # the device calls: the prefix, then the sums form of the run kernel (one lane walks the long read)
        t_prefix, p_prefix = device_prefix(d, values, at_least)
        got, rep = device_sums(d, reads, p_prefix, report=[0] * 6)
        same(got, want, name + ": device call")
        assert (rep == want_report).all(), (name, rep, want_report)
    want = rows_of(flat, n, random_values)
    t_prefix, p_prefix = device_prefix(d, random_values, stream=torch.cuda.Stream(device=0))
    got, rep = device_sums(d, reads, p_prefix, report=[1, 2, 3, 4, 5, 6], stream=torch.cuda.Stream(device=0), total_bases=0)
    same(got, want, "device call on a side stream, total_bases = 0")
    assert (rep == want_report + np.arange(1, 7, dtype=np.uint64)).all(), "the report is accumulated into"
    got, rep = device_sums(d, reads, p_prefix)  # a NULL report
    same(got, want, "device call, no report")
    # no reads at all, and reads without a base: rows of zeros over what was garbage
    d.streaming_sums_device(0, 0, 0, 0, 0, 0)
    got, rep = device_sums(d, ["", "", ""], p_prefix, report=[1] * 6, total_bases=0)
    assert (got["sum"] == 0).all() and (got["positive_kmers"] == 0).all() and (rep == 1).all(), "reads without a base"
    empty, _ = d.streaming_sums([], random_values)
    assert empty.shape == (0,)

    # ---- geometry independence: the test hooks of the run kernel and of the host call's pieces ----
    for hook in ("stream_move_out_every=1", "stream_move_out_every=7", "stream_piece_reads=300", "stream_piece_reads=257"):
        os.environ["SSHASH_AMD_TEST_HOOKS"] = hook
        got, rep = d.streaming_sums(reads, random_values)  # (pieces of 300 reads: the long read's piece by ids, the others by the run kernel)
        assert got.tobytes() == want.tobytes() and (report_row(rep) == want_report).all(), hook
        got, rep = device_sums(d, reads, p_prefix, report=[0] * 6)
        assert got.tobytes() == want.tobytes() and (rep == want_report).all(), hook
    # five pieces of four reads, the third without a base: nothing is launched for it, and its rows come back as zeros at their reads
    os.environ["SSHASH_AMD_TEST_HOOKS"] = "stream_piece_reads=4"
    picks = [i for i in range(n) if i != long_at and lengths[i] >= k][:16]
    assert hits[picks[:8]].sum() > 0 and hits[picks[8:]].sum() > 0
    got, rep = d.streaming_sums([reads[i] for i in picks[:8]] + [""] * 4 + [reads[i] for i in picks[8:]], random_values)
    want_batch = np.concatenate([want[picks[:8]], np.zeros(4, dtype=want.dtype), want[picks[8:]]])
    assert got.tobytes() == want_batch.tobytes() and (report_row(rep) == per_read_rows[picks].sum(0)).all(), "a piece of reads without a base"
    del os.environ["SSHASH_AMD_TEST_HOOKS"]

    # ---- segments: many lanes add into one row ----
    launches = d.read_segments()["segmented_launches"]
    assert launches == 0
    for S in (1, 7, 64):
        d.set_read_segments(S, device_calls=True)
        got, rep = device_sums(d, reads, p_prefix, report=[0] * 6)
        assert got.tobytes() == want.tobytes() and (rep == want_report).all(), ("segments, device call", S)
        assert d.read_segments()["segmented_launches"] == launches + 1
        got, rep = d.streaming_sums(reads, random_values)
        assert got.tobytes() == want.tobytes() and (report_row(rep) == want_report).all(), ("segments, host call", S)
        launches = d.read_segments()["segmented_launches"]
        assert launches >= 2
    d.set_read_segments()  # the default S, host calls only: the long read's piece goes over segments
    got, rep = d.streaming_sums(reads, random_values)
    assert got.tobytes() == want.tobytes() and (report_row(rep) == want_report).all(), "the long read at the default S"
    assert d.read_segments()["segmented_launches"] == launches + 1
    d.set_read_segments(sshash_amd.SEGMENTS_OFF)
    got, rep = d.streaming_sums([reads[long_at]], random_values)  # segments off: the per-k-mer route
    assert got.tobytes() == want[long_at:long_at + 1].tobytes() and d.read_segments()["segmented_launches"] == launches + 1

    # ---- a query file: one row a record, in file order, over batch seams ----
    in_file = [r for r in reads if r]
    want_file = rows_of(flat_ids([o for o, r in zip(oracle_per_read, reads) if r]), len(in_file), random_values)
    own = os.path.join(scratch, f"sums_reads_{which}_{int(canonical)}.fa")
    with open(own, "w") as f:
        for i, r in enumerate(in_file):
            f.write(f">{i}\n{r}\n")
    os.environ["SSHASH_AMD_TEST_HOOKS"] = "query_batch_bases=100000"
    seen = []

    def take(first_read, rows):
        assert first_read == sum(len(b) for b in seen)
        seen.append(rows)

    rep = d.streaming_sums_from_file(own, random_values, per_read=take)
    assert len(seen) > 2, "batch seams inside the file"
    same(np.concatenate(seen), want_file, "the file entry point")
    assert (report_row(rep) == want_report).all()
    got, _ = d.streaming_sums_from_file(own, random_values, at_least=500)
    same(got, rows_of(flat_ids([o for o, r in zip(oracle_per_read, reads) if r]), len(in_file), random_values, 500), "the file entry point, at_least")
    calls = []
    try:
        d.streaming_sums_from_file(own, random_values, per_read=lambda first, rows: calls.append(first) or 3)
        raise AssertionError("a callback's non-zero return did not stop the query")
    except sshash_amd.SSHashError as e:
        assert e.status == 1 and len(calls) == 1, (e, calls)
    calls = []

    def broken(first, rows):
        calls.append(first)
        if len(calls) == 2:
            raise KeyError("mine")

    try:
        d.streaming_sums_from_file(own, random_values, per_read=broken)
        raise AssertionError("a callback's exception did not stop the query")
    except KeyError as e:
        assert e.args == ("mine",) and len(calls) == 2 and calls[0] == 0 and calls[1] > 0, (e, calls)
    del os.environ["SSHASH_AMD_TEST_HOOKS"]

    print(json.dumps({"ok": True, "reads": n, "positive": int(want["positive_kmers"].sum(dtype=np.uint64)), "num_kmers": n_kmers,
                      "sk_slots": st["sk_slots"], "kinds": kinds}))


if __name__ == "__main__":
    main()
