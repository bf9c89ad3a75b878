#!/usr/bin/env python
"""Worker of tests/test_gpu_streaming_classes.py: one process = one dictionary and one setting of the environment switch that decides
whether a replica holds the super-k-mer table (SSHASH_AMD_SKTABLE=0: the run kernel takes the complete seed() path). Everything the
streaming classes promise -- rows[r, c] = the positive k-mers of read r in strings labelled c -- against ground truth that shares no code
with the kernels: numpy.add.at over labels[string_id] of the valid places, once from streaming_lookup's per-k-mer string_id and once from
the CPU oracle's point lookups of every k-mer of every read. All comparisons are exact. The reads are those of the sums worker and a few
that are made of pieces of two strings. The oracle's results also say, before anything runs on the GPU, that the reads hold what the
kernel has to tell apart. Prints one JSON line; any mismatch is an assertion error.

    python tests/gpu_classes_worker.py <k31|k63> <canonical 0|1> <scratch directory> [shards]"""
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import numpy as np

from gpu_depth_worker import upload
from gpu_per_read_worker import report_row, revcomp
from gpu_sums_worker import build, make_reads as sums_reads

INVALID = np.uint64(0xFFFFFFFFFFFFFFFF)
GUARD = 0x5A5A5A5A
GARBAGE = 0x77777777
CLASS_COUNTS = (1, 3, 64, 65, 4096)  # both sides of the finish kernel's group size, no power of two, the cap
READS_AT_THE_CAP = 64


def make_reads(sequences, k):
    """the sums worker's reads (-> reads, index of the read above 2^16 bases) and, behind them, reads made of pieces of two strings"""
    reads, long_at = sums_reads(sequences, k)
    rng = np.random.default_rng(29)
    usable = [s for s in sequences if len(s) >= k + 40]
    for j in range(24):
        a, b = (usable[int(i)] for i in rng.choice(len(usable), 2, replace=False))
        r = a[:k + 40] + b[-(k + 30):]
        reads.append(revcomp(r) if j % 2 else r)
    return reads, long_at


def oracle_hits(oracle, reads, k):
    """per read the (kmer_id, string_id) of every k-mer by the oracle's point lookup (either strand); INVALID where the k-mer holds anything
    but A, C, G, T in either case or is not in the dictionary"""
    ok = np.zeros(256, dtype=bool)
    ok[list(b"ACGTacgt")] = True
    ids, sids, kmers, where = [], [], [], []
    for i, r in enumerate(reads):
        b = np.frombuffer(r.encode("ascii", "replace"), dtype=np.uint8)
        ids.append(np.full(max(0, b.size - k + 1), INVALID, dtype=np.uint64))
        sids.append(np.full(max(0, b.size - k + 1), INVALID, dtype=np.uint64))
        if b.size < k:
            continue
        windows = np.lib.stride_tricks.sliding_window_view(b, k)
        valid = ok[windows].all(axis=1)
        kmers.append(windows[valid] & np.uint8(0xDF))  # (upper case)
        where.append((i, np.flatnonzero(valid)))
    if kmers:
        got = oracle.lookup_ascii(np.ascontiguousarray(np.concatenate(kmers)).reshape(-1), True)
        at = 0
        for i, places in where:
            found = got["kmer_id"][at:at + places.size] != INVALID
            ids[i][places] = got["kmer_id"][at:at + places.size]
            sids[i][places[found]] = got["string_id"][at:at + places.size][found]
            at += places.size
    return ids, sids


def flat_hits(ids_per_read, sids_per_read):
    """-> (read, string) of every valid place"""
    read = np.concatenate([np.full(ids.size, r, dtype=np.int64) for r, ids in enumerate(ids_per_read)] + [np.zeros(0, dtype=np.int64)])
    ids = np.concatenate(list(ids_per_read) + [np.zeros(0, dtype=np.uint64)])
    sids = np.concatenate(list(sids_per_read) + [np.zeros(0, dtype=np.uint64)])
    hit = ids != INVALID
    return read[hit], sids[hit].astype(np.int64)


def rows_of(flat, n_reads, labels, C):
    """numpy: rows[r, c] = the hits of read r in strings labelled c; a label >= C is counted nowhere"""
    read, sid = flat
    label = labels[sid].astype(np.int64)
    keep = label < C
    rows = np.zeros((n_reads, C), dtype=np.uint32)
    np.add.at(rows, (read[keep], label[keep]), np.uint32(1))
    return rows


def labels_for(name, n_strings, C, rng):
    if name == "mod":
        return (np.arange(n_strings, dtype=np.uint64) % np.uint64(C)).astype(np.uint32)
    if name == "one":
        return np.zeros(n_strings, dtype=np.uint32)
    labels = rng.integers(0, C, n_strings).astype(np.uint32)  # "random": a third of the strings in no class
    out = np.flatnonzero(rng.integers(0, 3, n_strings) == 0)
    labels[out] = np.array([C, C + 5, 0xFFFFFFFF, 0x80000000], dtype=np.uint64)[rng.integers(0, 4, out.size)].astype(np.uint32)
    return labels


def same(got, want, what):
    assert got.dtype == np.uint32 and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert bad.size == 0, (what, "(read, class)", bad[:5].tolist(), [int(got[tuple(b)]) for b in bad[:5]], [int(want[tuple(b)]) for b in bad[:5]])


def device_classes(d, reads, labels, C, report=None, stream=None, total_bases=None):
    """the device entry point on device 0 over rows that held garbage, at an address that is a multiple of 4 and not of 8, guard words on
    both sides; the labels between guard words too and asserted untouched -> (rows, report or None)"""
    import torch

    dev = torch.device("cuda", 0)
    n = len(reads)
    d_bases, d_off, n_bases = upload(reads)
    host = np.full(n * C + 4, GARBAGE, dtype=np.uint32)
    host[:3] = GUARD
    host[-1] = GUARD
    t = torch.from_numpy(host.view(np.int32).copy()).to(dev)
    p = t.data_ptr() + 12
    assert p % 4 == 0 and p % 8 != 0
    guarded_labels = np.full(labels.size + 2, GUARD, dtype=np.uint32)
    guarded_labels[1:-1] = labels
    d_labels = torch.from_numpy(guarded_labels.view(np.int32).copy()).to(dev)
    d_report = None if report is None else torch.from_numpy(np.asarray(report, dtype=np.uint64).view(np.int64).copy()).to(dev)
    torch.cuda.synchronize()  # (the copies run on torch's stream, the query may run on another)
    d.streaming_classes_device(0, d_bases.data_ptr(), d_off.data_ptr(), n, d_labels.data_ptr() + 4, C, p, d_report=0 if d_report is None else d_report.data_ptr(),
                               stream=0 if stream is None else stream.cuda_stream, total_bases=n_bases if total_bases is None else total_bases)
    (stream or torch.cuda.current_stream()).synchronize()
    torch.cuda.synchronize()
    got = t.cpu().numpy().view(np.uint32)
    assert (got[:3] == GUARD).all() and int(got[-1]) == GUARD, "a word outside rows[0 .. num_reads * C) was written"
    assert (d_labels.cpu().numpy().view(np.uint32) == guarded_labels).all(), "the labels were changed"
    return got[3:-1].copy().reshape(n, C), None if d_report is None else d_report.cpu().numpy().view(np.uint64)


def host_classes(d, reads, labels, C):
    """the host entry point itself (the binding hands it rows of zeros, which would hide a piece whose rows never came back): rows that
    held garbage, at an address that is a multiple of 4 and not of 8, guard words on both sides -> (rows, the six counters)"""
    import ctypes

    from sshash_amd import _binding as B

    n = len(reads)
    chunks = [r.encode("ascii", "replace") for r in reads]
    offsets = np.zeros(n + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum([len(c) for c in chunks], dtype=np.uint64)
    bases = np.frombuffer(b"".join(chunks) or b"\0", dtype=np.uint8)
    labels = np.ascontiguousarray(labels, dtype=np.uint32)
    host = np.full(n * C + 5, GARBAGE, dtype=np.uint32)
    at = 3 if host.ctypes.data % 8 == 0 else 2  # (numpy's buffers are aligned to 8 at the least)
    p = host.ctypes.data + 4 * at
    assert p % 4 == 0 and p % 8 != 0
    host[:at] = GUARD
    host[at + n * C:] = GUARD
    rep = B._Report()
    B._check(B._load().sshash_streaming_classes(d._h, bases.ctypes.data, offsets.ctypes.data, n, labels.ctypes.data, C, ctypes.c_void_p(p), ctypes.byref(rep)))
    assert (host[:at] == GUARD).all() and (host[at + n * C:] == GUARD).all(), "a word outside rows[0 .. num_reads * C) was written"
    return host[at:at + n * C].copy().reshape(n, C), report_row(d._report(rep))


def best_of(rows):
    """numpy: the finish of the rows, by a stable sort"""
    import sshash_amd

    rows = rows.astype(np.uint32)
    n, C = rows.shape
    out = np.zeros(n, dtype=sshash_amd.READ_CLASS_DTYPE)
    order = np.argsort(-rows.astype(np.int64), axis=1, kind="stable")  # (descending by count; among equals ascending by class)
    out["best_class"] = order[:, 0]
    out["best"] = rows[np.arange(n), order[:, 0]]
    out["second"] = rows[np.arange(n), order[:, 1]] if C > 1 else 0
    out["total"] = (rows.sum(axis=1, dtype=np.uint64) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    out["best_class"][out["best"] == 0] = sshash_amd.NO_CLASS
    return out


def check_finish(d, rows, what):
    """class_best and class_totals: the device kernels, the host variants and numpy agree on `rows` (outputs that held garbage, guarded)"""
    import torch

    import sshash_amd

    dev = torch.device("cuda", 0)
    n, C = rows.shape
    want_best, want_totals = best_of(rows), rows.sum(axis=0, dtype=np.uint64)
    host_best, host_totals = sshash_amd.class_best(rows), sshash_amd.class_totals(rows)
    assert host_best.tobytes() == want_best.tobytes(), (what, "class_best on the host", np.flatnonzero(host_best != want_best)[:5].tolist())
    assert (host_totals == want_totals).all(), (what, "class_totals on the host")
    d_rows = torch.from_numpy(np.ascontiguousarray(rows).view(np.int32).copy()).to(dev)
    best = np.full(4 * n + 2, GARBAGE, dtype=np.uint32)
    best[0] = best[-1] = GUARD
    totals = np.full(C + 2, 0x7777777777777777, dtype=np.uint64)
    totals[0] = totals[-1] = 0x5A5A5A5A5A5A5A5A
    d_best, d_totals = torch.from_numpy(best.view(np.int32).copy()).to(dev), torch.from_numpy(totals.view(np.int64).copy()).to(dev)
    torch.cuda.synchronize()
    d.class_best_device(0, d_rows.data_ptr(), n, C, d_best.data_ptr() + 4)
    d.class_totals_device(0, d_rows.data_ptr(), n, C, d_totals.data_ptr() + 8)
    torch.cuda.synchronize()
    got_best, got_totals = d_best.cpu().numpy().view(np.uint32), d_totals.cpu().numpy().view(np.uint64)
    assert int(got_best[0]) == GUARD and int(got_best[-1]) == GUARD and got_totals[0] == totals[0] and got_totals[-1] == totals[-1], (what, "guards")
    got_best = got_best[1:-1].copy().view(sshash_amd.READ_CLASS_DTYPE)
    bad = np.flatnonzero(got_best != want_best)
    assert bad.size == 0, (what, "class_best_device", bad[:5].tolist(), got_best[bad[:5]].tolist(), want_best[bad[:5]].tolist())
    assert (got_totals[1:-1] == want_totals).all(), (what, "class_totals_device")
    assert (d_rows.cpu().numpy().view(np.uint32).reshape(n, C) == rows).all(), "the rows were changed"


def tie_rows(C, rng):
    """rows made to tie: few distinct counts, so that most rows have several classes at the maximum; rows of zeros; counts of 0xFFFFFFFF;
    a single column that is not zero; the maximum in the last class alone and in the first and the last"""
    n = 300 if C <= 65 else 40
    rows = rng.integers(0, 3, (n, C)).astype(np.uint32)
    rows[::7] = 0
    rows[1::7] = rng.choice(np.array([0, 0xFFFFFFFF], dtype=np.uint32), (rows[1::7].shape[0], C))
    rows[2::7] = 0
    rows[2::7, rng.integers(0, C)] = 9
    rows[3::7, C - 1] = 5
    rows[4::7, 0] = 5
    rows[4::7, C - 1] = 5
    rows[5, :] = 0xFFFFFFFF
    return rows


def shards_main(which, canonical, scratch):
    """two minimizer shards: each counts the k-mers it owns, so the shards' rows added together are the rows of the whole index"""
    import sshash_amd

    whole, sequences, k = build(which, canonical, scratch)
    whole.to_device(0)
    reads, _ = make_reads(sequences, k)
    C = 5
    labels = labels_for("random", whole.num_strings(), C, np.random.default_rng(7))
    per_read, _ = whole.streaming_lookup(reads, full=True)
    want = rows_of(flat_hits([p.kmer_id for p in per_read], [p.string_id for p in per_read]), len(reads), labels, C)
    got, rep = whole.streaming_classes(reads, labels, C)
    same(got, want, "the whole index")
    total = np.zeros_like(want)
    parts = []
    for r in range(2):
        shard, _, _ = build(which, canonical, scratch, num_shards=2, shard_id=r)
        shard.to_device(0)
        assert shard.num_strings() == whole.num_strings()
        part, shard_rep = shard.streaming_classes(reads, labels, C)
        assert 0 < int(part.sum(dtype=np.uint64)) <= shard_rep.num_positive_kmers
        try:  # (the run kernel would follow an owned k-mer's run through k-mers of the other shard: the device call refuses)
            shard.streaming_classes_device(0, 8, 8, 1, 8, C, 8)
            raise AssertionError("the device call on a minimizer shard did not refuse")
        except sshash_amd.SSHashError as e:
            assert e.status == 1 and "minimizer shard" in str(e), e
        total += part
        parts.append(part.sum(axis=1, dtype=np.uint64))
    both = (parts[0] != 0) & (parts[1] != 0)
    alone = (parts[0] != 0) ^ (parts[1] != 0)
    assert both.any() and alone.any(), "reads whose k-mers lie in both shards, and reads of one shard alone"
    same(total, want, "the shards' rows added")
    print(json.dumps({"ok": True, "shards": 2, "positive": int(rep.num_positive_kmers), "counted": int(want.sum(dtype=np.uint64))}))


def main():
    import torch

    import sshash_amd
    from oracle import oracle as O

    which, canonical, scratch = sys.argv[1], bool(int(sys.argv[2])), sys.argv[3]
    if len(sys.argv) > 4 and sys.argv[4] == "shards":
        return shards_main(which, canonical, scratch)
    d, sequences, k = build(which, canonical, scratch)
    n_strings = d.num_strings()
    reads, long_at = make_reads(sequences, k)
    n = len(reads)
    short_reads = reads[:long_at] + reads[long_at + 1:]
    drop = lambda rows: np.concatenate([rows[:long_at], rows[long_at + 1:]])
    lengths = np.array([len(r) for r in reads])

    # ---- on the CPU, before anything runs on the GPU: the oracle's hits, the truth of every case, and what the reads have to hold ----
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "w.sshash")
        d.save(path)
        oracle_ids, oracle_sids = oracle_hits(O.OracleIndex(path), reads, k)
    flat = flat_hits(oracle_ids, oracle_sids)
    assert n_strings >= 6 and int(flat[1].max()) < n_strings
    rng = np.random.default_rng(7)
    cases = []  # (name, C, labels, rows wanted of all reads)
    for C in CLASS_COUNTS:
        for name in ("mod", "one", "random"):
            labels = labels_for(name, n_strings, C, rng)
            cases.append((f"{name} / {C}", C, labels, rows_of(flat, n, labels, C)))
    strings_hit = [np.unique(s[s != INVALID]).astype(np.int64) for s in oracle_sids]
    by_name = {name: (labels, want) for name, C, labels, want in cases}
    mod3 = by_name["mod / 3"][0]
    # (among the reads of a few hundred bases, which a lane of the run kernel walks, not only in the read above 2^16 bases)
    few = [i for i in range(n) if i != long_at and strings_hit[i].size >= 2]
    kinds = {"two_strings_of_different_classes": sum(np.unique(mod3[strings_hit[i]]).size >= 2 for i in few),
             "two_strings_of_the_same_class": sum(np.unique(mod3[strings_hit[i]]).size < strings_hit[i].size for i in few)
             + int(np.unique(mod3[strings_hit[long_at]]).size < strings_hit[long_at].size),
             "reads_above_2_16": int((lengths > (1 << 16)).sum()), "reads_with_N": sum("N" in r for r in reads),
             "reads_shorter_than_k": int((lengths < k).sum()), "empty_reads": int((lengths == 0).sum())}
    for C in CLASS_COUNTS:
        labels, want = by_name[f"random / {C}"]
        only_outside = [i for i in range(n) if strings_hit[i].size and (labels[strings_hit[i]] >= C).all()]
        kinds[f"hits_only_in_no_class_{C}"] = len(only_outside)
        assert all(int(want[i].sum()) == 0 for i in only_outside)
    assert all(v > 0 for v in kinds.values()), kinds
    assert kinds["reads_above_2_16"] == 1 and lengths[long_at] > (1 << 16) and 1800 <= n <= 2300, (kinds, n)

    # ---- the same truth from streaming_lookup on the GPU ----
    d.to_device(0)
    st = d.device_stats(0)
    per_read, _ = d.streaming_lookup(reads, full=True)
    assert all((p.kmer_id == o).all() for p, o in zip(per_read, oracle_ids)), "streaming_lookup's kmer_id against the oracle's point lookups"
    flat_gpu = flat_hits([p.kmer_id for p in per_read], [p.string_id for p in per_read])
    assert (flat_gpu[0] == flat[0]).all() and (flat_gpu[1] == flat[1]).all(), "streaming_lookup's string_id against the oracle's"
    for name, C, labels, want in cases:
        same(rows_of(flat_gpu, n, labels, C), want, name + ": the two ground truths")
    want_report = report_row(d.streaming_query(reads))
    want_short_report = report_row(d.streaming_query(short_reads))
    per_read_rows, _ = d.streaming_query_per_read(reads)

    for name, C, labels, want in cases:
        positive = want.sum(axis=1, dtype=np.uint64)
        assert (positive <= per_read_rows[:, 1]).all(), name
        if name.startswith("one") or name.startswith("mod"):  # (every string has a class: nothing is masked)
            assert (positive == per_read_rows[:, 1]).all(), name
        if name.startswith("one"):
            assert (want[:, 0] == per_read_rows[:, 1]).all() and not want[:, 1:].any(), "one class: column 1 of streaming_query_per_read"
        if name.startswith("random"):
            assert (positive < per_read_rows[:, 1]).any(), "the mask takes something away"
        if C == 4096:  # the cap: the first reads only
            few_reads, want_few = reads[:READS_AT_THE_CAP], want[:READS_AT_THE_CAP]
            got, rep = d.streaming_classes(few_reads, labels, C)
            same(got, want_few, name + ": host call")
            got, rep = device_classes(d, few_reads, labels, C, report=[0] * 6)
            same(got, want_few, name + ": device call")
            check_finish(d, want_few, name)
            continue
        # the host call: with the long read its piece takes the per-k-mer route (segments are off), without it the run kernel
        got, rep = d.streaming_classes(reads, labels, C)
        same(got, want, name + ": host call, per-k-mer route")
        assert (report_row(rep) == want_report).all(), (name, report_row(rep), want_report)
        got, rep = d.streaming_classes(short_reads, labels, C)
        same(got, drop(want), name + ": host call, run kernel")
        assert (report_row(rep) == want_short_report).all(), (name, report_row(rep), want_short_report)
        # the device call: the classes form of the run kernel (one lane walks the long read)
        got, rep = device_classes(d, reads, labels, C, report=[0] * 6)
        same(got, want, name + ": device call")
        assert (rep == want_report).all(), (name, rep, want_report)
        check_finish(d, want, name)
    for C in CLASS_COUNTS:
        check_finish(d, tie_rows(C, rng), f"rows made to tie / {C}")

    C = 65
    labels, want = by_name["random / 65"]
    got, rep = device_classes(d, reads, labels, C, report=[1, 2, 3, 4, 5, 6], stream=torch.cuda.Stream(device=0), total_bases=0)
    same(got, want, "device call on a side stream, total_bases = 0")
    assert (rep == want_report + np.arange(1, 7, dtype=np.uint64)).all(), "the report is accumulated into"
    got, rep = device_classes(d, reads, labels, C)  # a NULL report
    same(got, want, "device call, no report")
    # the host call itself over rows that held garbage (the binding hands it zeros): every piece's rows come back, hitless reads' too
    assert (want.sum(axis=1, dtype=np.uint64) == 0).any()
    got, rep = host_classes(d, reads, labels, C)
    same(got, want, "host call into rows that held garbage")
    assert (rep == want_report).all()
    got, rep = host_classes(d, ["", "", ""], labels, C)
    assert not got.any() and not rep.any(), "host call, reads without a base, into rows that held garbage"
    # no reads at all, and reads without a base: rows of zeros over what was garbage
    d.streaming_classes_device(0, 0, 0, 0, 0, C, 0)
    got, rep = device_classes(d, ["", "", ""], labels, C, report=[1] * 6, total_bases=0)
    assert not got.any() and (rep == 1).all(), "reads without a base"
    empty, _ = d.streaming_classes([], labels, C)
    assert empty.shape == (0, C)

    # ---- geometry independence: the test hooks of the run kernel and of the host call's pieces ----
    for hook in ("stream_move_out_every=1", "stream_move_out_every=7", "stream_piece_reads=300", "stream_piece_reads=257"):
        os.environ["SSHASH_AMD_TEST_HOOKS"] = hook
        got, rep = d.streaming_classes(reads, labels, C)  # (pieces of 300 reads: the long read's piece by ids, the others by the run kernel)
        assert got.tobytes() == want.tobytes() and (report_row(rep) == want_report).all(), hook
        got, rep = device_classes(d, reads, labels, C, report=[0] * 6)
        assert got.tobytes() == want.tobytes() and (rep == want_report).all(), hook
        got, rep = host_classes(d, reads, labels, C)  # (several pieces, rows that held garbage)
        assert got.tobytes() == want.tobytes() and (rep == want_report).all(), hook
    del os.environ["SSHASH_AMD_TEST_HOOKS"]
    # the cap on a piece's reads: 64 MiB of rows are 4096 reads at 4096 classes, and here are more
    labels_cap, want_cap = by_name["mod / 4096"]
    many = short_reads * 3
    assert len(many) > (64 << 20) // (4096 * 4)
    got, rep = d.streaming_classes(many, labels_cap, 4096)
    same(got, np.concatenate([drop(want_cap)] * 3), "more reads than a piece holds at the cap")
    assert (report_row(rep) == 3 * want_short_report).all()

    # ---- segments: many lanes add into one row ----
    launches = d.read_segments()["segmented_launches"]
    assert launches == 0
    for S in (1, 7, 64):
        d.set_read_segments(S, device_calls=True)
        got, rep = device_classes(d, reads, labels, C, report=[0] * 6)
        assert got.tobytes() == want.tobytes() and (rep == want_report).all(), ("segments, device call", S)
        assert d.read_segments()["segmented_launches"] == launches + 1
        got, rep = d.streaming_classes(reads, labels, C)
        assert got.tobytes() == want.tobytes() and (report_row(rep) == want_report).all(), ("segments, host call", S)
        launches = d.read_segments()["segmented_launches"]
        assert launches >= 2
    d.set_read_segments()  # the default S, host calls only: the long read's piece goes over segments
    got, rep = d.streaming_classes(reads, labels, C)
    assert got.tobytes() == want.tobytes() and (report_row(rep) == want_report).all(), "the long read at the default S"
    assert d.read_segments()["segmented_launches"] == launches + 1
    d.set_read_segments(sshash_amd.SEGMENTS_OFF)
    got, rep = d.streaming_classes([reads[long_at]], labels, C)  # segments off: the per-k-mer route
    assert got.tobytes() == want[long_at:long_at + 1].tobytes() and d.read_segments()["segmented_launches"] == launches + 1

    # ---- a query file: one row a record, in file order, over batch seams ----
    in_file = [i for i, r in enumerate(reads) if r]
    want_file = want[in_file]
    own = os.path.join(scratch, f"classes_reads_{which}_{int(canonical)}.fa")
    with open(own, "w") as f:
        for i in in_file:
            f.write(f">{i}\n{reads[i]}\n")
    os.environ["SSHASH_AMD_TEST_HOOKS"] = "query_batch_bases=100000"
    seen = []

    def take(first_read, rows):
        assert first_read == sum(len(b) for b in seen)
        seen.append(rows)

    rep = d.streaming_classes_from_file(own, labels, C, per_read=take)
    assert len(seen) > 2, "batch seams inside the file"
    same(np.concatenate(seen), want_file, "the file entry point")
    assert (report_row(rep) == want_report).all()
    got, _ = d.streaming_classes_from_file(own, by_name["mod / 3"][0], 3)
    same(got, by_name["mod / 3"][1][in_file], "the file entry point, rows kept")
    calls = []
    try:
        d.streaming_classes_from_file(own, labels, C, per_read=lambda first, rows: calls.append(first) or 3)
        raise AssertionError("a callback's non-zero return did not stop the query")
    except sshash_amd.SSHashError as e:
        assert e.status == 1 and len(calls) == 1, (e, calls)
    calls = []

    def broken(first, rows):
        calls.append(first)
        if len(calls) == 2:
            raise KeyError("mine")

    try:
        d.streaming_classes_from_file(own, labels, C, per_read=broken)
        raise AssertionError("a callback's exception did not stop the query")
    except KeyError as e:
        assert e.args == ("mine",) and len(calls) == 2 and calls[0] == 0 and calls[1] > 0, (e, calls)
    del os.environ["SSHASH_AMD_TEST_HOOKS"]

    print(json.dumps({"ok": True, "reads": n, "counted": int(want.sum(dtype=np.uint64)), "positive": int(per_read_rows[:, 1].sum()),
                      "strings": n_strings, "sk_slots": st["sk_slots"], "kinds": kinds}))


if __name__ == "__main__":
    main()
