"""For tests/gpu_forms_worker.py: the three forms of the streaming run kernel that came after the sweep of seven -- the classes
(STREAM_CLASSES: classes_add, labels[hit_sid]; classes_add_ids_kernel for reads above 2^16 bases), the best run (STREAM_BEST_RUN:
best_run_store; runs_best_kernel behind the run records of a long read) and the run records over segments
(STREAM_RUN_RECORDS_SEGMENTS: seg_record_store, cont[] / joined[], the kernels that turn E into run_offsets and merge a joined first
run into the record it continues). What a hit's string id is used for is new in each of them: an index into the labels, word 2 of a
record stored at the read's own index, and, under segments, a record whose place the joined[] bytes decide.

references(pt, ...) runs on the CPU, inside the worker's gate: every form gets two references that are not the library's GPU path,
asserted equal -- for the best run the argmax with the tie rule over the oracle's run records and over the run rule applied to the
oracle's per-k-mer results; for the classes the rows from the per-k-mer ids through id -> string (the strings' lengths) -> label, and the
rows from the run records, rows[read, labels[string_id]] += length; the run records over segments are the uncut ones. It also
counts what the reads must hold for a wrong kernel to show, and asserts every count positive. The other functions are the device checks
of one flavour, in the order the worker calls them: uncut, for one S, over the reads above 2^16 bases at the default S, uncut again.
All comparisons are byte for byte."""
from __future__ import annotations

import numpy as np

from gpu_best_run_worker import BACKWARD, LENGTH, best_of, device_best, device_runs_best, host_best, runs_of
from gpu_best_run_worker import same as same_best
from gpu_classes_worker import check_finish, device_classes, flat_hits, host_classes, labels_for, rows_of
from gpu_classes_worker import same as same_rows
from gpu_runs_segments_worker import chains, device_same, host_same
from gpu_segments_worker import launches

INVALID = np.uint64(0xFFFFFFFFFFFFFFFF)
CLASS_COUNTS = (3, 65)  # no power of two; on the other side of the finish kernel's group size of 64
LABELLINGS = ("mod", "random")  # string id % C: a string id that is off by one changes the column; random: a third of the strings in no class
DEFAULT_S = 256  # what set_read_segments() without a length stands for; asserted against read_segments() on the device


# ---- on the CPU ------------------------------------------------------------------------------------------------------------------------
def best_from_records(offsets, runs):
    """reference (a) of the best run: per read the argmax with the tie rule over its records of a CSR"""
    return np.concatenate([best_of(runs[int(a):int(b)]) for a, b in zip(offsets[:-1], offsets[1:])])


def best_from_rule(oracle, reads, offsets, runs, what):
    """reference (b): the run rule in numpy over the oracle's per-k-mer results, then the same argmax -> (best, the runs per read). The
    rule's runs are the CSR's, all of them, not only the longest."""
    per_read = [runs_of(oracle.streaming_read(r)) for r in reads]
    assert [p.size for p in per_read] == np.diff(offsets.astype(np.int64)).tolist(), f"{what}: the run rule counts other runs than the oracle's records"
    assert np.concatenate(per_read).tobytes() == runs.tobytes(), f"{what}: the run rule over the per-k-mer results against the oracle's records"
    return np.concatenate([best_of(p) for p in per_read]), per_read


def best_references(oracle, reads, offsets, runs, k, what):
    """-> (the best run of every read, what kinds of reads there are)"""
    want = best_from_records(offsets, runs)
    again, per_read = best_from_rule(oracle, reads, offsets, runs, what)
    same_best(again, want, f"{what}: the best run by the run rule against the best of the oracle's records")
    best_len = want["num_kmers"] & LENGTH
    lengths = np.array([len(r) for r in reads])
    assert (best_len[lengths < k] == 0).all() and not want[best_len == 0].tobytes().strip(b"\0"), f"{what}: a read without a hit is 32 zero bytes"

    def tied(p):
        n = p["num_kmers"] & LENGTH
        return p.size >= 2 and int((n == n.max()).sum()) >= 2

    kinds = {"ties_for_the_longest": sum(tied(p) for p in per_read),
             "longest_is_not_the_first": sum(p.size >= 2 and int(w["read_pos"]) != int(p["read_pos"][0]) for p, w in zip(per_read, want)),
             "longest_is_backward": int(((want["num_kmers"] & BACKWARD) != 0).sum()),
             "reads_without_a_hit": int(((best_len == 0) & (lengths >= k)).sum())}
    return want, kinds


def strings_of(ids_per_read, string_of):
    """per read the string of every k-mer id, from the strings' lengths alone (INVALID stays INVALID)"""
    out = []
    for ids in ids_per_read:
        s = np.full(ids.size, INVALID, dtype=np.uint64)
        hit = ids != INVALID
        s[hit] = string_of[ids[hit].astype(np.int64)]
        out.append(s)
    return out


def rows_from_records(offsets, runs, labels, C):
    """reference (b) of the classes, the kernel's own formula over the run records: rows[read, labels[string_id]] += length, nothing for
    a label >= C"""
    read = np.repeat(np.arange(offsets.size - 1), np.diff(offsets.astype(np.int64)))
    label = labels[runs["string_id"].astype(np.int64)].astype(np.int64)
    keep = label < C
    rows = np.zeros((offsets.size - 1, C), dtype=np.uint32)
    np.add.at(rows, (read[keep], label[keep]), (runs["num_kmers"] & LENGTH)[keep])
    return rows


def class_labels(n_strings, seed):
    """-> [(name, C, labels)]: for both C both labellings"""
    rng = np.random.default_rng(seed)
    return [(f"{name} / {C}", C, labels_for(name, n_strings, C, rng)) for C in CLASS_COUNTS for name in LABELLINGS]


def classes_references(labelled, ids_per_read, string_of, offsets, runs, what):
    """-> {name: rows} of the reads with these ids and these records, under every labelling; the two references asserted equal"""
    flat = flat_hits(ids_per_read, strings_of(ids_per_read, string_of))
    want = {}
    for name, C, labels in labelled:
        want[name] = rows_of(flat, len(ids_per_read), labels, C)
        same_rows(rows_from_records(offsets, runs, labels, C), want[name], f"{what}, {name}: labels[string_id] += length over the run records against id -> string -> label per k-mer")
    return want


def references(pt, oracle, string_of, batch_ids, hot_ids, hot_records, segment_sizes):
    """the gate's part for the three forms. pt holds the reads, their oracle ids, kinds and rows, the run records of pt.reads
    (want_offsets, want_runs) and of pt.batch (batch_offsets, batch_runs); hot_*: of the repeated read. Sets on pt what the device checks
    compare against -> the counts, every one asserted positive"""
    k, reads = pt.k, pt.reads
    # ---- the best run ----
    pt.want_best, best = best_references(oracle, reads, pt.want_offsets, pt.want_runs, k, "best run")
    assert all(v > 0 for v in best.values()) and best["ties_for_the_longest"] >= len(pt.jumps), best
    pt.want_batch_best, _ = best_references(oracle, pt.batch, pt.batch_offsets, pt.batch_runs, k, "best run of the reads above 2^16 bases")
    long_at = [i for i, r in enumerate(pt.batch) if len(r) > (1 << 16)]
    best["longest_of_the_long_reads"] = int((pt.want_batch_best["num_kmers"][long_at] & LENGTH).min())
    assert len(long_at) == 2 and best["longest_of_the_long_reads"] > 600, best  # (a whole string of 800 bases and more)
    pt.want_hot_best, _ = best_references(oracle, pt.repeated[:1], hot_records[0], hot_records[1], k, "best run of the repeated read")
    assert pt.want_hot_best.tobytes() == hot_records[1].tobytes()  # (its one run)
    # ---- the classes ----
    n_strings = int(string_of.max()) + 1
    assert n_strings == len(pt.sequences)
    pt.labelled = class_labels(n_strings, 8000 * k + 10 * pt.m + int(pt.canonical))
    pt.want_classes = classes_references(pt.labelled, pt.ids, string_of, pt.want_offsets, pt.want_runs, "classes")
    pt.want_batch_classes = classes_references(pt.labelled, batch_ids, string_of, pt.batch_offsets, pt.batch_runs, "classes of the reads above 2^16 bases")
    pt.want_hot_classes = classes_references(pt.labelled, hot_ids, string_of, hot_records[0], hot_records[1], "classes of the repeated read")
    positive = pt.want_rows[:, 1]
    classes = {}
    for name, C, labels in pt.labelled:
        rows = pt.want_classes[name]
        counted = rows.sum(axis=1, dtype=np.uint64)
        if name.startswith("mod"):  # every string has a class: nothing is masked
            assert (labels < C).all() and (counted == positive).all(), f"classes, {name}: a row's columns sum to column 1 of the per-read rows"
            classes[f"reads_with_two_columns / {C}"] = int(((rows != 0).sum(axis=1) >= 2).sum())
        else:
            assert (counted <= positive).all() and (labels >= C).any(), name
            classes[f"kmers_of_a_masked_label / {C}"] = int(positive.sum(dtype=np.uint64) - counted.sum(dtype=np.uint64))
        long_rows = pt.want_batch_classes[name][long_at]
        assert ((long_rows != 0).sum(axis=1) >= 2).all(), f"classes, {name}: the reads above 2^16 bases hit strings of several classes"
    assert all(v > 0 for v in classes.values()), classes
    # ---- the run records over segments: runs that span three whole segments and more, whose middle segments are a joined seam at both ends ----
    spanning = {str(S): chains(pt.kinds, S) for S in segment_sizes}
    spanning["long reads, default S"] = chains(pt.long_kinds, DEFAULT_S)
    assert all(v > 0 for v in spanning.values()), spanning
    return {"best_run": best, "classes": classes, "runs_over_three_segments": spanning}


# ---- on the device ---------------------------------------------------------------------------------------------------------------------
def check_best(d, reads, want, totals, what, host=True, device=True, no_report=False):
    if host:
        got, rep = host_best(d, reads)
        same_best(got, want, f"{what}: best run, host call")
        assert (rep == totals).all(), (f"{what}: best run, host call: the report", rep, totals)
    if device:
        got, rep = device_best(d, reads, report=[0] * 6)
        same_best(got, want, f"{what}: best run, device call")
        assert (rep == totals).all(), (f"{what}: best run, device call: the report", rep, totals)
    if no_report:
        got, _ = device_best(d, reads)
        same_best(got, want, f"{what}: best run, device call without a report")


def check_classes(d, reads, labelled, want, totals, what, host=True, device=True, no_report=False):
    for name, C, labels in labelled:
        if host:
            got, rep = host_classes(d, reads, labels, C)
            same_rows(got, want[name], f"{what}: classes {name}, host call")
            assert (rep == totals).all(), (f"{what}: classes {name}, host call: the report", rep, totals)
        if device:
            got, rep = device_classes(d, reads, labels, C, report=[0] * 6)
            same_rows(got, want[name], f"{what}: classes {name}, device call")
            assert (rep == totals).all(), (f"{what}: classes {name}, device call: the report", rep, totals)
        if no_report:
            got, _ = device_classes(d, reads, labels, C)
            same_rows(got, want[name], f"{what}: classes {name}, device call without a report")


def check_uncut(d, pt, totals, batch_totals, what, repeats, first=True):
    """SEGMENTS_OFF: the best run and the classes of the reads, host and device; the first time also without a report, the finish
    kernels, one read `repeats` times, and the reads above 2^16 bases (host calls: the position-parallel route; device calls: one lane a read)"""
    import sshash_amd

    reads = pt.reads
    check_best(d, reads, pt.want_best, totals, what, no_report=first)
    check_classes(d, reads, pt.labelled, pt.want_classes, totals, what, no_report=first)
    if not first:
        host_same(d, reads, pt.want_offsets, pt.want_runs, totals, f"{what}: run records")
        device_same(d, reads, int(pt.want_offsets[-1]), pt.want_offsets, pt.want_runs, f"{what}: run records", report=[0] * 6, want_report=totals)
        return
    run_offsets, runs, _ = d.streaming_runs(reads)
    same_best(sshash_amd.runs_best(run_offsets, runs), pt.want_best, f"{what}: runs_best over the records of streaming_runs")
    same_best(device_runs_best(d, run_offsets, runs), pt.want_best, f"{what}: runs_best_device over the records of streaming_runs")
    name = pt.labelled[-1][0]
    rows = pt.want_classes[name]
    assert (sshash_amd.class_totals(rows) == rows.sum(axis=0, dtype=np.uint64)).all(), f"{what}: class_totals, {name}"
    check_finish(d, rows, f"{what}: the finish of the rows, {name}")
    # one read many times: as many equal records, as many equal rows
    hot = pt.repeated
    assert len(hot) == repeats and int(pt.want_hot_best["num_kmers"][0]) == 101
    hot_totals = np.array([101, 101, 0, 0, 1, 100], dtype=np.uint64) * np.uint64(repeats)
    check_best(d, hot, np.repeat(pt.want_hot_best, repeats), hot_totals, f"{what}: one read {repeats} times")
    check_classes(d, hot, pt.labelled, {n: np.repeat(r, repeats, axis=0) for n, r in pt.want_hot_classes.items()}, hot_totals, f"{what}: one read {repeats} times", host=False)
    check_classes(d, hot, pt.labelled[:1], {n: np.repeat(r, repeats, axis=0) for n, r in pt.want_hot_classes.items()}, hot_totals, f"{what}: one read {repeats} times", device=False)
    # the reads above 2^16 bases
    batch = pt.batch
    host_same(d, batch, pt.batch_offsets, pt.batch_runs, batch_totals, f"{what}: the long reads uncut")
    check_best(d, batch, pt.want_batch_best, batch_totals, f"{what}: the long reads uncut")
    check_classes(d, batch, pt.labelled, pt.want_batch_classes, batch_totals, f"{what}: the long reads uncut")


def check_segmented(d, pt, S, totals, what):
    """segments of S k-mers, device calls too: the run records through the host call and through the device call at three capacities,
    the classes -- every call launches over segments --, the best run -- no call does -> how often the record form and the classes launched
    over segments"""
    reads = pt.reads
    want_offsets, want_runs = pt.want_offsets, pt.want_runs
    total = int(want_offsets[-1])
    begin = at = launches(d)
    host_same(d, reads, want_offsets, want_runs, totals, f"{what}: run records, S = {S}")
    assert launches(d) > at, f"{what}: S = {S}: the host call of the run records did not launch over segments"
    for capacity in (0, total - 1, total):
        at = launches(d)
        device_same(d, reads, capacity, want_offsets, want_runs, f"{what}: run records, S = {S}", report=[0] * 6 if capacity == total else None,
                    want_report=totals if capacity == total else None)
        assert launches(d) == at + 1, f"{what}: S = {S}: a device call of the run records counts one launch over segments"
    of_runs = launches(d) - begin
    begin = at = launches(d)
    check_classes(d, reads, pt.labelled, pt.want_classes, totals, f"{what}: S = {S}", device=False)
    assert launches(d) >= at + len(pt.labelled), f"{what}: S = {S}: the host calls of the classes did not launch over segments"
    at = launches(d)
    check_classes(d, reads, pt.labelled, pt.want_classes, totals, f"{what}: S = {S}", host=False)
    assert launches(d) == at + len(pt.labelled), f"{what}: S = {S}: every device call of the classes launches over segments once"
    of_classes = launches(d) - begin
    at = launches(d)
    check_best(d, reads, pt.want_best, totals, f"{what}: S = {S}")
    assert launches(d) == at, f"{what}: S = {S}: the best run was cut into segments"
    return of_runs, of_classes


def check_long(d, pt, batch_totals, what):
    """the reads above 2^16 bases at the default S: the run records by host call and by device call with all the room, the classes by host
    and device call, the best run by host call"""
    batch = pt.batch
    total = int(pt.batch_offsets[-1])
    at = launches(d)
    host_same(d, batch, pt.batch_offsets, pt.batch_runs, batch_totals, f"{what}: run records")
    assert launches(d) > at, f"{what}: the host call of the run records did not launch over segments"
    at = launches(d)
    device_same(d, batch, total, pt.batch_offsets, pt.batch_runs, f"{what}: run records", report=[0] * 6, want_report=batch_totals)
    assert launches(d) == at + 1
    check_classes(d, batch, pt.labelled, pt.want_batch_classes, batch_totals, what)
    assert launches(d) >= at + 1 + 2 * len(pt.labelled), f"{what}: the classes did not launch over segments"
    at = launches(d)
    check_best(d, batch, pt.want_batch_best, batch_totals, what, device=False)
    assert launches(d) == at, f"{what}: the best run was cut into segments"
