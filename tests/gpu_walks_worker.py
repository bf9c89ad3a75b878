#!/usr/bin/env python
"""Worker of tests/test_gpu_streaming_walks.py, and the input generator it shares with tests/test_walks_inputs.py: every output form
of the streaming run kernel over the three kinds of table on which the kernel's own walk -- its hand-inlined restatement of
sk_walk_step, one bucket a turn, with `lasts`, the remembered heavy key, the way back to the key's sequence and the unplaced key that
takes the complete path -- goes further than a key's first bucket as a matter of course:

    packed    SSHASH_AMD_TEST_HOOKS=slots_per_key=1.2,slots_per_kmer=1.2: a load factor above 0.75, second to fifth choices, items
              without a slot in five
    compact   SSHASH_AMD_SK_DENSITY=compact, the footprint switch of INTEGRATION.md
    shard     to_device(0, table_shards=3, table_shard_id=1): the keys of two shards in three take the complete path inside the
              table's kernel, beside lanes that walk

One worker process = one point (k, m, length of the table's keys) and one layer, regular then canonical. The worker sets nothing in
its environment (the test does) and asserts from device_stats(), after the upload and before the first streaming call, that the layer
took: replica_of below. Then everything tests/gpu_forms_worker.py does at the point -- make_inputs, gate, check_flavour, unchanged, on
this replica: all ten forms, host and device call, uncut, S = 1, 7, 64, uncut again, the reads above 2^16 bases, the read 4096 times.
No helper that check_flavour reuses sets or deletes SSHASH_AMD_TEST_HOOKS inside the process (those that do are the main() of other
workers), so the hook string of `packed` is still there when the second flavour uploads; replica_of's assertions run per flavour and say so.

Whole strings seed once per string. Two PROBE SETS make every item of the table a seed:

    1. every k-mer of the dictionary as a read of its own, id i forward for even i and reverse-complemented for odd i: every inline
       occurrence, every item without a slot (at the end of a walk over five buckets) and every k-mer of a heavy key (through the
       marker, then the k-mers' region) is sought as a seed
    2. windows of 2k + 8 bases out of every string that long, at a stride that gives 1500 to 3000 of them, with one substitution at
       base k + 3: four positive k-mers, k negative ones that mostly still elect a key the table holds, five positive ones; the strands
       alternate, the substituted base rotates. These are the misses that settle at the end of a walk and stand for the k-mers behind
       them (`lasts`, sk_key_persists), and the negatives under a remembered heavy key

They go through a slimmer pass (probe_pass) with no Python loop per read on the device's side: uncut, host and device call, the
counters, the per-read rows, the run offsets and records, cover, depth, the sums under full-range random values, the classes under
string id % 3 and under random labels over 65 a third of which are no class, the best run, and the ids of streaming_lookup; set 2 once
more at S = 7 for rows, run records and classes. The references are those the sweep trusts: the oracle's restated state machine, read
by read, and GroundTruth.lookup of every k-mer, asserted equal on the CPU before the first device call (probe_gate), and numpy over the
oracle's results for the rest -- sums, classes and best run once from the per-k-mer ids and once from the run records, asserted equal.
Nothing is compared with another GPU path alone; all comparisons are exact. Prints one JSON line; any mismatch is an assertion error.

    python tests/gpu_walks_worker.py <k> <m> <key_length or 0> <layer: packed|compact|shard> <table_keys binary> <scratch dir> [--cpu-only]"""
from __future__ import annotations

import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import numpy as np

from gpu_even_m_worker import key_length_of, kmers_of, table_keys
from gpu_forms_worker import HEAVY, INVALID, _adder, check_flavour, gate, make_inputs, rows_from_runs, string_of_ids, sums_cases
from gpu_per_read_worker import COLUMNS, random_dna, revcomp
from gpu_routing_worker import pack
from gpu_routing_worker import revcomp as packed_revcomp

BACKWARD = np.uint32(0x80000000)
LENGTH = np.uint32(0x7FFFFFFF)
PACKED_HOOKS = "slots_per_key=1.2,slots_per_kmer=1.2"
POINTS = {  # layer -> (k, m, key length or 0): where the walk's code differs -- one and two words, m < 12, a key length on either side of m, an even m, heavy keys
    "packed": [(21, 11, 0), (31, 7, 0), (31, 27, 0), (31, 21, 17), (31, 8, 0), (33, 13, 0), (47, 15, 31), (63, 25, 12), (63, 30, 0), (63, 31, 0)],
    "compact": [(31, 7, 0), (31, 21, 17), (33, 13, 0), (63, 31, 0)],
    "shard": [(31, 27, 0), (31, 8, 0), (47, 15, 31), (63, 25, 12)],
}
MATRIX = [(k, m, L, layer) for layer, points in POINTS.items() for k, m, L in points]  # one worker each
ENVIRONMENT = {"packed": {"SSHASH_AMD_TEST_HOOKS": PACKED_HOOKS}, "compact": {"SSHASH_AMD_SK_DENSITY": "compact"}, "shard": {}}
SHARDS, SHARD_ID = 3, 1
DEFERRED_FLOOR = {"packed": 8, "compact": 1}  # items without a slot in five choices, per flavour: conditions of the test, not tolerances
# Plain random strings behind the point's own, in bases, where the table would otherwise leave too few items without a slot for the
# floor above to hold on every upload (which items find no slot depends on the order in which the build's threads arrive; a table's
# items are its super-k-mers, a tenth to a thirtieth of the k-mers). Without them the two points left 3 items out per flavour on an
# MI355X (tests/test_gpu_streaming_walks.py), with them 7 to 12.
PLAIN_BASES = {("compact", 33, 13, 0): 60000, ("compact", 63, 31, 0): 90000}
# Two table keys with EQUAL 24-bit fingerprints whose first choice is the same bucket for every number of buckets in BUCKETS -- the
# packed table of this point has 2009 of them, which the worker derives from device_stats() and asserts --, both with an election hash
# in the lowest hundredth, so that they win the election of a window between random flanks more often than not (found by a search over
# all 4^13 keys of 13 bases; table_hash restates the arithmetic and tests/test_walks_inputs.py holds the pair against it). The first
# is planted LIGHT_COPIES times -- a light key, one inline slot per occurrence --, the second HEAVY_COPIES times -- a heavy key: one
# marker, its k-mers under keys of their own. The table places long super-k-mers first and a marker with the longest; an occurrence of
# the light key is the first LIGHT_RUN k-mers of a string of 2k bases and no more (the key starts at base LIGHT_RUN - 1; a string's LAST
# super-k-mer counts as a long one whatever it holds, sktable.hip: `run`), so the four are placed behind the marker. Four items and a
# marker want one bucket of two slots: at least three occurrences of the light key go on from it, and a seed on one of them meets a
# marker with its key's fingerprint and the bucket's go-on flag, finds nothing under the k-mer's own key and has to come BACK to the
# next choice of the key's sequence -- the one case in which `back` decides an answer. Two keys meet like that by chance once in 2^24
# pairs that share a bucket.
COLLIDING = {("packed", 33, 13, 0): ("ACGTACCACGTTA", "GATTTGGTTTTAT")}  # (the light key, the heavy key)
BUCKETS = (1850, 2200)
LIGHT_COPIES, HEAVY_COPIES = 4, 8  # (device_layout.hpp: SK_INLINE_MAX = 4 occurrences are held inline, a key with more is heavy)
LIGHT_RUN = 3
WINDOWS = (1500, 3000)
PATTERN_SHARE = 0.8  # of the windows of set 2: four positive k-mers, k negative, five positive (a substitution may land on another k-mer of the dictionary)
SEGMENT = 7


def environment_of(key_length, layer):
    """what the test puts into the worker's environment (every other SSHASH_AMD_* setting is taken out first)"""
    env = dict(ENVIRONMENT[layer])
    if key_length:
        env["SSHASH_AMD_SK_M"] = str(key_length)
    return env


def key_value(motif):
    """the bases of a table key as the table packs them: first base in the low bits, A0 C1 T2 G3"""
    return sum(((ord(c) >> 1) & 3) << (2 * j) for j, c in enumerate(motif))


def table_hash(keys):
    """device_layout.hpp: sk_hash_a restated -> (the 24-bit fingerprint, the word that choice 0 is taken from: bucket = word * buckets >> 32)"""
    key = np.asarray(keys, dtype=np.uint64)
    a = key * np.uint64(0xFF51AFD7ED558CCD)
    a ^= a >> np.uint64(32)
    a *= np.uint64(0xC4CEB9FE1A85EC53)
    a ^= a >> np.uint64(29)
    return a & np.uint64(0xFFFFFF), a >> np.uint64(32)


def with_plain_strings(seqs, k, bases, seed):
    """seqs and, behind them, plain random strings of 300 - 900 bases, `bases` bases of them"""
    rng = np.random.default_rng(seed)
    seqs = list(seqs)
    add = _adder(seqs, k)
    while bases > 0:
        n = int(rng.integers(300, 901))
        while not add(random_dna(rng, n)):
            pass
        bases -= n
    return seqs


def with_colliding_keys(seqs, k, key_length, pair, exe, seed):
    """seqs and, behind them, LIGHT_COPIES strings of 2k bases whose first LIGHT_RUN k-mers elect pair[0] as their table key, and
    HEAVY_COPIES strings of exactly k bases whose k-mer elects pair[1]: the flanks are drawn until tests/cpp/table_keys.cpp (the host's
    build of sk_key) says so"""
    rng = np.random.default_rng(seed)
    seqs = list(seqs)
    add = _adder(seqs, k)
    light, heavy = pair
    assert len(light) == len(heavy) == key_length
    candidates = [random_dna(rng, LIGHT_RUN - 1) + light + random_dna(rng, 2 * k - key_length - LIGHT_RUN + 1) for _ in range(600)]
    elected = table_keys(exe, kmers_of(candidates, k), k, key_length).reshape(len(candidates), k + 1)
    mine = (elected["key"] == np.uint64(key_value(light))) & (elected["tie"] == 0)
    good_light = np.flatnonzero(mine[:, :LIGHT_RUN].all(axis=1) & ~mine[:, LIGHT_RUN:].any(axis=1))
    more = [random_dna(rng, int(a)) + heavy + random_dna(rng, k - key_length - int(a)) for a in rng.integers(0, k - key_length + 1, 1500)]
    elected = table_keys(exe, kmers_of(more, k), k, key_length)
    good_heavy = np.flatnonzero((elected["key"] == np.uint64(key_value(heavy))) & (elected["tie"] == 0))
    for strings, good, copies in ((candidates, good_light, LIGHT_COPIES), (more, good_heavy, HEAVY_COPIES)):
        done = 0
        for i in good:
            done += add(strings[int(i)])
            if done == copies:
                break
        assert done == copies, (done, good.size)
    return seqs


def extension_of(k, m, key_length, layer, exe):
    """-> what make_inputs is to put behind the point's own strings for this layer (None: nothing)"""
    plain, pair = PLAIN_BASES.get((layer, k, m, key_length), 0), COLLIDING.get((layer, k, m, key_length))
    if not plain and not pair:
        return None

    def extend(seqs):
        if plain:
            seqs = with_plain_strings(seqs, k, plain, 9300 * k + m)
        if pair:
            seqs = with_colliding_keys(seqs, k, key_length or key_length_of(k, m), pair, exe, 9400 * k + m)
        return seqs

    return extend


def colliding_gate(pt, key_length, pair, exe):
    """what the table's key election makes of the two planted keys over the whole dictionary (on the CPU, tests/cpp/table_keys.cpp over
    every k-mer): the first is the key of the first LIGHT_RUN k-mers of LIGHT_COPIES strings -- as many occurrences, an inline slot each --, the second of
    HEAVY_COPIES strings of one k-mer; and the two keys hash to one fingerprint and one first bucket for every number of buckets -> the counts"""
    k = pt.k
    L = key_length or key_length_of(k, pt.m)
    elected = table_keys(exe, kmers_of(pt.sequences, k), k, L)
    string_of, sizes = string_of_ids(pt.case.gt, k)
    first = np.concatenate([[0], np.cumsum(sizes)[:-1]])  # the id of every string's first k-mer
    counts = {}
    for name, motif in zip(("light", "heavy"), pair):
        mine = np.flatnonzero((elected["key"] == np.uint64(key_value(motif))) & (elected["tie"] == 0))
        strings = np.unique(string_of[mine])
        if name == "light":  # the first LIGHT_RUN k-mers of LIGHT_COPIES strings that go on behind them
            assert strings.size == LIGHT_COPIES and (sizes[strings] == k + 1).all(), (name, motif, mine.size)
            assert mine.tolist() == sorted(int(first[s]) + j for s in strings for j in range(LIGHT_RUN)), (name, motif, mine.tolist())
        else:  # one string of one k-mer each
            assert mine.size == strings.size == HEAVY_COPIES and (sizes[strings] == 1).all(), (name, motif, mine.size)
        counts[name] = int(strings.size)
    assert LIGHT_COPIES <= 4 < HEAVY_COPIES
    fingerprint, word = table_hash([key_value(motif) for motif in pair])
    assert fingerprint[0] == fingerprint[1] and all(share_a_bucket(pair, buckets) for buckets in range(BUCKETS[0], BUCKETS[1] + 1))
    counts["fingerprint"] = int(fingerprint[0])
    return counts


def share_a_bucket(pair, buckets):
    """choice 0 of the two keys in a keys' region of `buckets` buckets (device_layout.hpp: sk_hash)"""
    _, word = table_hash([key_value(motif) for motif in pair])
    return int((word[0] * np.uint64(buckets)) >> np.uint64(32)) == int((word[1] * np.uint64(buckets)) >> np.uint64(32))


# ---- the probe sets ----------------------------------------------------------------------------------------------------------------------
def kmer_reads(sequences, k):
    """set 1: k-mer i of the dictionary (the strings in order) as a read, reverse-complemented for odd i"""
    reads = []
    for s in sequences:
        for a in range(len(s) - k + 1):
            r = s[a:a + k]
            reads.append(revcomp(r) if len(reads) & 1 else r)
    return reads


def window_reads(sequences, k):
    """set 2: 2k + 8 bases from every string that long, at one stride over all their places, base k + 3 substituted (the substitute
    rotates through the other three bases), every other window on the other strand -> (reads, which are reverse-complemented)"""
    L = 2 * k + 8
    places = [(i, a) for i, s in enumerate(sequences) for a in range(len(s) - L + 1)]
    stride = max(1, len(places) // 2200)
    reads, backward = [], []
    for j, (i, a) in enumerate(places[::stride]):
        w = sequences[i][a:a + L]
        sub = "ACGT"[("ACGT".index(w[k + 3]) + 1 + j % 3) % 4]
        w = w[:k + 3] + sub + w[k + 4:]
        reads.append(revcomp(w) if j & 1 else w)
        backward.append(bool(j & 1))
    return reads, np.array(backward)


class Probe:
    """one probe set: reads of one length, and everything the references say about them"""


def oracle_flat(oracle, reads):
    """the oracle's restated state machine over every read, each on its own -> its per-k-mer results back to back"""
    return np.concatenate([oracle.streaming_read(r) for r in reads])


def truth_flat(gt, reads, length, k):
    """GroundTruth.lookup (the input strings, sorted) of every k-mer of every read -> the ids, in order. The reads are `length` bases of
    A, C, G, T each: their k-mers are packed as one matrix"""
    W = 1 if k <= 31 else 2
    b = np.frombuffer("".join(reads).encode("ascii"), dtype=np.uint8).reshape(len(reads), length)
    assert np.isin(b, np.frombuffer(b"ACGT", dtype=np.uint8)).all()
    codes = ((b >> 1) & 3).astype(np.uint64)  # A0 C1 T2 G3
    q = pack(np.lib.stride_tricks.sliding_window_view(codes, k, axis=1).reshape(-1, k), W).reshape(-1, W)
    uniq, inverse = np.unique(q, axis=0, return_inverse=True)
    uniq = np.ascontiguousarray(uniq).reshape(-1)
    there = gt.lookup(uniq, False)["kmer_id"]
    back = gt.lookup(packed_revcomp(uniq, k, W), False)["kmer_id"]
    return np.where(there != INVALID, there, back)[inverse.reshape(-1)]


def best_of_records(offsets, runs, n_reads):
    """per read the longest of its records, among equals the first; 32 zero bytes without one"""
    best = np.zeros(n_reads, dtype=runs.dtype)
    if runs.size:
        read = np.repeat(np.arange(n_reads), np.diff(offsets.astype(np.int64)))
        order = np.lexsort((np.arange(runs.size), -(runs["num_kmers"] & LENGTH).astype(np.int64), read))  # by read, the longest first, the earlier first
        first = np.ones(order.size, dtype=bool)
        first[1:] = read[order][1:] != read[order][:-1]
        best[read[order][first]] = runs[order][first]
    return best


def make_probe(pt, reads, length, seed):
    """the references of one probe set, on the CPU: the oracle's state machine read by read against GroundTruth.lookup, and numpy over
    the oracle's results for every form -- the run rule for the records, then sums, classes and best run twice each"""
    import sshash_amd
    from gpu_cover_worker import bitmap_of
    from gpu_depth_worker import depth_of
    from gpu_forms_later import best_from_records, rows_from_records
    from gpu_classes_worker import labels_for

    case, k = pt.case, pt.k
    n_kmers, n, per = case.gt.num_kmers, len(reads), length - k + 1
    pb = Probe()
    pb.reads, pb.length = reads, length
    res = oracle_flat(case.oracle, reads)
    assert res.size == n * per
    ids, sid, ori = res["kmer_id"], res["string_id"], res["kmer_orientation"].astype(np.int64)
    truth = truth_flat(case.gt, reads, length, k)
    bad = np.flatnonzero(ids != truth)
    assert bad.size == 0, ("the oracle's ids against GroundTruth.lookup", bad[:5].tolist(), ids[bad[:5]].tolist(), truth[bad[:5]].tolist())
    pb.ids, pb.ori = ids.reshape(n, per), ori.reshape(n, per)
    # the run rule: a positive k-mer continues the run of the k-mer before it in its read iff that one is positive, in the same string, and its id is that one's + that one's orientation
    hit = ids != INVALID
    follows = np.zeros(ids.size, dtype=bool)
    follows[1:] = hit[1:] & hit[:-1] & (sid[1:] == sid[:-1]) & (ids[1:].astype(np.int64) == ids[:-1].astype(np.int64) + ori[:-1])
    follows[::per] = False  # (a read's first k-mer)
    kind = np.where(hit, np.where(follows, 3, 2), 1).reshape(n, per)
    pb.kind = kind
    pb.rows = np.stack([np.full(n, per), (kind >= 2).sum(1), (kind == 1).sum(1), np.zeros(n, dtype=np.int64), (kind == 2).sum(1), (kind == 3).sum(1)], axis=1).astype(np.uint64)
    pb.totals = pb.rows.sum(0)
    rep = case.oracle.streaming_query(reads)
    assert [rep[c] for c in COLUMNS] == pb.totals.tolist(), "the oracle's report against its per-k-mer results"
    starts = np.flatnonzero(hit & ~follows)
    run_of = np.cumsum(hit & ~follows) - 1
    runs = np.zeros(starts.size, dtype=sshash_amd.RUN_DTYPE)
    runs["kmer_id"], runs["string_id"], runs["kmer_id_in_string"] = ids[starts], sid[starts], res["kmer_id_in_string"][starts]
    runs["read_pos"] = starts % per
    runs["num_kmers"] = np.bincount(run_of[hit], minlength=starts.size).astype(np.uint32) | np.where(ori[starts] < 0, BACKWARD, np.uint32(0))
    pb.offsets = np.zeros(n + 1, dtype=np.uint64)
    pb.offsets[1:] = np.cumsum(np.bincount(starts // per, minlength=n))
    pb.runs = runs
    assert int(pb.offsets[-1]) == runs.size == int(pb.totals[4])
    pb.cover, pb.depth = bitmap_of(ids, (n_kmers + 63) // 64), depth_of(ids, n_kmers)
    # the sums: values[ids].sum() per read, and P[hi] - P[lo] over the run records
    _, pb.values, _ = sums_cases(n_kmers, seed)[0]
    read_of_hit = np.flatnonzero(hit) // per
    pb.sums = np.zeros(n, dtype=sshash_amd.READ_SUM_DTYPE)
    np.add.at(pb.sums["sum"], read_of_hit, pb.values.astype(np.uint64)[ids[hit].astype(np.int64)])
    np.add.at(pb.sums["positive_kmers"], read_of_hit, np.uint64(1))
    assert rows_from_runs(pb.offsets, runs, pb.values, 0, n_kmers).tobytes() == pb.sums.tobytes(), "sums: P[hi] - P[lo] over the run records against values[ids].sum()"
    # the classes: id -> string (the strings' lengths) -> label per k-mer, and labels[string_id] += length over the run records
    string_of, sizes = string_of_ids(case.gt, k)
    rng = np.random.default_rng(seed + 1)
    pb.labelled = [("mod / 3", 3, labels_for("mod", sizes.size, 3, rng)), ("random / 65", 65, labels_for("random", sizes.size, 65, rng))]
    pb.classes = {}
    for name, C, labels in pb.labelled:
        label = labels[string_of[ids[hit].astype(np.int64)]].astype(np.int64)
        rows = np.zeros((n, C), dtype=np.uint32)
        np.add.at(rows, (read_of_hit[label < C], label[label < C]), np.uint32(1))
        assert (rows_from_records(pb.offsets, runs, labels, C) == rows).all(), f"classes {name}: the run records against id -> string -> label per k-mer"
        pb.classes[name] = rows
    assert (pb.classes["random / 65"].sum(1) <= pb.rows[:, 1]).all() and (pb.classes["mod / 3"].sum(1) == pb.rows[:, 1]).all()
    # the best run: the argmax with the tie rule in one numpy pass, and read by read for the first 2000 reads
    pb.best = best_of_records(pb.offsets, runs, n)
    few = min(n, 2000)
    assert best_from_records(pb.offsets[:few + 1], runs).tobytes() == pb.best[:few].tobytes(), "the best run: one pass against read by read"
    return pb


def probe_gate(pt):
    """the two probe sets of the point's dictionary and their references (on the CPU) -> what they hold"""
    case, k = pt.case, pt.k
    n_kmers = case.gt.num_kmers
    seed = 7100 * k + 10 * pt.m + int(pt.canonical)
    # ---- set 1 ----
    reads = kmer_reads(pt.sequences, k)
    assert len(reads) == n_kmers
    one = pt.kmer_probe = make_probe(pt, reads, k, seed)
    assert (one.ids[:, 0] == np.arange(n_kmers, dtype=np.uint64)).all(), "read i of set 1 is k-mer i"
    assert (one.kind == 2).all() and (one.rows[:, 4] == 1).all(), "every read of set 1 is one search"
    backward = int((one.ori[:, 0] < 0).sum())
    assert backward == n_kmers // 2 and (one.ori[1::2, 0] < 0).all(), "half of set 1 is found backward: the odd ids"
    # ---- set 2 ----
    reads, flipped = window_reads(pt.sequences, k)
    two = pt.window_probe = make_probe(pt, reads, 2 * k + 8, seed + 2)
    assert WINDOWS[0] <= len(reads) <= WINDOWS[1], len(reads)
    expected = np.array([True] * 4 + [False] * k + [True] * 5)
    positive = two.ids != INVALID
    positive = np.where(flipped[:, None], positive[:, ::-1], positive)  # (a window on the other strand holds its k-mers in the other order)
    as_expected = (positive == expected).all(axis=1) & (two.rows[:, 4] == 2)  # (and its positive k-mers are two runs)
    assert as_expected.mean() >= PATTERN_SHARE, (int(as_expected.sum()), len(reads))
    assert (two.rows[:, 2] > 0).any() and int(flipped.sum()) == len(reads) // 2
    return {"kmer_reads": n_kmers, "kmer_reads_backward": backward, "windows": len(reads), "windows_as_expected": int(as_expected.sum()),
            "windows_with_another_kmer_of_the_dictionary": int((two.rows[:, 1] > 9).sum()), "window_runs": int(two.totals[4]),
            "window_negatives": int(two.totals[2])}


# ---- the device --------------------------------------------------------------------------------------------------------------------------
def lookup_ids(d, pb, k):
    """streaming_lookup: the ids of every k-mer of every read, as one array (the per-read results are views of it, a read's k-mers at
    the offset of its first base)"""
    per_read, report = d.streaming_lookup(pb.reads)
    whole = per_read[0].kmer_id.base
    n, per = len(pb.reads), pb.length - k + 1
    assert whole is not None and whole.size == n * pb.length and len(per_read) == n
    at = (np.arange(n) * pb.length)[:, None] + np.arange(per)[None, :]
    return whole[at], report


def probe_pass(d, pt, pb, what, segmented):
    """one probe set through every form, host call and device call, uncut; `segmented`: once more at S = SEGMENT for rows, run records
    and classes. No Python loop per read here: the helpers compare whole arrays"""
    import sshash_amd
    from gpu_best_run_worker import device_best, host_best
    from gpu_best_run_worker import same as same_best
    from gpu_classes_worker import device_classes, host_classes
    from gpu_classes_worker import same as same_rows
    from gpu_per_read_worker import report_row
    from gpu_runs_segments_worker import device_same, host_same
    from gpu_runs_worker import check_both
    from gpu_segments_worker import device_rows_guarded, everything, launches, same
    from gpu_sums_worker import device_prefix, device_sums
    from gpu_sums_worker import same as same_sums

    reads, totals = pb.reads, pb.totals
    d.set_read_segments(sshash_amd.SEGMENTS_OFF, device_calls=True)
    at = launches(d)
    host = {"totals": totals, "rows": pb.rows, "rows_report": totals, "cover": pb.cover, "cover_report": totals, "depth": pb.depth, "depth_report": totals}
    same(everything(d, reads, False), host, f"{what}: uncut, host calls")
    same(everything(d, reads, True), dict(host, rows_no_report=pb.rows, cover_no_report=pb.cover, depth_no_report=pb.depth), f"{what}: uncut, device calls")
    check_both(d, reads, pb.offsets, pb.runs, f"{what}: run records")
    got, rep = d.streaming_sums(reads, pb.values)
    same_sums(got, pb.sums, f"{what}: sums, host call")
    assert (report_row(rep) == totals).all(), f"{what}: sums, host call: the report"
    prefix = device_prefix(d, pb.values)
    got, rep = device_sums(d, reads, prefix[1], report=[0] * 6)
    same_sums(got, pb.sums, f"{what}: sums, device call")
    assert (rep == totals).all(), f"{what}: sums, device call: the report"
    del prefix

    def classes(where):
        for name, C, labels in pb.labelled:
            got, rep = host_classes(d, reads, labels, C)
            same_rows(got, pb.classes[name], f"{what}: classes {name}, {where}host call")
            assert (rep == totals).all(), f"{what}: classes {name}, {where}host call: the report"
            got, rep = device_classes(d, reads, labels, C, report=[0] * 6)
            same_rows(got, pb.classes[name], f"{what}: classes {name}, {where}device call")
            assert (rep == totals).all(), f"{what}: classes {name}, {where}device call: the report"

    classes("")
    got, rep = host_best(d, reads)
    same_best(got, pb.best, f"{what}: best run, host call")
    assert (rep == totals).all(), f"{what}: best run, host call: the report"
    got, rep = device_best(d, reads, report=[0] * 6)
    same_best(got, pb.best, f"{what}: best run, device call")
    assert (rep == totals).all(), f"{what}: best run, device call: the report"
    got, rep = lookup_ids(d, pb, pt.k)
    bad = np.argwhere(got != pb.ids)
    assert bad.size == 0, (f"{what}: streaming_lookup, (read, k-mer)", bad[:5].tolist())
    assert (report_row(rep) == totals).all(), f"{what}: streaming_lookup: the report"
    assert launches(d) == at, "SEGMENTS_OFF launched over segments"
    if segmented:
        d.set_read_segments(SEGMENT, device_calls=True)
        where = f"S = {SEGMENT}, "
        rows, rep = d.streaming_query_per_read(reads)
        same({"rows": rows, "report": report_row(rep)}, {"rows": pb.rows, "report": totals}, f"{what}: {where}rows, host call")
        rows, rep = device_rows_guarded(d, reads, report=[0] * 6)
        same({"rows": rows, "report": rep}, {"rows": pb.rows, "report": totals}, f"{what}: {where}rows, device call")
        host_same(d, reads, pb.offsets, pb.runs, totals, f"{what}: {where}run records")
        device_same(d, reads, int(pb.offsets[-1]), pb.offsets, pb.runs, f"{what}: {where}run records", report=[0] * 6, want_report=totals)
        classes(where)
        assert launches(d) >= at + 4 + 2 * len(pb.labelled), f"{what}: S = {SEGMENT} did not launch over segments"
        d.set_read_segments(sshash_amd.SEGMENTS_OFF, device_calls=True)


def default_stats(index_path):
    """what device_stats() shows for a plain upload of the same index file at the default density: a second handle, and the density
    switch taken out of the environment for the time of its upload"""
    import sshash_amd

    held = os.environ.pop("SSHASH_AMD_SK_DENSITY", None)
    try:
        other = sshash_amd.Dictionary.load(index_path).to_device(0)
        st = other.device_stats(0)
        other.close()
    finally:
        if held is not None:
            os.environ["SSHASH_AMD_SK_DENSITY"] = held
    return st


def replica_of(layer, k, m, key_length, index_path, seen):
    """-> (upload, replica) for check_flavour: how the layer's replica is uploaded, and what device_stats() has to show of it before the
    first streaming call; the figures go into `seen`"""
    def upload(dictionary):
        return dictionary.to_device(0, table_shards=SHARDS, table_shard_id=SHARD_ID) if layer == "shard" else dictionary.to_device(0)

    def replica(st, what):
        what = f"{layer}, {what}"
        seen.update({name: st[name] for name in ("sk_slots", "sk_keys", "sk_deferred_keys", "sk_heavy_kmers", "sk_load_factor")})
        assert os.environ.get("SSHASH_AMD_TEST_HOOKS", "") == ENVIRONMENT[layer].get("SSHASH_AMD_TEST_HOOKS", ""), f"{what}: the hooks in the environment"
        assert os.environ.get("SSHASH_AMD_SK_DENSITY", "") == ENVIRONMENT[layer].get("SSHASH_AMD_SK_DENSITY", ""), f"{what}: the density in the environment"
        if layer == "packed":
            assert st["sk_load_factor"] > 0.75 and st["sk_deferred_keys"] >= DEFERRED_FLOOR[layer] and st["sk_heavy_kmers"] > 0, (what, st)
            assert (k, m, key_length) in HEAVY
            if (layer, k, m, key_length) in COLLIDING:
                # (sktable.hip: two entries a bucket in the k-mers' region at k > 31, 1.2 places per k-mer and eight buckets more; the rest are the keys' buckets, two slots each)
                assert k > 31
                buckets = (st["sk_slots"] - 2 * (int(st["sk_heavy_kmers"] * 1.2 / 2) + 8)) // 2
                seen["key_buckets"] = buckets
                assert BUCKETS[0] <= buckets <= BUCKETS[1] and share_a_bucket(COLLIDING[(layer, k, m, key_length)], buckets), (what, buckets, st)
        elif layer == "compact":
            plain = default_stats(index_path)
            seen["default_load_factor"] = plain["sk_load_factor"]
            assert st["sk_slots"] > 0 and st["sk_deferred_keys"] >= DEFERRED_FLOOR[layer], (what, st)
            assert plain["sk_slots"] > st["sk_slots"] and st["sk_load_factor"] > plain["sk_load_factor"] > 0, (what, st, plain)
        else:
            whole = default_stats(index_path)
            seen["whole_sk_keys"] = whole["sk_keys"]
            assert 0.15 * whole["sk_keys"] <= st["sk_keys"] <= 0.6 * whole["sk_keys"], (what, st["sk_keys"], whole["sk_keys"])

    return upload, replica


def main():
    import tempfile

    k, m, key_length, layer, exe, scratch = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), sys.argv[4], sys.argv[5], sys.argv[6]
    cpu_only = "--cpu-only" in sys.argv[7:]
    assert (k, m, key_length, layer) in MATRIX
    out, seconds = {}, {}
    with tempfile.TemporaryDirectory(dir=scratch) as tmp:
        for canonical in (False, True):
            name = "canonical" if canonical else "regular"
            t0 = time.time()
            pt = make_inputs(k, m, key_length, canonical, exe, tmp, extend=extension_of(k, m, key_length, layer, exe))
            out[name] = gate(pt)
            out[name]["probes"] = probe_gate(pt)
            if (layer, k, m, key_length) in COLLIDING:
                out[name]["colliding_keys"] = colliding_gate(pt, key_length, COLLIDING[(layer, k, m, key_length)], exe)
            t1 = time.time()
            if not cpu_only:
                seen = {}
                upload, replica = replica_of(layer, k, m, key_length, pt.case.index_path, seen)

                def then(d, what, pt=pt):
                    probe_pass(d, pt, pt.kmer_probe, f"{layer}, {what}: every k-mer as a read", False)
                    probe_pass(d, pt, pt.window_probe, f"{layer}, {what}: substituted windows", True)

                out[name].update(check_flavour(pt, key_length, "table", upload=upload, replica=replica, then=then))
                out[name]["stats"] = seen
            seconds[name] = [round(t1 - t0, 2), round(time.time() - t1, 2)]  # (inputs and references on the CPU, calls on the device)
    print(json.dumps({"ok": True, "k": k, "m": m, "key_length": key_length, "layer": layer, "cpu_only": cpu_only, "dictionaries": out, "seconds": seconds}))


if __name__ == "__main__":
    main()
