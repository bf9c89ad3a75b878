#!/usr/bin/env python
"""Worker of tests/test_gpu_forms_sweep.py, and the input generator it shares with tests/test_forms_sweep_inputs.py: ALL TEN output
forms of the streaming run kernel -- the batch counters, the per-read rows, the run counts and records, the cover bitmap, the depth
deltas, the per-read sums over a value per k-mer, the per-read classes of the strings hit, the per-read best run, the run records over
segments -- and the segment machinery for long reads, at one point (k, m, length of the table's keys, replica layer), regular then
canonical. The run forms do arithmetic the per-k-mer forms never do (kmer_id = offset - string_id *
(k - 1), the first id of a backward run, a segment's end at + S + k - 1, the first invalid base of a window, the funnel shift of a
two-word seed), and the length of the table's keys is a parameter of its own (`hashed`, sk_key_persists); the points of the sweep are
where these change: k = 33 (one base in the second word; for the sums, the first k at which a run's two words of the prefix are added
where the run is measured and not at the end of the turn), m = k, m < 12, even m (a self-complementary m-mer ties the two strands), a
key length on either side of m.

One worker process = one point (the replica layer and the key length are read from the environment when a replica is uploaded; the
worker sets nothing itself and asserts from device_stats() that the setting took). On the CPU first (gate): the reads hold every kind
of read, run and seam the kernels have a branch for, and the ids of the oracle's restated state machine equal GroundTruth.lookup of
every valid k-mer of every read -- two references, neither of them the library's GPU path. The sums have two references of their own,
both numpy over the oracle's results: values[ids].sum() per read, and the kernel's formula restated -- per run record P[hi] - P[lo] over
P = cumsum(values) --, asserted equal, over values under which a slip by one id at either end of any run changes the sum. The three
forms that came last consume a hit's string id in ways of their own -- an index into the labels; word 2 of a record stored at the read's
own index; under segments, a record whose place the joined[] bytes decide -- and have two references each as well
(tests/gpu_forms_later.py): the best run as the argmax with the tie rule over the oracle's run records and over the run rule applied to
its per-k-mer results; the classes, for 3 and 65 classes under string id % C and under random labels a third of which are no class,
from the per-k-mer ids through id -> string -> label and from the run records; the run records over segments are the uncut records. The
reads hold what makes a wrong kernel show: ties for the longest run, a longest run that is not the first or is backward, reads of two
strings of different classes, k-mers of a masked label, runs that span three whole segments and more. Then every form through the host
and the device entry point, uncut, cut into segments of 1, 7 and 64 k-mers, and uncut again; all comparisons exact. Prints one JSON
line; any mismatch is an assertion error.

    python tests/gpu_forms_worker.py <k> <m> <key_length or 0> <layer: table|directory> <table_keys binary> <scratch dir> [--cpu-only]"""
from __future__ import annotations

import functools
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import numpy as np

from gpu_even_m_worker import POINTS as EVEN_POINTS
from gpu_even_m_worker import FLOOR, assert_floors, canonical_strings, key_length_of, kmers_of, make_point
from gpu_per_read_worker import COLUMNS, random_dna, revcomp, synthetic_reads
from gpu_routing_worker import revcomp as packed_revcomp

INVALID = np.uint64(0xFFFFFFFFFFFFFFFF)
ODD_POINTS = [(21, 11), (23, 23), (27, 9), (29, 17), (31, 7), (31, 27), (31, 31), (33, 13), (35, 31), (41, 21), (47, 15),
              (55, 19), (61, 29), (63, 31)]  # tests/test_gpu_km_sweep.py: POINTS
KEY_POINTS = [(31, 21, 25), (31, 21, 17), (31, 13, 12), (31, 13, 30), (31, 20, 14), (21, 11, 20), (15, 7, 14), (33, 13, 31), (47, 15, 31),
              (63, 25, 12), (63, 31, 20), (63, 17, 17)]  # (k, m, SSHASH_AMD_SK_M)
DIRECTORY_POINTS = [(23, 23), (31, 12), (33, 13), (35, 30), (55, 19), (63, 16)]
MATRIX = ([(k, m, 0, "table") for k, m in ODD_POINTS + EVEN_POINTS] + [(k, m, L, "table") for k, m, L in KEY_POINTS]
          + [(k, m, 0, "directory") for k, m in DIRECTORY_POINTS])  # (k, m, key length or 0, layer): one worker each
LAYERS = {  # name -> (environment, what device_stats() must show)
    "table": ({}, lambda st: st["sk_slots"] > 0),
    "directory": ({"SSHASH_AMD_SKTABLE": "0", "SSHASH_AMD_DIRECTORY": "1"}, lambda st: st["sk_slots"] == 0 and st["directory_sectors"] > 0),
}
SEGMENT_SIZES = (1, 7, 64)
LONG_STRINGS, LONG_LENGTHS = 12, (800, 1501)  # reads of 300 - 600 bases are cut out of these at every k
REPEATS = 4096
# a planted m-mer needs k - m >= ROOM bases around it: conftest.skewed_sequences redraws the flanks of every copy until its k-mers are new, and a
# hundred copies of one m-mer cannot be a hundred distinct k-mers at every place in the window when 4^(k - m) is small (it never returns at k - m = 1)
ROOM = 4
JUMP = 12  # k-mers on either side of the jump of a jump read
# (k, m, key length or 0) of the table layer where device_stats()["sk_heavy_kmers"] > 0: k-mers under a key with more occurrences than
# the table lists, answered by the complete path. Found on the first run on an MI355X and held since.
HEAVY = {(21, 11, 0), (27, 9, 0), (29, 17, 0), (31, 7, 0), (31, 27, 0), (33, 13, 0), (35, 31, 0), (41, 21, 0), (47, 15, 0), (61, 29, 0), (63, 31, 0),
         (15, 4, 0), (31, 6, 0), (31, 8, 0), (47, 20, 0), (63, 30, 0), (31, 21, 25), (31, 21, 17), (31, 13, 12), (31, 20, 14), (47, 15, 31), (63, 25, 12),
         (63, 31, 20)}


def environment_of(key_length, layer):
    """what the test puts into the worker's environment (every other SSHASH_AMD_* setting is taken out first)"""
    env = dict(LAYERS[layer][0])
    if key_length:
        env["SSHASH_AMD_SK_M"] = str(key_length)
    return env


# ---- the dictionary's strings ----------------------------------------------------------------------------------------------------------
def _adder(seqs, k):
    """-> add(t): appends t to seqs if its canonical k-mers are pairwise distinct and new (no dictionary may hold a k-mer twice)"""
    seen = set()
    for s in seqs:
        seen |= canonical_strings(s, k)

    def add(t):
        mine = canonical_strings(t, k)
        if len(mine) != len(t) - k + 1 or (mine & seen):
            return False
        seen.update(mine)
        seqs.append(t)
        return True

    return add


def jump_string(k, seed):
    """-> (A + R + B + R + C, where the two R start): one string that holds the same k - 1 bases R twice. Its k-mers are distinct (the bases
    around the two R differ), but a read can step from the k-mer that ends with the first R to the k-mer that starts with the second:
    two neighbours in the read, both in the dictionary and in the same string, that are NOT neighbours in the string -- the one place
    where whether a k-mer extends a run is decided by the ids and not by whether the k-mer before it was found"""
    rng = np.random.default_rng(seed + 77)
    while True:
        a, r, b, c = (random_dna(rng, n) for n in (k + JUMP, k - 1, k + JUMP, k + JUMP))
        if len({a[-1], b[-1]}) == 2 and len({b[0], c[0]}) == 2:  # (or the k-mers around the two R were the same)
            return a + r + b + r + c, (len(a), len(a) + len(r) + len(b))


def jump_reads(k, seed):
    """the reads that jump inside jump_string: forward from the first R to behind the second, back from the second to behind the first,
    and both on the other strand"""
    s, (first, second) = jump_string(k, seed)
    there = s[first - JUMP:first + k - 1] + s[second + k - 1:second + k - 1 + JUMP]
    back = s[second - JUMP:second + k - 1] + s[first + k - 1:first + k - 1 + JUMP]
    return [there, back, revcomp(there), revcomp(back)]


def with_long_strings(seqs, k, seed):
    """seqs and, behind them, LONG_STRINGS random strings of 800 - 1500 bases and the jump string"""
    rng = np.random.default_rng(seed)
    seqs = list(seqs)
    add = _adder(seqs, k)
    for n in rng.integers(LONG_LENGTHS[0], LONG_LENGTHS[1], LONG_STRINGS):
        while not add(random_dna(rng, int(n))):
            pass
    assert add(jump_string(k, seed)[0]), "the jump string holds a k-mer twice, or one of another string"
    return seqs


_ODD = {}


@functools.lru_cache(maxsize=None)
def _skewed(k, m, n_heavy, n_mid):
    from conftest import skewed_sequences

    return skewed_sequences(k, m, seed=k + m, n_heavy=n_heavy, n_mid=n_mid, n_plain=0)


def odd_sequences(k, m, key_length):
    """an odd m: random strings of ragged lengths, the shortest exactly one k-mer long (tests/test_gpu_km_sweep.py, at the size of the
    even-m inputs), the long strings, and what conftest.skewed_sequences plants where it applies: m-mers that win the minimizer election
    of any window (MIDLOAD and HEAVYLOAD buckets; m < k, or the copies of one m-mer were copies of one k-mer) and m-mers that win the
    table's key election (keys with a list of occurrences, and with more than the table lists) -- the latter again at the length of the
    table's keys where that is not m. Deterministic, the same for both flavours."""
    if (k, m, key_length) in _ODD:
        return _ODD[(k, m, key_length)]
    rng = np.random.default_rng(9000 * k + m)
    seqs = []
    add = _adder(seqs, k)
    target = 1500 if k <= 15 else 3500
    for n in [k, k + 1, 2 * k - 1, 2 * k] + [int(x) for x in rng.integers(k, 6 * k, max(12, target // (5 * k // 2)))]:
        while not add(random_dna(rng, n)):
            pass
    seqs[:] = with_long_strings(seqs, k, 9100 * k + m)
    add = _adder(seqs, k)
    planted = 0
    if k - m >= ROOM:
        for t in _skewed(k, m, 70, 7):
            planted += add(t)
    L = key_length or key_length_of(k, m)
    if L != m and k - L >= ROOM:
        more = _skewed(k, L, 0, 0)
        # what is left of the minimizer part with no heavy and no mid-load copies: the two strings of the third motif and the single k-mer;
        # behind them the 100 + 9 + 2 copies of the three table motifs
        assert [len(t) for t in more[:3]] == [k + 3 + L + 2 * k] * 2 + [k] and len(more) == 3 + 111, [len(t) for t in more[:4]]
        assert any(more[3][at:at + L] in more[4] for at in range(k + 3, k + 30)), "the strings behind them share a motif of the key's length"
        table = sum(add(t) for t in more[3:])
        assert table >= 100, (k, L, table)
        planted += table
    assert k - m < ROOM or planted >= 100, (k, m, planted)
    _ODD[(k, m, key_length)] = seqs
    return seqs


def two_string_reads(seqs, k, seed):
    """reads for the forms that tell a read's strings and its runs apart (the classes, the best run): pieces of two strings whose ids differ
    modulo 3 and modulo 65 back to back, the first run the longer (k + 40 bases, then k + 30) or the second (k + 10, then k + 60), every other
    one on the other strand; and a string's prefix with one substitution at base k + 5: a run of 6 k-mers, k k-mers that are nowhere, the rest"""
    rng = np.random.default_rng(seed)
    usable = [i for i, s in enumerate(seqs) if len(s) >= k + 60]
    reads = []
    for j in range(16):
        while True:
            a, b = (int(i) for i in rng.choice(usable, 2, replace=False))
            if (a - b) % 3 and (a - b) % 65:
                break
        first, second = ((k + 40, k + 30), (k + 10, k + 60))[j % 2]
        r = seqs[a][:first] + seqs[b][-second:]
        reads.append(revcomp(r) if j % 4 >= 2 else r)
    lengthy = [s for s in seqs if len(s) >= 3 * k + 30]
    for j in range(4):
        r = list(lengthy[int(rng.integers(0, len(lengthy)))][:3 * k + 30])
        r[k + 5] = "ACGT"[("ACGT".index(r[k + 5]) + 1) % 4]
        reads.append(revcomp("".join(r)) if j % 2 else "".join(r))
    return reads


class Point:
    """one dictionary with its reads and everything the references say about them (on the CPU)"""


def long_read_of(sequences, with_n):
    """the dictionary's strings back to back on alternating strands, again and again until the read has more than 2^16 bases"""
    parts, size, i = [], 0, 0
    while size <= (1 << 16) + 500:
        s = sequences[i % len(sequences)]
        parts.append(revcomp(s) if (i + i // len(sequences)) % 2 else s)  # (a string comes on both strands as the rounds go)
        size += len(s) + int(with_n)
        i += 1
    return ("N" if with_n else "").join(parts)


def make_inputs(k, m, key_length, canonical, exe, scratch, extend=None):
    """-> Point: the dictionary (conftest.Case), the reads, the long reads and the repeated read. `extend`: strings -> the strings with
    more behind them (tests/gpu_walks_worker.py; None: the sweep's dictionary)"""
    from conftest import Case
    from gpu_segments_worker import make_reads

    pt = Point()
    pt.k, pt.m, pt.canonical, pt.W, pt.floors = k, m, canonical, 1 if k <= 31 else 2, None
    if m % 2 == 0:
        even = make_point(k, m, canonical, exe, scratch, key_length=key_length or None,
                          extend=lambda seqs: (extend or list)(with_long_strings(seqs, k, 9100 * k + m)))
        pt.floors = assert_floors(even)  # at least FLOOR tying k-mers that the reads hold and the dictionary contains, of every kind
        pt.case, own = even.case, even.reads
    else:
        seqs = (extend or list)(odd_sequences(k, m, key_length))
        pt.case, own = Case(f"forms_k{k}_m{m}_{int(canonical)}", seqs, k, m, canonical, scratch), []
    seqs = pt.sequences = pt.case.sequences
    pt.jumps = jump_reads(k, 9100 * k + m)
    reads = make_reads(seqs, k) + synthetic_reads(seqs, k, 160, seed=k + m, read_len=3 * k) + own + pt.jumps
    for s in seqs:
        reads += [s, revcomp(s)]
    pt.reads = reads + two_string_reads(seqs, k, 9200 * k + m)  # (behind the others: what the references say of those stays)
    pt.long_reads = [long_read_of(seqs, False), long_read_of(seqs, True)]
    assert all(len(r) > (1 << 16) for r in pt.long_reads)
    hot = next(s for s in seqs if len(s) >= 800)[40:40 + k + 100]
    pt.repeated = [hot] * REPEATS
    return pt


# ---- the references ----------------------------------------------------------------------------------------------------------------------
def classify(oracle, reads, k):
    from gpu_segments_worker import per_kmer

    per = [per_kmer(oracle, r, k) for r in reads]
    return [p[0] for p in per], [p[1] for p in per], [p[2] for p in per]


def rows_of(kinds):
    return np.array([[kd.size, (kd >= 2).sum(), (kd == 1).sum(), (kd == 0).sum(), (kd == 2).sum(), (kd == 3).sum()] for kd in kinds], dtype=np.uint64).reshape(-1, 6)


_TRUTH = {}


def truth_ids(gt, sequences, reads, kinds, k):
    """GroundTruth.lookup (the input strings, sorted) of every valid k-mer of every read, in order -> the ids. The two flavours of a point
    have the same strings and the same reads, so the same truth: it is looked up once per process."""
    key = (k, hash(tuple(sequences)), hash(tuple(reads)))
    if key not in _TRUTH:
        _TRUTH.clear()
        _TRUTH[key] = _truth_ids(gt, reads, k)
    ids, valid_per_read = _TRUTH[key]
    assert valid_per_read == [int((kd != 0).sum()) for kd in kinds]  # (the oracle's idea of a valid k-mer is the input's)
    return ids


def _truth_ids(gt, reads, k):
    ok = np.zeros(256, dtype=bool)
    ok[list(b"ACGTacgt")] = True
    stretches, valid_per_read = [], []
    for r in reads:
        b = np.frombuffer(r.encode("ascii", "replace"), dtype=np.uint8)
        bad = np.flatnonzero(~ok[b])
        edges = np.concatenate([[-1], bad, [b.size]])
        mine = [r[int(a) + 1:int(e)] for a, e in zip(edges[:-1], edges[1:]) if e - a - 1 >= k]
        valid_per_read.append(sum(len(s) - k + 1 for s in mine))
        stretches += mine
    W = 1 if k <= 31 else 2
    q = kmers_of(stretches, k).reshape(-1, W)
    uniq, inverse = np.unique(q, axis=0, return_inverse=True)
    uniq = np.ascontiguousarray(uniq).reshape(-1)
    there = gt.lookup(uniq, False)["kmer_id"]  # (strand by strand, the other strand by numpy: GroundTruth turns a two-word k-mer base by base)
    back = gt.lookup(packed_revcomp(uniq, k, W), False)["kmer_id"]
    return np.where(there != INVALID, there, back)[inverse.reshape(-1)], valid_per_read


def string_of_ids(gt, k):
    """id -> string, from the strings' lengths alone"""
    sizes = (np.diff(gt.endpoints).astype(np.int64) - (k - 1))
    return np.repeat(np.arange(sizes.size), sizes), sizes


# ---- the sums: values, and two references in numpy ---------------------------------------------------------------------------------------
ALL_ONES = 0xFFFFFFFF
HALF = 1 << 31  # the threshold that about half of the random values pass
BACKWARD = 0x80000000


def sums_cases(n_kmers, seed):
    """-> [(name, values, at_least)]: full-range random values (a run of two already carries across 2^32 as often as not), whether
    they reach HALF, and all 0xFFFFFFFF"""
    v = np.random.default_rng(seed).integers(0, 1 << 32, n_kmers, dtype=np.uint64).astype(np.uint32)
    return [("random", v, 0), ("at least 2^31", v, HALF), ("all ones", np.full(n_kmers, ALL_ONES, dtype=np.uint32), 0)]


def run_words(runs, n_kmers):
    """per run record the two words of the prefix that the kernel reads (sums_run_anchor, sums_run_far), by orientation: the one that
    does not depend on the run's length -- id forward, id + 1 backward -- and the one that does -- id + n forward, id + 1 - n backward
    -> (anchor, far, n, forward). A backward run's ids go down from its first k-mer's."""
    n = (runs["num_kmers"] & np.uint32(BACKWARD - 1)).astype(np.int64)
    forward = (runs["num_kmers"] & np.uint32(BACKWARD)) == 0
    kmer_id = runs["kmer_id"].astype(np.int64)
    anchor = np.where(forward, kmer_id, kmer_id + 1)
    far = np.where(forward, kmer_id + n, kmer_id + 1 - n)
    assert (n >= 1).all() and (np.minimum(anchor, far) >= 0).all() and (np.maximum(anchor, far) <= n_kmers).all(), "a run outside the ids"
    return anchor, far, n, forward


def rows_from_runs(offsets, runs, values, at_least, n_kmers):
    """the sums form's own formula in numpy, over the run records: per read the sum over its runs of P[hi] - P[lo], P the exclusive
    prefix sums of the values in 64 bits, and of the runs' lengths"""
    import sshash_amd

    v = values.astype(np.uint64) if at_least == 0 else (values >= np.uint32(at_least)).astype(np.uint64)
    P = np.zeros(n_kmers + 1, dtype=np.uint64)
    np.cumsum(v, dtype=np.uint64, out=P[1:])
    anchor, far, n, forward = run_words(runs, n_kmers)
    worth = np.where(forward, P[far] - P[anchor], P[anchor] - P[far])  # (modulo 2^64, as the kernel)
    read = np.repeat(np.arange(offsets.size - 1), np.diff(offsets.astype(np.int64)))
    out = np.zeros(offsets.size - 1, dtype=sshash_amd.READ_SUM_DTYPE)
    np.add.at(out["sum"], read, worth)
    np.add.at(out["positive_kmers"], read, n.astype(np.uint64))
    return out


def neighbours_differ(runs, values, n_kmers):
    """under `values` a run [lo, hi) that is read one id too low or too high, at one end or at both, sums to something else: the values
    of the ids that would come in are not those of the ids that would go out, and none of them is zero. The ids below 0 and above the
    last do not exist: the runs that begin at id 0 or end at the last id are asked for what there is
    -> how many runs have no id below them, how many none above"""
    anchor, far, n, forward = run_words(runs, n_kmers)
    lo, hi = np.minimum(anchor, far), np.maximum(anchor, far)
    assert (hi - lo == n).all()
    v = values.astype(np.int64)
    below, above = lo > 0, hi < n_kmers
    assert (v[lo[below] - 1] != v[hi[below] - 1]).all(), "a run moved down by one id would sum to the same"
    assert (v[lo[above]] != v[hi[above]]).all(), "a run moved up by one id would sum to the same"
    assert (v[lo] != 0).all() and (v[hi - 1] != 0).all() and (v[lo[below] - 1] != 0).all() and (v[hi[above]] != 0).all(), "an end moved by one id would go unseen"
    return int((~below).sum()), int((~above).sum())


def sums_references(pt, cases, reads, ids, oracle):
    """-> ({name: rows}, (run_offsets, run records)) the rows of `reads` under every case, from the oracle's ids per k-mer; asserted equal to the rows from
    its run records"""
    from gpu_runs_worker import oracle_runs
    from gpu_sums_worker import flat_ids, rows_of
    from gpu_sums_worker import same as same_rows

    n_kmers = pt.case.gt.num_kmers
    flat = flat_ids(ids)
    offsets, runs = oracle_runs(oracle, reads)
    want = {}
    for name, values, at_least in cases:
        want[name] = rows_of(flat, len(reads), values, at_least)
        same_rows(rows_from_runs(offsets, runs, values, at_least, n_kmers), want[name], f"sums, {name}: P[hi] - P[lo] over the run records against values[ids].sum()")
    return want, (offsets, runs)


def gate(pt):
    """on the CPU, before any device call: every kind of read, run and seam is there, and the oracle's ids are the input's"""
    from gpu_cover_worker import bitmap_of
    from gpu_depth_worker import depth_of, runs_of
    from gpu_forms_later import references as later_references
    from gpu_segments_worker import kinds_of

    case, k, reads = pt.case, pt.k, pt.reads
    n_kmers = case.gt.num_kmers
    pt.kinds, pt.oris, pt.ids = classify(case.oracle, reads, k)
    found = kinds_of(reads, pt.kinds, pt.oris, k)  # (asserts every count positive: the kinds of reads and, for S of 1, 2, 7, 64, of seams)
    all_ids = np.concatenate(pt.ids)
    valid = np.concatenate(pt.kinds) != 0
    truth = truth_ids(case.gt, pt.sequences, reads, pt.kinds, k)
    bad = np.flatnonzero(all_ids[valid] != truth)
    assert bad.size == 0, ("the oracle's ids against GroundTruth.lookup", bad[:5].tolist(), all_ids[valid][bad[:5]].tolist(), truth[bad[:5]].tolist())
    assert (all_ids[~valid] == INVALID).all()
    lo, n, backward, read_of_run = runs_of(pt.ids)
    lengths = np.array([len(r) for r in reads])
    hits = np.array([int((ids != INVALID).sum()) for ids in pt.ids])
    kinds = {"forward": int((~backward & (n > 1)).sum()), "backward": int(backward.sum()), "runs_of_one": int((n == 1).sum()),
             "runs_of_64_and_more": int((n >= 64).sum()), "runs_from_id_0": int((lo == 0).sum()), "runs_to_the_last_id": int((lo + n == n_kmers).sum()),
             "reads_shorter_than_k": int(((lengths < k) & (lengths > 0)).sum()), "empty_reads": int((lengths == 0).sum()),
             "reads_without_a_hit": int(((lengths >= k) & (hits == 0)).sum()), "reads_with_N": sum("N" in r for r in reads)}
    assert all(v > 0 for v in kinds.values()), kinds
    # the jump reads: two neighbours in the read that are both found, in the same string, and not neighbours there -- a search, no extension
    jumps = 0
    for r in pt.jumps:
        res = case.oracle.streaming_read(r)
        ids, sid, ori = res["kmer_id"], res["string_id"], res["kmer_orientation"]
        assert (ids != INVALID).all() and (sid == sid[0]).all() and res.size == 2 * JUMP, "a jump read lies in one string"
        step = ids[1:].astype(np.int64) - ids[:-1].astype(np.int64)
        assert (step != ori[:-1]).sum() == 1 and abs(int(step[JUMP - 1])) > 1, "a jump read jumps once, behind its first JUMP k-mers"
        assert case.oracle.streaming_query([r])["num_searches"] == 2
        jumps += 1
    kinds["jumps_inside_a_string"] = jumps
    kinds["seams"] = {name: v for name, v in found.items() if "@" in name}
    # the expected answers of every form, from the oracle's per-k-mer results
    pt.want_rows = rows_of(pt.kinds)
    pt.want_totals = pt.want_rows.sum(0)
    rep = case.oracle.streaming_query(reads)
    assert [rep[c] for c in COLUMNS] == pt.want_totals.tolist(), "the oracle's report against its per-k-mer results"
    pt.cover_words = (n_kmers + 63) // 64
    pt.want_cover, pt.want_depth = bitmap_of(all_ids, pt.cover_words), depth_of(all_ids, n_kmers)
    # the long reads: the same references
    lk, lo_, lids = classify(case.oracle, pt.long_reads, k)
    assert (np.concatenate(lids)[np.concatenate(lk) != 0] == truth_ids(case.gt, pt.sequences, pt.long_reads, lk, k)).all(), "the long reads: the oracle's ids against GroundTruth.lookup"
    pt.long_kinds, pt.long_ids = lk, lids
    assert (lk[0] != 0).all() and (lk[1] == 0).sum() >= k and min(int((x >= 2).sum()) for x in lk) > 20000
    # the repeated read: one run
    hk, _, hids = classify(case.oracle, pt.repeated[:1], k)
    assert (hk[0] == np.array([2] + [3] * 100)).all(), "the repeated read is one run of 101 k-mers"
    pt.hot_ids = hids[0]
    # the sums: per read values[ids].sum() and the number of ids, and the same from the run records
    pt.sums_cases = sums_cases(n_kmers, 7000 * k + 10 * pt.m + int(pt.canonical))
    assert 0.4 < (pt.sums_cases[0][1] >= np.uint32(HALF)).mean() < 0.6
    pt.want_sums, (pt.want_offsets, pt.want_runs) = sums_references(pt, pt.sums_cases, reads, pt.ids, case.oracle)
    assert int(pt.want_offsets[-1]) == int(pt.want_totals[4])
    for name, rows in pt.want_sums.items():
        assert (rows["positive_kmers"] == pt.want_rows[:, 1]).all(), f"sums, {name}: positive_kmers against column 1 of the rows"
    no_id_below, no_id_above = neighbours_differ(pt.want_runs, pt.sums_cases[0][1], n_kmers)
    assert no_id_below > 0 and no_id_above > 0, "runs from id 0 and runs to the last id"
    backward_runs = (pt.want_runs["num_kmers"] & np.uint32(BACKWARD)) != 0
    assert backward_runs.any() and not backward_runs.all()
    pt.batch = reads[:20] + [pt.long_reads[0], ""] + reads[20:40] + [pt.long_reads[1]]
    batch_ids = pt.ids[:20] + [pt.long_ids[0], pt.ids[0][:0]] + pt.ids[20:40] + [pt.long_ids[1]]
    pt.want_batch_sums, (pt.batch_offsets, pt.batch_runs) = sums_references(pt, pt.sums_cases, pt.batch, batch_ids, case.oracle)
    pt.want_hot_sums, (hot_offsets, hot_runs) = sums_references(pt, pt.sums_cases[:1], pt.repeated[:1], hids, case.oracle)
    assert hot_runs.size == 1
    # the classes, the best run and the run records over segments: two references each, and what the reads hold for them
    later = later_references(pt, case.oracle, string_of_ids(case.gt, k)[0], batch_ids, hids, (hot_offsets, hot_runs), SEGMENT_SIZES)
    sums = {"positive_kmers": int(pt.want_sums["random"]["positive_kmers"].sum(dtype=np.uint64)), "largest_row_sum": int(pt.want_sums["random"]["sum"].max()),
            "largest_row_sum_of_the_long_reads": int(pt.want_batch_sums["all ones"]["sum"].max()), "runs": int(pt.want_runs.size),
            "runs_without_an_id_below": no_id_below, "runs_without_an_id_above": no_id_above}
    assert sums["positive_kmers"] == int(pt.want_totals[1]) > 0 and sums["largest_row_sum"] > (1 << 32)
    return {"kmers": n_kmers, "sums": sums, "strings": len(pt.sequences), "reads": len(reads), "read_kmers": int(pt.want_totals[0]), "runs": int(pt.want_totals[4]),
            "seams_joined": {str(S): found[f"seam_in_forward_run@{S}"] + found[f"seam_in_backward_run@{S}"] for S in SEGMENT_SIZES}, "kinds": kinds,
            "floors": pt.floors, **later}


# ---- the device --------------------------------------------------------------------------------------------------------------------------
def sums_everything(d, reads, cases, prefixes, device):
    """the sums of `reads` under every case through the host call (device False), or through the device call over the case's prefix,
    once with a report and once with a NULL report -> a dict of arrays, compared word for word (gpu_segments_worker.same)"""
    from gpu_per_read_worker import report_row
    from gpu_sums_worker import device_sums

    out = {}
    for (name, values, at_least), (_, p_prefix) in zip(cases, prefixes):
        if device:
            out[name], out[name + ": report"] = device_sums(d, reads, p_prefix, report=[0] * 6)
            out[name + ": no report"], _ = device_sums(d, reads, p_prefix)
        else:
            rows, rep = d.streaming_sums(reads, values, at_least)
            out[name], out[name + ": report"] = rows, report_row(rep)
    return out


def sums_wanted(want, cases, totals):
    """-> (what sums_everything must give through the host calls, through the device calls)"""
    host, device = {}, {}
    for name, _, _ in cases:
        host[name], host[name + ": report"] = want[name], totals
    for name, _, _ in cases:
        device[name], device[name + ": report"], device[name + ": no report"] = want[name], totals, want[name]
    return host, device


def check_flavour(pt, key_length, layer, upload=None, replica=None, then=None):
    """`upload`: dictionary -> the dictionary on device 0, where that is not a plain to_device(0); `replica`: (stats, what) -> None, what
    device_stats() has to show beyond the layer's own, asserted before the first streaming call; `then`: (d, what) -> None, more calls
    on the same replica behind the sweep's own (tests/gpu_walks_worker.py passes all three; the sweep none)"""
    import sshash_amd
    from gpu_cover_worker import bitmap_of, device_string_counts
    from gpu_depth_worker import depth_of, device_depth, device_string_sums
    from gpu_forms_later import DEFAULT_S, check_long, check_segmented, check_uncut
    from gpu_per_read_worker import oracle_rows
    from gpu_runs_worker import check_both
    from gpu_segments_worker import accumulated, everything, launches, same
    from gpu_sums_worker import device_prefix, device_sums
    from test_gpu_streaming import _as_dict

    case, k, m, reads = pt.case, pt.k, pt.m, pt.reads
    what = f"{layer} k={k} m={m} key={key_length} {'canonical' if pt.canonical else 'regular'}"
    d = case.dict.to_device(0) if upload is None else upload(case.dict)
    st = d.device_stats(0)
    assert LAYERS[layer][1](st), f"{what}: the replica is not the {layer} layer: {st}"
    assert st["sk_key_length"] == (key_length or key_length_of(k, m)), (what, st["sk_key_length"])
    if replica is not None:
        replica(st, what)
    n_kmers = case.gt.num_kmers
    assert d.num_kmers() == n_kmers and d.cover_words() == pt.cover_words
    totals, rows, cover, depth = pt.want_totals, pt.want_rows, pt.want_cover, pt.want_depth
    want_host = {"totals": totals, "rows": rows, "rows_report": totals, "cover": cover, "cover_report": totals, "depth": depth, "depth_report": totals}
    want_device = dict(want_host, rows_no_report=rows, cover_no_report=cover, depth_no_report=depth)
    cases = pt.sums_cases
    sums_host, sums_device = sums_wanted(pt.want_sums, cases, totals)

    # ---- uncut: the first seven forms, host and device (rows into a prefilled array between guard rows) ----
    assert d.read_segments()["kmers"] == sshash_amd.SEGMENTS_OFF, "a new dictionary does not segment"
    d.set_read_segments(sshash_amd.SEGMENTS_OFF, device_calls=True)
    assert _as_dict(d.streaming_query(reads)) == case.oracle.streaming_query(reads), f"{what}: streaming_query"
    assert (oracle_rows(case.oracle, reads) == rows).all()
    same(everything(d, reads, False), want_host, f"{what}: uncut, host calls")
    same(everything(d, reads, True), want_device, f"{what}: uncut, device calls")
    prefixes = [device_prefix(d, values, at_least) for _, values, at_least in cases]  # (against numpy.cumsum in 64 bits, guard words around it; held to the end)
    same(sums_everything(d, reads, cases, prefixes, False), sums_host, f"{what}: sums uncut, host calls")
    same(sums_everything(d, reads, cases, prefixes, True), sums_device, f"{what}: sums uncut, device calls")
    want_offsets, want_runs = pt.want_offsets, pt.want_runs
    check_both(d, reads, want_offsets, want_runs, what)
    per_read, report = d.streaming_lookup(reads, full=True)
    assert _as_dict(report) == case.oracle.streaming_query(reads), f"{what}: streaming_lookup report"
    for r, (got, ids) in enumerate(zip(per_read, pt.ids)):
        assert (got.kmer_id == ids).all(), f"{what}: streaming_lookup, read {r}"
    run_offsets, runs, _ = d.streaming_runs(reads)
    for r, (back, got) in enumerate(zip(sshash_amd.expand_runs(run_offsets, runs, [len(x) for x in reads], k), per_read)):
        hit = got.kmer_id != INVALID
        for f in ("kmer_id", "kmer_id_in_string", "string_id"):
            assert (getattr(back, f) == getattr(got, f)).all(), f"{what}: expand_runs against streaming_lookup, read {r}, {f}"
        assert (back.kmer_orientation[hit] == got.kmer_orientation[hit]).all(), f"{what}: expand_runs orientation, read {r}"
    # ---- cover and depth per string, against numpy over the strings' lengths ----
    string_of, sizes = string_of_ids(case.gt, k)
    held = np.flatnonzero(depth)
    want_counts = np.bincount(string_of[held], minlength=sizes.size).astype(np.uint64)
    want_sums = np.bincount(string_of, weights=depth.astype(np.float64), minlength=sizes.size).astype(np.uint64)
    for counts, total in (d.cover_string_counts(cover), device_string_counts(d, cover)):
        assert (counts == want_counts).all() and total == held.size, f"{what}: cover_string_counts"
    for sums, total in (d.depth_string_sums(depth), device_string_sums(d, depth)):
        assert (sums == want_sums).all() and total == int(depth.sum(dtype=np.uint64)), f"{what}: depth_string_sums"
    # ---- depth: the deltas, finished in place and out of place, arrays at an address that is no multiple of 16 ----
    for in_place in (True, False):
        got, deltas, _ = device_depth(d, reads, in_place=in_place, skew=1)
        assert (got == depth).all(), f"{what}: depth, device call, skew 1, in place {in_place}"
        assert (np.cumsum(deltas, dtype=np.uint32) == depth).all(), f"{what}: the deltas' prefix sum"
        assert (deltas != 0).sum() <= 2 * int(totals[4]), f"{what}: at most two deltas a run"
    want_hot = depth_of(pt.hot_ids, n_kmers) * np.uint32(REPEATS)
    got, deltas, _ = device_depth(d, pt.repeated)
    assert (got == want_hot).all(), f"{what}: one read {REPEATS} times"
    hi = int(pt.hot_ids.max())
    assert sorted(deltas[deltas != 0].tolist()) == ([REPEATS] if hi == n_kmers - 1 else [REPEATS, (1 << 32) - REPEATS]), f"{what}: the deltas of the repeated read"
    got, _ = d.streaming_depth(pt.repeated)
    assert (got == want_hot).all(), f"{what}: one read {REPEATS} times, host call"
    want_hot_rows = np.repeat(pt.want_hot_sums["random"], REPEATS)
    assert int(want_hot_rows["positive_kmers"][0]) == 101 and int(want_hot_rows["sum"][0]) > (1 << 32)
    got, rep = device_sums(d, pt.repeated, prefixes[0][1], report=[0] * 6)
    assert got.tobytes() == want_hot_rows.tobytes() and int(rep[1]) == 101 * REPEATS, f"{what}: sums, one read {REPEATS} times: {REPEATS} equal rows"
    got, _ = d.streaming_sums(pt.repeated, cases[0][1])
    assert got.tobytes() == want_hot_rows.tobytes(), f"{what}: sums, one read {REPEATS} times, host call"

    # ---- reads above 2^16 bases: the host calls (the position-parallel route), the device calls (one lane each) ----
    batch = pt.batch
    bk, bids = pt.kinds[:20] + [pt.long_kinds[0], pt.kinds[0][:0]] + pt.kinds[20:40] + [pt.long_kinds[1]], pt.ids[:20] + pt.long_ids[:1] + pt.ids[20:40] + pt.long_ids[1:]
    brows = rows_of(bk)
    assert (brows == oracle_rows(case.oracle, batch)).all()
    bcover, bdepth = bitmap_of(np.concatenate(bids), pt.cover_words), depth_of(np.concatenate(bids), n_kmers)
    long_host = {"totals": brows.sum(0), "rows": brows, "rows_report": brows.sum(0), "cover": bcover, "cover_report": brows.sum(0), "depth": bdepth,
                 "depth_report": brows.sum(0)}
    long_device = dict(long_host, rows_no_report=brows, cover_no_report=bcover, depth_no_report=bdepth)
    same(everything(d, batch, False), long_host, f"{what}: the long reads uncut, host calls")
    same(everything(d, batch, True), long_device, f"{what}: the long reads uncut, device calls")
    long_sums_host, long_sums_device = sums_wanted(pt.want_batch_sums, cases, brows.sum(0))
    same(sums_everything(d, batch, cases, prefixes, False), long_sums_host, f"{what}: sums, the long reads uncut, host calls (the per-k-mer route)")
    same(sums_everything(d, batch, cases, prefixes, True), long_sums_device, f"{what}: sums, the long reads uncut, device calls (one lane each)")
    # ---- the classes, the best run, and the run records of the long reads: uncut ----
    check_uncut(d, pt, totals, brows.sum(0), f"{what}: uncut", REPEATS)
    assert launches(d) == 0, "SEGMENTS_OFF launched over segments"

    # ---- segments of S k-mers: byte for byte the uncut answers, also into arrays that hold values ----
    rng = np.random.default_rng(5)
    before_cover = rng.integers(0, 1 << 63, pt.cover_words, dtype=np.uint64) & rng.integers(0, 1 << 63, pt.cover_words, dtype=np.uint64)
    before_cover[-1] &= np.uint64((1 << (n_kmers % 64 or 64)) - 1)
    before_depth = rng.integers(0, 1 << 32, n_kmers, dtype=np.uint64).astype(np.uint32)
    start = np.arange(1, 7, dtype=np.uint64) * np.uint64(1000003)
    acc_host = {"cover": cover | before_cover, "depth": depth + before_depth}
    acc_device = dict(cover=acc_host["cover"], depth=depth + np.cumsum(before_depth, dtype=np.uint32), totals=totals + start, rows_report=totals + start,
                      cover_report=totals + start, depth_report=totals + start)  # (the device call adds to DELTAS: what they held is scanned with them)
    segmented, of_runs, of_classes = {}, {}, {}
    for S in SEGMENT_SIZES:
        d.set_read_segments(S, device_calls=True)
        assert d.read_segments()["kmers"] == S
        at = launches(d)
        same(everything(d, reads, False), want_host, f"{what}: S = {S}, host calls")
        assert launches(d) >= at + 4, f"{what}: S = {S}: the host calls did not launch over segments"
        at = launches(d)
        same(everything(d, reads, True), want_device, f"{what}: S = {S}, device calls")
        assert launches(d) > at, f"{what}: S = {S}: the device calls did not launch over segments"
        same(accumulated(d, reads, False, before_cover, before_depth), acc_host, f"{what}: S = {S}, host calls into arrays that hold values")
        same(accumulated(d, reads, True, before_cover, before_depth), acc_device, f"{what}: S = {S}, device calls into arrays that hold values")
        at = launches(d)
        same(sums_everything(d, reads, cases, prefixes, False), sums_host, f"{what}: sums, S = {S}, host calls")
        assert launches(d) >= at + len(cases), f"{what}: S = {S}: the host calls of the sums did not launch over segments"
        at = launches(d)
        same(sums_everything(d, reads, cases, prefixes, True), sums_device, f"{what}: sums, S = {S}, device calls")
        assert launches(d) == at + 2 * len(cases), f"{what}: S = {S}: every device call of the sums launches over segments once"
        of_runs[str(S)], of_classes[str(S)] = check_segmented(d, pt, S, totals, what)
        segmented[str(S)] = launches(d)
    # ---- the long reads at the default S ----
    d.set_read_segments(device_calls=True)
    S = d.read_segments()["kmers"]
    assert 1 < S < (1 << 14), S
    assert S == DEFAULT_S, "the gate counted the runs over three segments of the long reads at another S"
    at = launches(d)
    same(everything(d, batch, False), long_host, f"{what}: the long reads at the default S, host calls")
    same(everything(d, batch, True), long_device, f"{what}: the long reads at the default S, device calls")
    assert launches(d) > at
    at = launches(d)
    same(sums_everything(d, batch, cases, prefixes, False), long_sums_host, f"{what}: sums, the long reads at the default S, host calls")
    assert launches(d) >= at + len(cases)
    at = launches(d)
    same(sums_everything(d, batch, cases, prefixes, True), long_sums_device, f"{what}: sums, the long reads at the default S, device calls")
    assert launches(d) == at + 2 * len(cases)
    check_long(d, pt, brows.sum(0), f"{what}: the long reads at the default S")
    # ---- and off again ----
    d.set_read_segments(sshash_amd.SEGMENTS_OFF, device_calls=True)
    at = launches(d)
    same(everything(d, reads, False), want_host, f"{what}: SEGMENTS_OFF again, host calls")
    same(everything(d, reads, True), want_device, f"{what}: SEGMENTS_OFF again, device calls")
    same(sums_everything(d, reads, cases, prefixes, False), sums_host, f"{what}: sums, SEGMENTS_OFF again, host calls")
    same(sums_everything(d, reads, cases, prefixes, True), sums_device, f"{what}: sums, SEGMENTS_OFF again, device calls")
    check_uncut(d, pt, totals, brows.sum(0), f"{what}: SEGMENTS_OFF again", REPEATS, first=False)
    assert launches(d) == at, "SEGMENTS_OFF launched over segments"
    del prefixes
    if then is not None:
        then(d, what)
    d.close()
    return {"sk_slots": st["sk_slots"], "directory_sectors": st["directory_sectors"], "sk_key_length": st["sk_key_length"], "sk_heavy_kmers": st["sk_heavy_kmers"],
            "default_S": S, "segmented_launches": segmented, "segmented_launches_of_run_records": of_runs, "segmented_launches_of_classes": of_classes}


def main():
    import tempfile

    k, m, key_length, layer, exe, scratch = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), sys.argv[4], sys.argv[5], sys.argv[6]
    cpu_only = "--cpu-only" in sys.argv[7:]
    assert layer in LAYERS
    out, seconds = {}, {}
    with tempfile.TemporaryDirectory(dir=scratch) as tmp:
        for canonical in (False, True):
            name = "canonical" if canonical else "regular"
            t0 = time.time()
            pt = make_inputs(k, m, key_length, canonical, exe, tmp)
            out[name] = gate(pt)
            t1 = time.time()
            if not cpu_only:
                out[name].update(check_flavour(pt, key_length, layer))
                if layer == "table" and (k, m, key_length) in HEAVY:
                    assert out[name]["sk_heavy_kmers"] > 0, (k, m, key_length, name, "no k-mer under a heavy key")
            seconds[name] = [round(t1 - t0, 2), round(time.time() - t1, 2)]  # (inputs and references on the CPU, calls on the device)
    print(json.dumps({"ok": True, "k": k, "m": m, "key_length": key_length, "layer": layer, "cpu_only": cpu_only, "dictionaries": out, "seconds": seconds}))


if __name__ == "__main__":
    main()
