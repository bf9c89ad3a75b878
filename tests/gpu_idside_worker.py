#!/usr/bin/env python
"""Worker of tests/test_gpu_idside.py, and the input generator it shares with tests/test_idside_inputs.py: the id -> k-mer side of the
library -- iterate_kernel, access_kernel, weight_kernel, expand_neighbours_kernel, revcomp_kernel and check_compare_kernel behind
sshash_check_device, and the host's string_neighbours -- at one k, m = min(k, 13), regular then canonical.

The fixtures of the suite hold dozens to thousands of k-mers per string and under 5 M k-mers per dictionary, so on an MI355X a block of
iterate_kernel never owned a second tile (the hand-over of the string index `s0`), a tile never staged more than its first 256 string
starts (the second to ninth round of the staging loop, last_leq over more than 256 entries, the entries past num_strings), and
sshash_check_device never took a second round. The dictionary of make_dense() is dense in strings -- stretches of thousands of strings
that hold ONE k-mer each, as a unitig set has them -- and the two hooks iterate_blocks and check_chunk (csrc/hooks.hpp) bring the tiles
per block and the rounds of the check down to its size. plan() lists the (begin, end, iterate_blocks) launches, describe() restates the
tile arithmetic of each (and nothing else of the kernel), summary() counts what the launches reach; tests/test_idside_inputs.py asserts
on the CPU that each of the gaps is reached at every k.

All comparisons are exact, against the input strings (GroundTruth, input order) and the CPU oracle. Prints one JSON line; any mismatch is
an assertion error.

    python tests/gpu_idside_worker.py <k> <scratch dir> [--cpu-only]"""
from __future__ import annotations

import json
import os
import sys
import time
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import numpy as np

KS = (15, 17, 31, 33, 35, 47, 61, 63)  # one word: small, 17, full; two words: one base in the second word, 35, 47, 61, full
INVALID = 0xFFFFFFFFFFFFFFFF
TILE, ROUND, STAGE = 2048, 256, 2304  # IT_TILE, IT_BLOCK, IT_STAGE of csrc/engine.hip
DEFAULT_BLOCKS = 256 * 32  # CUs x IT_BLOCKS_PER_CU of an MI355X: what iterate_blocks replaces (no launch of the plan has that many tiles)
BLOCKS = (None, 1, 2, 3, 7)  # iterate_blocks: unset, then values that make a block own all, half, a third and a seventh of the tiles
LENGTHS = (TILE - 1, TILE, TILE + 1, 3 * TILE + 5)
SHIFTS = (-1, 0, 1, TILE - 1, TILE)
SINGLES, PAIRS, RAGGED, SINGLES_AT_THE_END = 3 * TILE + 300, 1500, 200, 2100
CHECK_CHUNKS = (None, TILE, 3 * TILE + 5, -1)  # check_chunk: unset, ..., and (-1) num_kmers - 1
FIELDS = ("kmers", "forward_not_found", "forward_other_id", "reverse_complement_wrong", "not_member", "first_failure")
DUP_CHUNK = 4096


def m_of(k):
    return min(k, 13)


# ---- the dictionary's strings ------------------------------------------------------------------------------------------------------------
def make_dense(k, seed):
    """random DNA whose canonical k-mers are distinct over the whole collection (at k = 15 random strings collide), in order: one string
    of k + 700 bases, 3 x 2048 + 300 strings of one k-mer, one string of k + 1000 bases, 1500 strings of two k-mers, 200 strings of
    ragged length in [k, 6k), and 2100 strings of one k-mer: the dictionary ends inside a single-k-mer stretch"""
    from conftest import random_dna
    from gpu_forms_worker import _adder

    rng = np.random.default_rng(seed)
    seqs = []
    add = _adder(seqs, k)
    lengths = [k + 700] + [k] * SINGLES + [k + 1000] + [k + 1] * PAIRS + [int(x) for x in rng.integers(k, 6 * k, RAGGED)] + [k] * SINGLES_AT_THE_END
    for n in lengths:
        while not add(random_dna(rng, n)):
            pass
    return seqs


def first_ids_of(sequences, k):
    """first k-mer id of every string, and num_kmers behind them"""
    return np.concatenate([[0], np.cumsum([len(s) - k + 1 for s in sequences])]).astype(np.int64)


def stretches(first):
    """-> ((first id, end) of the single-k-mer stretch behind string 0, of the one the dictionary ends in)"""
    sizes = np.diff(first)
    assert sizes[0] > 1 and (sizes[1:1 + SINGLES] == 1).all() and sizes[1 + SINGLES] > 1 and (sizes[-SINGLES_AT_THE_END:] == 1).all()
    n = int(first[-1])
    return (int(first[1]), int(first[1 + SINGLES])), (n - SINGLES_AT_THE_END, n)


# ---- the launches ------------------------------------------------------------------------------------------------------------------------
def plan(first_ids, k):
    """-> [(begin, end, iterate_blocks or None)]: the whole range and test_iterate.sub_ranges; ranges that begin at the first id of a
    single-k-mer stretch moved by -1, 0, +1, +2047 and +2048; ranges of 2047, 2048, 2049 and 3 x 2048 + 5 ids; ranges that end at
    num_kmers -- each under every value of BLOCKS. sub_ranges gives two ranges of at most 5 ids for EVERY single-k-mer string, 17 000
    launches of one tile and one block whatever the hook says: of those, the ones at the edges of the stretches and of the tiles counted
    from id 0, and every 16th of the rest, run once, with the hook unset."""
    from test_iterate import sub_ranges

    first = np.asarray(first_ids, dtype=np.int64)
    n = int(first[-1])
    (a1, e1), (a2, _) = stretches(first)
    named = {(0, n)}
    for start in (a1, a2):
        for shift in SHIFTS:
            b = start + shift
            named |= {(b, min(n, b + L)) for L in LENGTHS} | {(b, n)}
    for L in LENGTHS:
        named |= {(n - L, n), (0, L), (e1 - L, e1), (e1 - L + 1, e1 + 1)}
    named |= {(e1 - 100 - ROUND * j, e1 + 5) for j in range(8)}  # one tile of 102 + 256 j entries: every number of rounds of the staging loop
    # (sub_ranges reads the strings' lengths only)
    ranges = sub_ranges(SimpleNamespace(k=k, sequences=[range(int(size) + k - 1) for size in np.diff(first)]), seed=k, n_random=60)
    assert all(0 <= b <= e <= n for b, e in named | set(ranges))
    short = sorted({r for r in ranges if r[1] - r[0] <= 5} - named)
    rest = sorted((set(ranges) - set(short)) | named)
    edges = np.array([0, a1, e1, a2, n])
    kept = [r for i, r in enumerate(short) if i % 16 == 0 or np.abs(edges - r[0]).min() <= 3 or (r[0] + 3) % TILE <= 6]
    out = [(b, e, blocks) for blocks in BLOCKS for b, e in rest]
    out += [(b, e, None) for b, e in kept]
    return out


def describe(triples, first_ids, default_blocks=DEFAULT_BLOCKS):
    """the tile arithmetic of iterate_packed_device restated, per launch: tiles are counted from `begin`, a block takes
    ceil(tiles / blocks) consecutive tiles. Per tile: `needs`, the strings it touches as IT_STAGE counts them -- the strings that hold
    one of its ids and the next one, whose first id closes the stage: 2049 for 2048 strings of one k-mer --, the entries it stages
    (rounds of 256 until `needs` are there) and whether the last of them lies past entry num_strings. An empty range launches nothing."""
    first = np.asarray(first_ids, dtype=np.int64)
    num_strings = first.size - 1
    out = []
    for b, e, blocks in triples:
        if b == e:
            continue
        tiles = -(-(e - b) // TILE)
        allowed = blocks or default_blocks
        tiles_per_block = -(-tiles // allowed)
        lo = b + TILE * np.arange(tiles, dtype=np.int64)
        hi = np.minimum(e, lo + TILE)
        string_lo = np.searchsorted(first, lo, "right") - 1  # the string of the tile's first id
        closing = np.searchsorted(first, hi, "left")  # the first string whose first id is >= hi (entry num_strings holds num_kmers)
        needs = closing - string_lo + 1
        staged = ROUND * -(-needs // ROUND)
        assert (needs <= TILE + 1).all() and (staged <= STAGE).all() and (closing <= num_strings).all()
        out.append(dict(begin=b, end=e, blocks=blocks, allowed=allowed, tiles=tiles, tiles_per_block=tiles_per_block, grid=-(-tiles // tiles_per_block),
                        string_lo=string_lo, closing=closing, needs=needs, staged=staged, past_the_strings=string_lo + staged - 1 > num_strings))
    return out


def summary(launches):
    """what the launches reach -> counts (tests/test_idside_inputs.py asserts each positive)"""
    c = dict(launches=len(launches), tiles=0, most_tiles_per_block=0, tiles_of_2049_strings=0, tiles_of_257_to_2048_strings=0, tiles_staging_past_the_strings=0,
             blocks_of_3_tiles_and_more_than_one_stage=0, blocks_ending_in_a_partial_tile=0, launches_with_fewer_blocks_than_allowed=0)
    for d in launches:
        tpb = d["tiles_per_block"]
        c["tiles"] += d["tiles"]
        c["most_tiles_per_block"] = max(c["most_tiles_per_block"], min(tpb, d["tiles"]))
        c["tiles_of_2049_strings"] += int((d["needs"] == TILE + 1).sum())
        c["tiles_of_257_to_2048_strings"] += int(((d["needs"] > ROUND) & (d["needs"] <= TILE)).sum())
        c["tiles_staging_past_the_strings"] += int(d["past_the_strings"].sum())
        for t0 in range(0, d["tiles"], tpb):
            t1 = min(d["tiles"], t0 + tpb)
            # a block whose string index stayed at its first tile's would stage IT_STAGE entries from there: short of its last tile
            c["blocks_of_3_tiles_and_more_than_one_stage"] += int(t1 - t0 >= 3 and d["closing"][t1 - 1] - d["string_lo"][t0] + 1 > STAGE)
        last = d["tiles"] - (d["grid"] - 1) * tpb  # tiles of the last block
        c["blocks_ending_in_a_partial_tile"] += int(last >= 2 and (d["end"] - d["begin"]) % TILE != 0)
        c["launches_with_fewer_blocks_than_allowed"] += int(d["blocks"] is not None and d["grid"] < d["blocks"])
    return c


def check_rounds(n, chunk):
    """sizes of the rounds of sshash_check_device under check_chunk = chunk"""
    chunk = min(n, chunk)
    return [min(chunk, n - b) for b in range(0, n, chunk)]


def chunk_of(n, setting):
    return n - 1 if setting == -1 else setting


# ---- the inputs of the other calls -------------------------------------------------------------------------------------------------------
def make_dup(k, seed):
    """tests/test_gpu_iterate.py::test_check_counts_failures_as_the_oracle_predicts at this k, for a check in rounds of 4096: one short
    string twice among random ones, the first copy behind 5000 k-mers -- not in the first round --, the second 13000 k-mers (more than
    three rounds) further on -> (strings, index of the first copy, of the second)"""
    from conftest import random_dna
    from gpu_forms_worker import _adder

    rng = np.random.default_rng(seed)
    seqs = []
    add = _adder(seqs, k)

    def fresh(n):
        while not add(random_dna(rng, n)):
            pass

    for _ in range(10):
        fresh(k + 499)
    fresh(k + 6)
    at_a = len(seqs) - 1
    for _ in range(26):
        fresh(k + 499)
    at_b = len(seqs)
    seqs.append(seqs[at_a])
    for n in rng.integers(k, 4 * k, 20):
        fresh(int(n))
    return seqs, at_a, at_b


def weight_depths(first):
    """-> {name: depth per id}. "constant": ONE interval. "edges": a new interval at every id of the single-k-mer stretches (1, 2, 1,
    ...); every other string holds 9 but for its last id, 10 -- a run that starts exactly at a string's last id and, behind it, one that
    starts exactly at the next string's first; a stretch of 7 over whole strings that starts and ends inside one; values above 2^16
    and, at the last id but one, 2^32 - 1."""
    first = np.asarray(first, dtype=np.int64)
    n, sizes = int(first[-1]), np.diff(first)
    ids = np.arange(n, dtype=np.int64)
    string_of = np.repeat(np.arange(sizes.size), sizes)
    single = sizes[string_of] == 1
    depth = np.full(n, 9, dtype=np.uint32)
    depth[(ids == first[string_of + 1] - 1) & ~single] = 10
    depth[single] = (1 + (ids[single] & 1)).astype(np.uint32)
    r0 = 1 + SINGLES + 1 + PAIRS  # the first ragged string
    big = [s for s in range(r0, r0 + RAGGED) if sizes[s] >= 4]
    depth[first[big[2]] + 1:first[big[40]] + 2] = 7
    depth[first[big[50]] + 1] = 70000
    depth[first[big[60]]] = 1 << 31
    depth[n - 2] = 0xFFFFFFFF
    (a1, e1), (a2, _) = stretches(first)
    for a, e in ((a1, e1), (a2, n - 2)):
        assert (depth[a + 1:e] != depth[a:e - 1]).all(), "a new interval at every id of a single-k-mer stretch"
    starts = np.flatnonzero(np.concatenate([[True], depth[1:] != depth[:-1]]))  # the first ids of the intervals
    at_first, at_last = np.isin(starts, first[:-1]), np.isin(starts, first[1:] - 1)
    assert (at_first & ~single[starts]).sum() > 1000 and (at_last & ~single[starts]).sum() > 1000 and (~at_first & ~at_last).sum() >= 2
    return {"constant": np.full(n, 5, dtype=np.uint32), "edges": depth}


def neighbour_queries(case, seed):
    """2000 k-mers of the dictionary, every other one reverse-complemented, and 500 random ones, shuffled"""
    return case.queries(2000, 500, seed=seed)


def string_picks(first, seed):
    """400 strings: string 0, the last, both ends of the single-k-mer stretches, the long strings, and random ones of every part"""
    num_strings = first.size - 1
    rng = np.random.default_rng(seed)
    fixed = [0, num_strings - 1, 1, 2, SINGLES, 1 + SINGLES, 2 + SINGLES, num_strings - SINGLES_AT_THE_END - 1, num_strings - SINGLES_AT_THE_END]
    parts = [rng.integers(1, 1 + SINGLES, 130), rng.integers(2 + SINGLES, 2 + SINGLES + PAIRS, 90), rng.integers(2 + SINGLES + PAIRS, 2 + SINGLES + PAIRS + RAGGED, 130),
             rng.integers(num_strings - SINGLES_AT_THE_END, num_strings, 90)]
    more = [int(s) for s in np.concatenate(parts) if int(s) not in fixed]
    picks = np.array(fixed + more[:400 - len(fixed)], dtype=np.uint64)
    assert picks.size == 400 and (np.diff(first)[picks.astype(np.int64)] == 1).sum() >= 150
    return picks


class Inputs:
    """one dictionary of make_dense with what the references say about it (on the CPU)"""


def make_inputs(k, canonical, scratch, sequences=None):
    from conftest import Case

    pt = Inputs()
    pt.k, pt.m, pt.canonical, pt.W = k, m_of(k), canonical, 1 if k <= 31 else 2
    pt.sequences = sequences if sequences is not None else make_dense(k, 4000 + k)
    pt.case = Case(f"idside_k{k}_{int(canonical)}", pt.sequences, k, pt.m, canonical, scratch)
    pt.first = first_ids_of(pt.sequences, k)
    pt.n = int(pt.first[-1])
    pt.plan = plan(pt.first, k)
    return pt


def gate(pt):
    """on the CPU, before any device call: the host iterator, the host access and the oracle agree with the input strings on every id"""
    case, n = pt.case, pt.n
    ids = np.arange(n, dtype=np.uint64)
    pt.all_kmers = want = case.gt.kmers(ids)
    assert case.dict.num_kmers() == n == case.gt.num_kmers and case.dict.num_strings() == len(pt.sequences)
    assert np.array_equal(case.dict.kmers(), want), "Dictionary.kmers() against the input strings"
    assert np.array_equal(case.dict.access_packed(ids), want), "Dictionary.access_packed() against the input strings"
    assert np.array_equal(case.oracle.lookup_ids(want), ids), "the oracle's id of k-mer i is i"
    return summary(describe(pt.plan, pt.first))


# ---- the device --------------------------------------------------------------------------------------------------------------------------
class hooks:
    """SSHASH_AMD_TEST_HOOKS for the calls inside the block (read once per C-ABI call)"""

    def __init__(self, text):
        self.text = text

    def __enter__(self):
        if self.text:
            os.environ["SSHASH_AMD_TEST_HOOKS"] = self.text
        else:
            os.environ.pop("SSHASH_AMD_TEST_HOOKS", None)

    def __exit__(self, *exc):
        os.environ.pop("SSHASH_AMD_TEST_HOOKS", None)


def check_iterate(pt, d, what):
    from test_gpu_iterate import iterate_on_device

    want = pt.all_kmers.reshape(-1, pt.W)
    for blocks in BLOCKS:
        with hooks(f"iterate_blocks={blocks}" if blocks else None):
            for b, e, _ in (t for t in pt.plan if t[2] == blocks):
                got, margins = iterate_on_device(d, b, e, pt.W)
                assert margins, f"{what}: kmers_device({b}, {e}), iterate_blocks={blocks}: wrote outside its range"
                if not np.array_equal(got, want[b:e].reshape(-1)):
                    bad = np.flatnonzero((got.reshape(-1, pt.W) != want[b:e]).any(1))
                    raise AssertionError(f"{what}: kmers_device({b}, {e}), iterate_blocks={blocks}: {bad.size} k-mers differ from the input strings, the first at id {b + int(bad[0])}")


def check_access(pt, d, what):
    import torch

    rng = np.random.default_rng(pt.k)
    n = pt.n
    ids = np.concatenate([rng.permutation(n).astype(np.uint64), np.array([n, n + 1, 1 << 63, INVALID], dtype=np.uint64)])
    order = rng.permutation(ids.size)  # (the ids past the end anywhere in the batch)
    ids = ids[order]
    d_ids = torch.from_numpy(ids.view(np.int64)).cuda()
    out = torch.full((ids.size * pt.W + 2 * TILE,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
    d.access_packed_device(0, d_ids.data_ptr(), ids.size, out.data_ptr() + TILE * 8, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    host = out.cpu().numpy().view(np.uint64)
    assert (host[:TILE] == 0x5A5A5A5A5A5A5A5A).all() and (host[-TILE:] == 0x5A5A5A5A5A5A5A5A).all(), f"{what}: access_packed_device wrote outside its output"
    got = host[TILE:-TILE].reshape(-1, pt.W)
    inside = ids < np.uint64(n)
    assert (~inside).sum() == 4 and (got[~inside] == np.uint64(INVALID)).all(), f"{what}: access_packed_device of ids past the end"
    assert np.array_equal(got[inside], pt.all_kmers.reshape(-1, pt.W)[ids[inside].astype(np.int64)]), f"{what}: access_packed_device against the input strings"


def check_check(pt, d, what):
    clean = dict(zip(FIELDS, (pt.n, 0, 0, 0, 0, INVALID)))
    for setting in CHECK_CHUNKS:
        chunk = chunk_of(pt.n, setting)
        with hooks(f"check_chunk={chunk}" if chunk else None):
            got = d.check(0)
        assert got == clean, f"{what}: check(0) under check_chunk={chunk}: {got}"


def dup_expectations(case, at_a, at_b):
    """the oracle's picture of the dictionary with one string twice (test_check_counts_failures_as_the_oracle_predicts) -> what check()
    must count; the library's own lookups, by the same rules, give the smallest failing id"""
    from gpu_routing_worker import revcomp as packed_revcomp

    k, seqs = case.k, case.sequences
    n = case.gt.num_kmers
    ids = np.arange(n, dtype=np.uint64)
    fwd_q = case.gt.kmers(ids)
    rc_q = packed_revcomp(fwd_q, k, case.W)  # (numpy: GroundTruth turns a two-word k-mer base by base)
    first = first_ids_of(seqs, k)
    size = len(seqs[at_a]) - k + 1
    copy_a, copy_b = np.arange(first[at_a], first[at_a] + size), np.arange(first[at_b], first[at_b] + size)
    assert copy_a[0] >= DUP_CHUNK and copy_b[0] - copy_a[-1] >= 3 * DUP_CHUNK, "both copies behind the first round, more than three rounds apart"
    in_copies = np.zeros(n, dtype=bool)
    in_copies[copy_a] = in_copies[copy_b] = True

    def failures(fwd, rc):
        not_found = fwd == np.uint64(INVALID)
        return not_found, ~not_found & (fwd != ids), rc != ids

    def picture(not_found, other, rc_wrong, whose):
        assert not not_found.any() and not (other | rc_wrong)[~in_copies].any(), f"{whose}: failures only inside the copies"
        assert (other[copy_a] ^ other[copy_b]).all() and (rc_wrong[copy_a] ^ rc_wrong[copy_b]).all(), f"{whose}: one of the two ids of every k-mer"

    o_nf, o_other, o_rc = failures(case.oracle.lookup_packed(fwd_q, True)["kmer_id"], case.oracle.lookup_packed(rc_q, True)["kmer_id"])
    picture(o_nf, o_other, o_rc, "the oracle")
    want = (n, 0, int(o_other.sum()), int(o_rc.sum()), 0)
    assert size > 0 and want[2] == want[3] == size
    return SimpleNamespace(ids=ids, fwd_q=fwd_q, rc_q=rc_q, want=want, failures=failures, picture=picture, copies=set(copy_a.tolist()) | set(copy_b.tolist()))


def check_dup(dup, exp, what):
    d = dup.dict.to_device(0)
    l_nf, l_other, l_rc = exp.failures(d.lookup(exp.fwd_q).kmer_id, d.lookup(exp.rc_q).kmer_id)
    exp.picture(l_nf, l_other, l_rc, "the library's lookups")
    smallest = int(exp.ids[l_other | l_rc].min())
    assert smallest >= DUP_CHUNK, "the smallest failing id lies in a round other than the first"
    for chunk in (DUP_CHUNK, None):
        with hooks(f"check_chunk={chunk}" if chunk else None):
            got = d.check(0)
        assert tuple(got[f] for f in FIELDS[:5]) == exp.want, f"{what}: check(0) of one string twice, check_chunk={chunk}: {got}"
        assert got["first_failure"] in exp.copies and got["first_failure"] == smallest, f"{what}: first_failure, check_chunk={chunk}: {got}, {smallest}"
    d.close()


def check_neighbours(pt, d, what):
    import torch

    from test_gpu_parity import U64_FIELDS, _expand_neighbours

    case = pt.case
    q = neighbour_queries(case, 700 + pt.k)
    expanded = _expand_neighbours(q, pt.k, pt.W)
    want = case.oracle.lookup_packed(expanded)
    got = d.neighbours(q, full=True)
    for f in U64_FIELDS:
        assert (getattr(got, f) == want[f]).all(), f"{what}: neighbours, {f}"
    assert (got.kmer_orientation.astype(np.int64) == want["kmer_orientation"]).all(), f"{what}: neighbours, kmer_orientation"
    assert (got.minimizer_found.astype(np.int64) == want["minimizer_found"]).all(), f"{what}: neighbours, minimizer_found"
    assert (d.neighbours(q, check_reverse_complement=False).kmer_id == case.oracle.lookup_packed(expanded, False)["kmer_id"]).all(), f"{what}: neighbours, one strand"
    found = int((want["kmer_id"] != np.uint64(INVALID)).sum())
    assert found > 1000, "k-mers from inside a string have neighbours in the dictionary"
    n = q.size // pt.W
    dq = torch.from_numpy(q.view(np.int64)).cuda()
    out = torch.full((8 * n + 2 * TILE,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
    d.neighbours_device(0, dq.data_ptr(), n, out.data_ptr() + TILE * 8, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    host = out.cpu().numpy().view(np.uint64)
    assert (host[:TILE] == 0x5A5A5A5A5A5A5A5A).all() and (host[-TILE:] == 0x5A5A5A5A5A5A5A5A).all(), f"{what}: neighbours_device wrote outside its output"
    assert (host[TILE:-TILE] == want["kmer_id"]).all(), f"{what}: neighbours_device"
    return found


def check_string_neighbours(pt, d, what):
    from test_gpu_parity import _expand_neighbours

    import sshash_amd

    case, k, W, first = pt.case, pt.k, pt.W, pt.first
    sids = string_picks(first, 900 + k)
    got = d.string_neighbours(sids).reshape(-1, 8)
    at = sids.astype(np.int64)
    first_ids, last_ids = first[at], first[at + 1] - 1
    want_f = case.oracle.lookup_packed(_expand_neighbours(case.gt.kmers(last_ids), k, W))["kmer_id"].reshape(-1, 8)
    want_b = case.oracle.lookup_packed(_expand_neighbours(case.gt.kmers(first_ids), k, W))["kmer_id"].reshape(-1, 8)
    assert (got[:, :4] == want_f[:, :4]).all() and (got[:, 4:] == want_b[:, 4:]).all(), f"{what}: string_neighbours"
    try:
        d.string_neighbours([len(pt.sequences)])
    except sshash_amd.SSHashError:
        pass
    else:
        raise AssertionError(f"{what}: string_neighbours of a string past the last")


def build_weighted(pt, depth, path):
    import sshash_amd

    sshash_amd.write_weighted_fasta(pt.case.dict, depth, path)
    w = sshash_amd.Dictionary.build(path, k=pt.k, m=pt.m, canonical=pt.canonical, weighted=True, num_threads=4)
    assert w.weighted() and w.num_kmers() == pt.n and w.num_strings() == len(pt.sequences)
    assert (w.weight(np.arange(pt.n, dtype=np.uint64)) == depth.astype(np.uint64)).all(), "the host's weights against the depths"
    assert np.array_equal(w.kmers(), pt.all_kmers), "the weighted dictionary numbers its k-mers as the first"
    return w


def check_weights(pt, weighted, what):
    import torch

    n = pt.n
    for name, (w, depth) in weighted.items():
        w.to_device(0)
        ids = torch.arange(n + 3, dtype=torch.int64, device="cuda")  # three ids past the end
        out = torch.full((n + 3 + 2 * TILE,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
        w.weight_device(0, ids.data_ptr(), n + 3, out.data_ptr() + TILE * 8, stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        host = out.cpu().numpy().view(np.uint64)
        assert (host[:TILE] == 0x5A5A5A5A5A5A5A5A).all() and (host[-TILE:] == 0x5A5A5A5A5A5A5A5A).all(), f"{what}: weight_device wrote outside its output"
        got = host[TILE:-TILE]
        assert (got[:n] == depth.astype(np.uint64)).all(), f"{what}: weight_device, {name}"
        assert (got[n:] == np.uint64(INVALID)).all(), f"{what}: weight_device, {name}: ids past the end"
        w.close()


def check_flavour(pt, dup, dup_exp, weighted):
    what = f"k={pt.k} m={pt.m} {'canonical' if pt.canonical else 'regular'}"
    d = pt.case.dict.to_device(0)
    check_iterate(pt, d, what)
    check_access(pt, d, what)
    check_check(pt, d, what)
    found = check_neighbours(pt, d, what)
    check_string_neighbours(pt, d, what)
    d.close()
    check_dup(dup, dup_exp, what)
    if weighted:
        check_weights(pt, weighted, what)
    return {"neighbours_found": found}


def main():
    import tempfile

    from conftest import Case

    k, scratch = int(sys.argv[1]), sys.argv[2]
    cpu_only = "--cpu-only" in sys.argv[3:]
    assert k in KS
    out, seconds = {}, {}
    os.environ.pop("SSHASH_AMD_TEST_HOOKS", None)
    with tempfile.TemporaryDirectory(dir=scratch) as tmp:
        sequences = make_dense(k, 4000 + k)  # the same strings for both flavours
        dup_strings, at_a, at_b = make_dup(k, 5000 + k)
        for canonical in (False, True):
            name = "canonical" if canonical else "regular"
            t0 = time.time()
            pt = make_inputs(k, canonical, tmp, sequences)
            out[name] = gate(pt)
            out[name].update(kmers=pt.n, strings=len(sequences), check_rounds={str(chunk_of(pt.n, s)): len(check_rounds(pt.n, chunk_of(pt.n, s))) for s in CHECK_CHUNKS[1:]})
            dup = Case(f"idside_dup_k{k}_{int(canonical)}", dup_strings, k, pt.m, canonical, tmp)
            dup_exp = dup_expectations(dup, at_a, at_b)
            weighted = {}
            if not canonical:  # (the weights know nothing of the flavour)
                for kind, depth in weight_depths(pt.first).items():
                    weighted[kind] = (build_weighted(pt, depth, os.path.join(tmp, f"weighted_{kind}.fa")), depth)
            t1 = time.time()
            if not cpu_only:
                out[name].update(check_flavour(pt, dup, dup_exp, weighted))
            seconds[name] = [round(t1 - t0, 2), round(time.time() - t1, 2)]  # (inputs and references on the CPU, calls on the device)
    print(json.dumps({"ok": True, "k": k, "m": m_of(k), "cpu_only": cpu_only, "dictionaries": out, "seconds": seconds}))


if __name__ == "__main__":
    main()
