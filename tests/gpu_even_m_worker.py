#!/usr/bin/env python
"""Worker of tests/test_gpu_even_m.py, and the input generator it shares with tests/test_even_m_inputs.py: dictionaries with an EVEN
minimizer length. Only an even-length m-mer can equal its own reverse complement; such an m-mer reads the same on both strands, which is
the condition of the library's "tie" branches -- a canonical dictionary whose two strands elect the same minimizer value (both
alignments are tried, `minimizer_found` of a miss is the second probe's), and a k-mer whose strands elect equal table-key hashes (no
table key: the complete path; routed by the first word of its smaller strand). With an odd m those branches fire by hash coincidence
alone, a handful of times per fixture or never.

The generator (make_sequences) builds, for a point (k, m): random strings of ragged lengths, plus self-complementary m-mers
P = h + revcomp(h) planted in the middle of strings, as the first and as the last m bases of a string, and twice inside one window.
The P's kept are, of CANDIDATES drawn, those whose trial plantings produce the most ties -- measured with tests/cpp/table_keys.cpp (the
host's build of sk_key) and with gpu_routing_worker.minimizers applied to both strands --, never assumed. Every string is added only if
its canonical k-mers are pairwise distinct and new (the two k-mers that hold a P of k - 1 bases are reverse complements of each other
whenever their flanks are complements: one canonical k-mer twice, which no dictionary may hold). Which k-mers of the result tie, and
which substituted copies of them still tie and are absent, is again measured (make_point), and FLOOR of each kind is asserted.

One worker process = one replica layer (read from the environment when a replica is uploaded) x one point, regular and canonical:
every k-mer on both strands and random negatives through every host and device form; batches of ties only at the sizes around a wave
and a workgroup and one that fills the deferred queue; the routing calls on ties; the streaming calls over reads that walk through P.
Everything against the CPU oracle, and against the input where the input decides the answer. Prints one JSON line; any mismatch is an
assertion error.

    python tests/gpu_even_m_worker.py <layer> <k> <m> <table_keys binary> <route_owners binary> <scratch directory>"""
from __future__ import annotations

import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import numpy as np

from gpu_per_read_worker import random_dna, revcomp as revcomp_str
from gpu_routing_worker import codes_of, minimizers, pack, revcomp

INVALID = np.uint64(0xFFFFFFFFFFFFFFFF)
POINTS = [(15, 4), (31, 6), (31, 8), (31, 12), (31, 20), (21, 20), (31, 30),  # one word
          (33, 12), (35, 30), (47, 20), (63, 16), (63, 30)]                   # two words
FLOOR = 8  # of every kind of tie, per dictionary and per call
TIE_SIZES = (1, 63, 64, 65, 256, 257)  # around a wave and a workgroup
QUEUE_FILLING = 8193  # with launch pieces of 4096 queries: every query of a piece defers
ROUTE_SHARDS = (3, 1024)
CANDIDATES = 96
LAYERS = {  # name -> (environment, what device_stats() must show)
    "table": ({}, lambda st: st["sk_slots"] > 0),
    "table_pieces": ({"SSHASH_AMD_TEST_HOOKS": "piece=4096"}, lambda st: st["sk_slots"] > 0),
    "directory": ({"SSHASH_AMD_SKTABLE": "0", "SSHASH_AMD_DIRECTORY": "1"}, lambda st: st["sk_slots"] == 0 and st["directory_sectors"] > 0),
    "mphf": ({"SSHASH_AMD_SKTABLE": "0", "SSHASH_AMD_DIRECTORY": "0"}, lambda st: st["sk_slots"] == 0 and st["directory_sectors"] == 0),
}
RECORD = np.dtype([("tie", "u1"), ("rc", "u1"), ("pos", "<u2"), ("zero", "<u4"), ("key", "<u8")])  # tests/cpp/table_keys.cpp


def key_length_of(k, m):
    """the length of the table's key m-mers (csrc/sktable.hip: sk_table_m); the worker holds device_stats()["sk_key_length"] against it"""
    return m if k <= 31 else max(m, k - 32)


def build_host_tool(name, directory):
    """tests/cpp/<name>.cpp by plain g++"""
    exe = os.path.join(str(directory), name)
    subprocess.check_call(["g++", "-O2", "-std=c++17", os.path.join(ROOT, "tests", "cpp", name + ".cpp"), "-o", exe])
    return exe


def table_keys(exe, kmers, k, key_length):
    """-> one RECORD per packed k-mer: what sk_key elects"""
    p = subprocess.run([exe, str(k), str(key_length)], input=np.ascontiguousarray(kmers, dtype=np.uint64).tobytes(), capture_output=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    return np.frombuffer(p.stdout, dtype=RECORD)


def minimizer_ties(kmers, k, m, W, magic):
    """the two strands elect the same minimizer VALUE (what a canonical dictionary calls a tie)"""
    codes = codes_of(kmers, k, W)
    return minimizers(codes, m, magic) == minimizers(codes[:, ::-1] ^ np.uint64(2), m, magic)


def kmers_of(strings, k):
    """every k-mer of every string, in order, packed (W words each)"""
    from oracle.ground_truth import encode_bases, pack_kmers

    W = 1 if k <= 31 else 2
    parts = []
    for s in strings:
        lo, hi = pack_kmers(encode_bases(s), k)
        parts.append(lo if W == 1 else np.stack([lo, hi], axis=1).reshape(-1))
    return np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint64)


def canonical_strings(t, k):
    return {min(x, revcomp_str(x)) for x in (t[i:i + k] for i in range(len(t) - k + 1))}


def canonical_words(kmers, k, W):
    """(n, W) words of the smaller strand of every k-mer, most significant word first (rows compare like the k-mers)"""
    a = np.ascontiguousarray(kmers, dtype=np.uint64).reshape(-1, W)[:, ::-1]
    b = revcomp(kmers, k, W).reshape(-1, W)[:, ::-1]
    less = np.zeros(a.shape[0], dtype=bool)
    undecided = np.ones(a.shape[0], dtype=bool)
    for j in range(W):
        less |= undecided & (b[:, j] < a[:, j])
        undecided &= b[:, j] == a[:, j]
    return np.where(less[:, None], b, a)


_SEQUENCES = {}


def make_sequences(k, m, exe):
    """-> (strings, planted): the input of the point (k, m) -- the same for both flavours -- and, for every planting, (P, index of the
    string, where P starts in it). Deterministic."""
    if (k, m) in _SEQUENCES:
        return _SEQUENCES[(k, m)]
    from oracle import oracle as O

    assert m % 2 == 0 and k % 2 == 1 and m < k
    W, key_length, magic = 1 if k <= 31 else 2, key_length_of(k, m), O.xxh64_u64(1, 0)
    rng = np.random.default_rng(5000 * k + m)
    seen, seqs, planted = set(), [], []

    def add(t):
        mine = canonical_strings(t, k)
        if len(mine) != len(t) - k + 1 or (mine & seen):
            return False
        seen.update(mine)
        seqs.append(t)
        return True

    def add_redrawn(make, tries=60):  # (redraw the flanks until the string's canonical k-mers are new)
        for _ in range(tries):
            t, places = make()
            if add(t):
                planted.extend((t[at:at + m], len(seqs) - 1, at) for at in places)
                return True
        return False

    # ---- random strings of ragged lengths, the shortest exactly one k-mer long
    target = 1500 if k <= 15 else 3500
    lengths = [k, k + 1, 2 * k - 1, 2 * k] + [int(x) for x in rng.integers(k, 6 * k, max(12, target // (5 * k // 2)))]
    for n in lengths:
        while not add(random_dna(rng, n)):
            pass

    # ---- candidates P = h + revcomp(h): trial plantings between random flanks, the ties they produce counted per candidate
    halves = sorted({random_dna(rng, m // 2) for _ in range(4 * CANDIDATES)})
    halves = [halves[int(i)] for i in rng.permutation(len(halves))[:CANDIDATES]]  # (m = 4 has 16 of them: all)
    candidates = [h + revcomp_str(h) for h in halves]
    assert all(p == revcomp_str(p) for p in candidates) and (len(candidates) >= 64 or len(candidates) == 4 ** (m // 2))
    flank = k - m
    trials = [[random_dna(rng, flank) + p + random_dna(rng, flank) for _ in range(4)] for p in candidates]
    per_trial = 4 * (flank + 1)
    trial_kmers = kmers_of([t for four in trials for t in four], k)
    by_key = table_keys(exe, trial_kmers, k, key_length)["tie"].reshape(len(candidates), per_trial).sum(axis=1, dtype=np.int64)
    by_minimizer = minimizer_ties(trial_kmers, k, m, W, magic).reshape(len(candidates), per_trial).sum(axis=1, dtype=np.int64)
    # how many canonical k-mers can hold one P at all: (k - m + 1) places, 4^(k - m) flanks, two strands for one k-mer
    room = (k - m + 1) * 4 ** (k - m) // 2
    few = room < 1000  # m close to k: many P's, each planted as often as its few k-mers allow, some of them left absent
    if few:  # (the best third by either count)
        keep = list(dict.fromkeys(int(i) for x in (by_key, by_minimizer) for i in np.argsort(-x, kind="stable")[:16]))
    else:
        keep = list(dict.fromkeys(int(np.argmax(x)) for x in (by_key, by_minimizer, by_key + by_minimizer)))

    # ---- the plantings
    def between():
        a, b = random_dna(rng, flank + int(rng.integers(1, 6))), random_dna(rng, flank + int(rng.integers(1, 6)))
        return a + p + b, [len(a)]

    def twice():
        gap = int(rng.integers(0, k - 2 * m + 1))  # the second copy starts m + gap <= k - m bases behind the first: one k-mer holds both
        a = random_dna(rng, flank)
        return a + p + random_dna(rng, gap) + p + random_dna(rng, flank), [len(a), len(a) + m + gap]

    for j, i in enumerate(keep):
        p = candidates[i]
        for _ in range(max(1, room // 4) if few else 14):  # (few: half of P's k-mers stay absent)
            if not add_redrawn(between):
                break
        if not few or j == 0:
            add_redrawn(lambda: (p + random_dna(rng, flank + int(rng.integers(0, 4))), [0]))  # P = the string's first m bases
        if not few or j == 1:
            add_redrawn(lambda: ((a := random_dna(rng, flank + int(rng.integers(0, 4)))) + p, [len(a)]))  # ... its last m bases
        if k - m >= m + 1:
            add_redrawn(twice)
    _SEQUENCES[(k, m)] = (seqs, planted)
    return seqs, planted


class Point:
    """one dictionary of an even m, with everything measured about its ties (on the CPU: references only)"""


def substituted(kmers, k, W, rng, limit=400):
    """single substitutions of up to `limit` of the k-mers, at every position -> (packed k-mers, index of the k-mer each one came from)"""
    q = np.ascontiguousarray(kmers, dtype=np.uint64).reshape(-1, W)
    pick = rng.permutation(q.shape[0])[:limit]
    codes = codes_of(q[pick].reshape(-1), k, W)
    out = np.repeat(codes, k, axis=0)
    at = np.tile(np.arange(k), codes.shape[0])
    out[np.arange(out.shape[0]), at] = (out[np.arange(out.shape[0]), at] + rng.integers(1, 4, out.shape[0]).astype(np.uint64)) & np.uint64(3)
    return pack(out, W), np.repeat(pick, k)


def make_point(k, m, canonical, exe, scratch, extend=None, key_length=None):
    """`extend`: strings -> the strings with more behind them (tests/gpu_forms_worker.py adds long ones); `key_length`: the length of
    the table's keys where it is not the default (SSHASH_AMD_SK_M), for what is measured about table-key ties"""
    from conftest import Case
    from oracle import oracle as O
    from test_gpu_streaming import _synthetic_reads

    seqs, planted = make_sequences(k, m, exe)
    if extend is not None:
        seqs = extend(seqs)  # (behind the others: `planted` holds indices)
    pt = Point()
    pt.k, pt.m, pt.canonical, pt.W, pt.key_length, pt.magic = k, m, canonical, 1 if k <= 31 else 2, key_length or key_length_of(k, m), O.xxh64_u64(1, 0)
    pt.sequences, pt.planted = seqs, planted
    pt.case = case = Case(f"even_k{k}_m{m}_{int(canonical)}", seqs, k, m, canonical, scratch)
    W, n = pt.W, case.gt.num_kmers
    pt.every = every = case.gt.kmers(np.arange(n))
    assert (every == kmers_of(seqs, k)).all()
    pt.every_rc = revcomp(every, k, W)
    rng = np.random.default_rng(7000 * k + m + int(canonical))
    neg = rng.integers(0, 1 << 62, (n, W), dtype=np.uint64)
    neg[:, -1] &= np.uint64((1 << (2 * k - 64 * (W - 1))) - 1)
    pt.random_negatives = neg.reshape(-1)

    def ties_of(kmers):  # -> {"table": ..., "minimizer": ...}; a regular dictionary has no minimizer ties (it probes strand by strand)
        t = {"table": table_keys(exe, kmers, k, pt.key_length)["tie"] != 0}
        if canonical:
            t["minimizer"] = minimizer_ties(kmers, k, m, W, pt.magic)
        return t

    pt.kinds = ("table", "minimizer") if canonical else ("table",)
    pt.ties = ties_of(every)
    for kind, t in ties_of(pt.every_rc).items():
        assert (t == pt.ties[kind]).all(), f"{kind}: a k-mer ties and its reverse complement does not"
    # negatives that tie: one substitution in a k-mer that ties, kept if the tie survives (the substitution lies outside what the
    # election looks at, or makes another tie) and the k-mer is absent -- both measured
    pt.negative_ties = {}
    for kind in pt.kinds:
        source = every.reshape(n, W)[pt.ties[kind]].reshape(-1)
        if source.size == 0:
            pt.negative_ties[kind] = np.zeros(0, dtype=np.uint64)
            continue
        cand, _ = substituted(source, k, W, rng)
        ok = ties_of(cand)[kind] & (case.oracle.lookup_ids(cand) == INVALID)
        cand = np.unique(cand.reshape(-1, W)[ok], axis=0)
        pt.negative_ties[kind] = np.ascontiguousarray(cand[rng.permutation(cand.shape[0])[:256]]).reshape(-1)
    # the pool the tie-only batches are cut from: every tie of the dictionary on both strands, and the negative ties
    parts = []
    for kind in pt.kinds:
        mine = every.reshape(n, W)[pt.ties[kind]]
        parts += [mine, pt.every_rc.reshape(n, W)[pt.ties[kind]], pt.negative_ties[kind].reshape(-1, W)]
    pool = np.unique(np.concatenate(parts), axis=0)
    pt.pool = np.ascontiguousarray(pool[rng.permutation(pool.shape[0])]).reshape(-1)
    pt.pool_ties = ties_of(pt.pool)
    pt.pool_found = case.oracle.lookup_ids(pt.pool) != INVALID
    # reads: the sweep's, and hand-made ones that walk through P
    reads = _synthetic_reads(case, 160, seed=k + m, read_len=3 * k)
    done = set()
    for p, s, at in planted:
        t = seqs[s]
        if (p, at == 0, at + m == len(t)) in done and len(done) > 6:
            continue
        done.add((p, at == 0, at + m == len(t)))
        inside = at + m // 2
        reads += [t, revcomp_str(t), t[:inside] + "ACGT"[("ACGT".index(t[inside]) + 1) % 4] + t[inside + 1:], t[:inside] + "N" + t[inside + 1:]]
    pt.reads = reads
    valid = set("ACGTacgt")
    windows = [r[i:i + k].upper() for r in reads for i in range(len(r) - k + 1) if all(c in valid for c in r[i:i + k])]
    pt.read_kmers = kmers_of(windows, k)
    pt.read_ties = ties_of(pt.read_kmers)
    pt.read_found = case.oracle.lookup_ids(pt.read_kmers) != INVALID
    return pt


def tie_counts(pt):
    """what the floors are asked of: per kind, ties among the dictionary's k-mers, negative ties, ties the reads walk over (found and not)"""
    out = {}
    for kind in pt.kinds:
        out[kind] = {"dictionary": int(pt.ties[kind].sum()), "negatives": int(pt.negative_ties[kind].size // pt.W),
                     "read_kmers_found": int((pt.read_ties[kind] & pt.read_found).sum()), "read_kmers_absent": int((pt.read_ties[kind] & ~pt.read_found).sum())}
    return out


def assert_floors(pt):
    counts = tie_counts(pt)
    for kind, c in counts.items():
        assert c["dictionary"] >= FLOOR and c["negatives"] >= FLOOR, (pt.k, pt.m, pt.canonical, kind, c)
        assert c["read_kmers_found"] >= FLOOR, (pt.k, pt.m, pt.canonical, kind, c)
    return counts


def batch_counts(pt, index):
    """per kind: how many queries of pool[index] tie and are in the dictionary, and how many tie and are not"""
    return {kind: [int((pt.pool_ties[kind][index] & pt.pool_found[index]).sum()), int((pt.pool_ties[kind][index] & ~pt.pool_found[index]).sum())]
            for kind in pt.kinds}


# ---- the device ----------------------------------------------------------------------------------------------------------------------
def check_flavour(pt, layer, route_owners_exe):
    import torch

    import sshash_amd
    from gpu_cover_worker import device_cover
    from gpu_layer_worker import ALL_FIELDS, DEVICE_FORMS, assert_fields, device_lookup, mixed_case, packed_to_ascii
    from gpu_per_read_worker import device_rows, oracle_rows, report_row
    from gpu_routing_worker import ENTRIES, Reference, host_key_owners, to_device, two_calls
    from gpu_runs_worker import check_both, oracle_runs
    from test_gpu_streaming import _as_dict

    case, k, m, W = pt.case, pt.k, pt.m, pt.W
    what = f"{layer} k={k} m={m} {'canonical' if pt.canonical else 'regular'}"
    d = case.dict.to_device(0)
    st = d.device_stats(0)
    assert LAYERS[layer][1](st), f"{what}: the replica is not the {layer} layer: {st}"
    assert st["sk_key_length"] == pt.key_length, (what, st["sk_key_length"], pt.key_length)
    n = case.gt.num_kmers
    sent = {}

    def count(call, index):
        c = batch_counts(pt, index)
        mine = sent.setdefault(call, {kind: [0, 0] for kind in pt.kinds})
        for kind in pt.kinds:
            mine[kind] = [max(a, b) for a, b in zip(mine[kind], c[kind])]  # (the largest batch of the call: batches repeat k-mers)

    # ---- every k-mer, every reverse complement, as many random negatives
    Q = np.concatenate([pt.every, pt.every_rc, pt.random_negatives])
    N = Q.size // W
    want = case.oracle.lookup_packed(Q, True)
    want_fwd = case.oracle.lookup_packed(Q, False)
    ids = np.arange(n, dtype=np.uint64)
    assert (want["kmer_id"][:n] == ids).all() and (want["kmer_id"][n:2 * n] == ids).all(), f"{what}: the oracle's ids are not the file order"
    assert_fields(d.lookup(Q, full=True), want, ALL_FIELDS, f"{what} host full")
    assert_fields(d.lookup(Q), want, ("kmer_id",), f"{what} host ids")
    assert (d.is_member(Q) == (want["kmer_id"] != INVALID)).all(), f"{what} host is_member"
    assert_fields(d.lookup(Q, check_reverse_complement=False, full=True), want_fwd, ALL_FIELDS, f"{what} host forward only")
    dq = torch.from_numpy(Q.view(np.int64)).to("cuda:0")
    for form, fields in DEVICE_FORMS.items():
        assert_fields(device_lookup(d, dq.data_ptr(), N, fields), want, fields, f"{what} device packed {form}")
    assert_fields(device_lookup(d, dq.data_ptr(), N, ("kmer_id",), check_rc=False), want_fwd, ("kmer_id",), f"{what} device forward only")
    member = torch.full((N,), 7, dtype=torch.uint8, device="cuda:0")
    d.is_member_device(0, dq.data_ptr(), N, member.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert (member.cpu().numpy() == (want["kmer_id"] != INVALID)).all(), f"{what} device is_member"
    text = mixed_case(packed_to_ascii(Q, k), k + m)
    assert_fields(d.lookup(text, full=True), want, ALL_FIELDS, f"{what} ascii host")
    staged = torch.zeros(text.size + 1, dtype=torch.uint8, device="cuda:0")
    staged[1:] = torch.from_numpy(text.reshape(-1)).to("cuda:0")
    for form in ("ids", "full"):
        assert_fields(device_lookup(d, staged.data_ptr() + 1, N, DEVICE_FORMS[form], ascii_input=True), want, DEVICE_FORMS[form], f"{what} ascii device {form}")
    dictionary_ties = {kind: int(pt.ties[kind].sum()) for kind in pt.kinds}

    # ---- batches of ties only: dictionary k-mers that tie on both strands, negatives that tie
    pool_n = pt.pool.size // W
    pool = pt.pool.reshape(pool_n, W)
    for size in TIE_SIZES + (QUEUE_FILLING,):
        index = (np.arange(size) + size) % pool_n  # (a window of the shuffled pool that moves with the size; repeats beyond the pool's size)
        b = np.ascontiguousarray(pool[index]).reshape(-1)
        w = case.oracle.lookup_packed(b, True)
        for kind in pt.kinds:
            assert pt.pool_ties[kind][index].any() or size == 1
        assert_fields(d.lookup(b, full=True), w, ALL_FIELDS, f"{what} ties, host full, {size}")
        count("lookup_host", index)
        db = torch.from_numpy(b.view(np.int64)).to("cuda:0")
        for form, fields in DEVICE_FORMS.items():
            assert_fields(device_lookup(d, db.data_ptr(), size, fields), w, fields, f"{what} ties, device {form}, {size}")
        count("lookup_device", index)
        truth = case.gt.lookup(b)  # the input decides ids and strands of the k-mers that are there
        assert (w["kmer_id"] == truth["kmer_id"]).all(), f"{what} ties: oracle against the input, {size}"
    # ---- the routing calls on ties: minimizer owners against the numpy restatement, key owners against the host's sk_key / sk_owner
    index = np.arange(min(pool_n, 4096))
    b = np.ascontiguousarray(pool[index]).reshape(-1)
    ref = Reference(b, k, m, W, pt.canonical, pt.magic, host_key_owners(route_owners_exe, b, k, pt.key_length, ROUTE_SHARDS))
    d_b = to_device(b)
    for S in ROUTE_SHARDS:
        owners = [torch.full((ref.n,), -1, dtype=torch.int32, device="cuda:0") for _ in range(2)]
        d.route_device(0, d_b.data_ptr(), ref.n, S, owners[0].data_ptr(), owners[1].data_ptr())
        torch.cuda.synchronize()
        for got, expected, which in zip(owners, ref.owners(S, "minimizer", True), ("forward", "reverse")):
            bad = np.flatnonzero(got.cpu().numpy() != expected)
            assert bad.size == 0, (what, "route_device on ties", S, which, "first differing query", int(bad[0]))
        for entry, check_rc in ENTRIES:
            f, r = ref.owners(S, entry, check_rc)
            two_calls(d, entry, check_rc, b, W, S, f, r, f"{what} ties, {entry} owners, check_rc={int(check_rc)}, S={S}")
    count("route_device", index)
    count("route_bucket", index)
    count("route_bucket_by_key", index)

    # ---- streaming: the reads walk through P on both strands, with a substitution and an N inside it
    reads = pt.reads
    want_report = case.oracle.streaming_query(reads)
    assert _as_dict(d.streaming_query(reads)) == want_report, f"{what} streaming_query"
    per_read, report = d.streaming_lookup(reads, full=True)
    assert _as_dict(report) == want_report, f"{what} streaming_lookup report"
    for r, (read, got) in enumerate(zip(reads, per_read)):
        wr = case.oracle.streaming_read(read)
        assert got.kmer_id.size == wr.size == max(0, len(read) - k + 1)
        found = wr["kmer_id"] != INVALID
        assert_fields(got, wr, ("kmer_id", "kmer_id_in_string", "string_id", "string_begin", "string_end"), f"{what} streaming read {r}")
        assert (got.kmer_orientation[found] == wr["kmer_orientation"][found]).all(), f"{what} streaming read {r} orientation"
    want_rows = oracle_rows(case.oracle, reads)
    rows, rep = d.streaming_query_per_read(reads)
    assert (rows == want_rows).all(), f"{what} per-read rows: reads {np.flatnonzero((rows != want_rows).any(1))[:10]} differ"
    assert (report_row(rep) == want_rows.sum(0)).all(), f"{what} per-read report"
    rows, _ = device_rows(d, reads, prefill=-1, report=[0] * 6)
    assert (rows == want_rows).all(), f"{what} per-read device rows: reads {np.flatnonzero((rows != want_rows).any(1))[:10]} differ"
    want_offsets, want_runs = oracle_runs(case.oracle, reads)
    check_both(d, reads, want_offsets, want_runs, what)
    run_offsets, runs, _ = d.streaming_runs(reads)
    for r, (back, got) in enumerate(zip(sshash_amd.expand_runs(run_offsets, runs, [len(x) for x in reads], k), per_read)):
        found = got.kmer_id != INVALID
        assert_fields(back, got, ("kmer_id", "kmer_id_in_string", "string_id"), f"{what} expand_runs against streaming_lookup, read {r}")
        assert (back.kmer_orientation[found] == got.kmer_orientation[found]).all(), f"{what} expand_runs orientation, read {r}"
    positive = np.concatenate([p.kmer_id for p in per_read])
    positive = np.unique(positive[positive != INVALID])
    cover, rep = d.streaming_cover(reads)
    assert (sshash_amd.cover_to_ids(cover) == positive).all() and _as_dict(rep) == want_report, f"{what} streaming_cover"
    cover, _ = device_cover(d, reads)
    assert sshash_amd.cover_to_ids(cover).tolist() == positive.tolist(), f"{what} streaming_cover_device"
    for call in ("streaming_query", "streaming_lookup", "streaming_query_per_read", "streaming_runs", "streaming_cover"):
        sent[call] = {kind: [int((pt.read_ties[kind] & pt.read_found).sum()), int((pt.read_ties[kind] & ~pt.read_found).sum())] for kind in pt.kinds}
    d.close()
    return {"kmers": n, "strings": len(pt.sequences), "sk_slots": st["sk_slots"], "directory_sectors": st["directory_sectors"],
            "dictionary_ties": dictionary_ties, "sent": sent}


def main():
    import tempfile

    layer, k, m, table_keys_exe, route_owners_exe = sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), sys.argv[4], sys.argv[5]
    out, seconds = {}, {}
    with tempfile.TemporaryDirectory(dir=sys.argv[6]) as tmp:
        for canonical in (False, True):
            t0 = time.time()
            pt = make_point(k, m, canonical, table_keys_exe, tmp)
            floors = assert_floors(pt)
            t1 = time.time()
            name = "canonical" if canonical else "regular"
            out[name] = dict(check_flavour(pt, layer, route_owners_exe), floors=floors)
            seconds[name] = [round(t1 - t0, 2), round(time.time() - t1, 2)]  # (references on the CPU, calls on the device)
    print(json.dumps({"ok": True, "layer": layer, "k": k, "m": m, "dictionaries": out, "seconds": seconds}))


if __name__ == "__main__":
    main()
