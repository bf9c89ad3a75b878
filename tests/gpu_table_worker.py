#!/usr/bin/env python
"""Worker of tests/test_gpu_table_build.py, and the inputs it shares with tests/test_table_inputs.py: the super-k-mer table that a
replica builds at upload (csrc/sktable.hip), exported (Dictionary.device_table) and held against what the strings say it must hold
(tests/table_reference.py: Reference and verify).

One worker process = one point (k, m, length of the table's keys), regular then canonical. The dictionary is the walks' (make_inputs
with gpu_walks_worker.extension_of: at (33, 13) the two colliding keys under the packed layer) with the strings that table_extension
plants behind -- and, where it has to, in front of -- them, so that every point reaches the edges that conditions() asserts. Per
flavour SIX uploads of fresh handles of the same index file, one after the other:

    default | packed (SSHASH_AMD_TEST_HOOKS=slots_per_key=1.2,slots_per_kmer=1.2) | SSHASH_AMD_SK_DENSITY=compact | shards 0, 1, 2 of 3

sktable.hip reads SSHASH_AMD_SK_DENSITY at every build and the hooks are read at every call of the C ABI, so the worker sets the two in
its own environment between the uploads (and asserts from the published numbers that each took: they are compared exactly with what
the reference says for that density). SSHASH_AMD_SK_M is the test's to set: it is the same for all six.

Per upload: device_stats() and device_table_histogram() against the reference, exact; the info of the export against both; verify()
without a violation, the items present and absent against sk_slots_used and sk_deferred_keys; then lookups on the same replica: every
k-mer of the dictionary on both strands returns its id, and every window of k bases across the border of two neighbouring stored
strings, and its reverse complement, gets the oracle's answer (GroundTruth.lookup says the same, asserted on the CPU first) -- the one
query whose answer an over-long extent changes. On the default upload also the export's own edges (export_edges: info alone, a capacity
one byte short, a larger buffer, a replica without a table). Over the three shards: every key is owned exactly once, and the sums of
sk_keys and of the items are the whole table's. Prints one JSON line; any mismatch is an assertion error.

    python tests/gpu_table_worker.py <k> <m> <key_length or 0> <table_keys binary> <table_hashes binary> <scratch dir> [--cpu-only]"""
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

from gpu_even_m_worker import key_length_of, table_keys
from gpu_forms_worker import INVALID, _adder, make_inputs
from gpu_per_read_worker import random_dna
from gpu_routing_worker import pack
from gpu_routing_worker import revcomp as packed_revcomp
from gpu_walks_worker import COLLIDING, PACKED_HOOKS, colliding_gate, extension_of
from table_reference import DENSITIES, SK_INLINE_MAX, Reference, verify

POINTS = [(21, 11, 0), (31, 7, 0), (31, 21, 17), (31, 27, 0), (33, 13, 0), (47, 15, 31), (63, 25, 12), (63, 31, 0)]  # (k, m, key length or 0), of the walks' list
SHARDS = 3
UPLOADS = [  # (name, density of table_reference.DENSITIES, environment, table shards, shard id)
    ("default", "default", {}, 1, 0),
    ("packed", "packed", {"SSHASH_AMD_TEST_HOOKS": PACKED_HOOKS}, 1, 0),
    ("compact", "compact", {"SSHASH_AMD_SK_DENSITY": "compact"}, 1, 0),
    ("shard 0", "default", {}, SHARDS, 0),
    ("shard 1", "default", {}, SHARDS, 1),
    ("shard 2", "default", {}, SHARDS, 2),
]
FLOOR = 8  # buckets that are the first choice of more items than they hold
STAT_NAMES = ("sk_keys", "sk_inline_keys", "sk_heavy_keys", "sk_heavy_kmers", "sk_key_length", "sk_slots", "sk_bytes")


def environment_of(key_length):
    """what the test puts into the worker's environment (every other SSHASH_AMD_* setting is taken out first)"""
    return {"SSHASH_AMD_SK_M": str(key_length)} if key_length else {}


# ---- the strings ---------------------------------------------------------------------------------------------------------------------------
_EDGES = {}
_LETTERS = np.frombuffer(b"ACTG", dtype=np.uint8)  # code -> character


def _planted(rng, motif, n, k):
    """n k-mers of random bases with the motif's codes at a random place each -> (n, k) codes"""
    codes = rng.integers(0, 4, (n, k)).astype(np.uint64)
    at = rng.integers(0, k - motif.size + 1, n)
    codes[np.arange(n)[:, None], at[:, None] + np.arange(motif.size)[None, :]] = motif[None, :]
    return codes


def with_table_edges(seqs, k, L, keys_exe, hashes_exe, seed):
    """seqs with what conditions() asks for and the point may lack: behind, five strings of exactly k bases whose k-mer elects one new key
    and four that elect another (a key with exactly SK_INLINE_MAX + 1 tuples, a marker, and one with exactly SK_INLINE_MAX, inline; the
    last of them ends the collection); in front, a string whose first k-mers elect an inline occurrence less than k - L bases into the
    collection (read_bases' negative positions) -- only where the first string has none. The motifs are, of 96 drawn, the two that win
    the most elections between random flanks, and the flanks are drawn until tests/cpp/table_keys.cpp says so. The same for both
    flavours: kept per process."""
    at = (k, L, seed, hash(tuple(seqs)))
    if at in _EDGES:
        return list(_EDGES[at])
    rng = np.random.default_rng(seed)
    seqs = list(seqs)
    km, W = k - L, 1 if k <= 31 else 2
    taken = set(Reference(seqs, k, L, keys_exe, hashes_exe).all_keys.tolist())
    add = _adder(seqs, k)

    def wins(motif, n):
        codes = _planted(rng, motif, n, k)
        elected = table_keys(keys_exe, pack(codes, W), k, L)
        value = sum(int(c) << (2 * j) for j, c in enumerate(motif))
        return codes[(elected["key"] == np.uint64(value)) & (elected["tie"] == 0)], value

    motifs = [m for m in rng.integers(0, 4, (96, L)).astype(np.uint64) if sum(int(c) << (2 * j) for j, c in enumerate(m)) not in taken]
    motifs.sort(key=lambda m: -wins(m, 80)[0].shape[0])
    for copies, motif in ((SK_INLINE_MAX + 1, motifs[0]), (SK_INLINE_MAX, motifs[1])):
        good, value = wins(motif, 1500)
        done = 0
        for row in good:
            done += add(_LETTERS[row.astype(np.int64)].tobytes().decode("ascii"))
            if done == copies:
                break
        assert done == copies and value not in taken, (done, good.shape)
        taken.add(value)
    if not (Reference(seqs, k, L, keys_exe, hashes_exe).inline.p < km).any():
        for _ in range(400):
            t = random_dna(rng, 2 * k)
            if add(t):
                seqs.pop()
                if (Reference([t] + seqs, k, L, keys_exe, hashes_exe).inline.p < km).any():
                    seqs = [t] + seqs
                    break
        else:
            raise AssertionError("no first string with an occurrence less than k - L bases in")
    _EDGES[at] = list(seqs)
    return seqs


def table_extension(k, m, key_length, keys_exe, hashes_exe):
    """-> what make_inputs puts around the point's own strings: the walks' extension for the packed layer, then with_table_edges"""
    walks = extension_of(k, m, key_length, "packed", keys_exe)
    L = key_length or key_length_of(k, m)

    def extend(seqs):
        return with_table_edges(walks(seqs) if walks else seqs, k, L, keys_exe, hashes_exe, 9500 * k + m)

    return extend


def first_choices(ref, density):
    """how many items of the keys' region have each of its buckets as their first choice, at that density"""
    lay = ref.layout(density)
    inline, markers, _ = ref.choices(lay["key_buckets"], lay["kmer_buckets"])
    return np.bincount(np.concatenate([np.repeat(inline[:, 0], ref.inline.mult), markers[:, 0]]), minlength=lay["key_buckets"])


def conditions(ref):
    """the edges that the inputs of a point must reach, asserted on the reference alone -> what it holds"""
    k, L, km, I = ref.k, ref.L, ref.k - ref.L, ref.inline
    ends_last = int((I.p + L + I.right == ref.num_bases).sum()) + (int((ref.heavy.start + k == ref.num_bases).sum()) if ref.heavy.n else 0)
    got = {"keys_with_4_tuples": int((ref.key_sizes == 4).sum()), "keys_with_5_tuples": int((ref.key_sizes == 5).sum()),
           "keys_in_bins_1_2_3_and_5_to_8": [ref.histogram[i] for i in (0, 1, 2, 4)],
           "inline_occurrences_less_than_k_minus_L_bases_in": int((I.p < km).sum()), "strings_of_k_bases": int((ref.string_lengths == k).sum()),
           "items_that_end_the_collection": ends_last, "super_kmers_of_1_kmer": int((ref.tuple_kmers == 1).sum()),
           "super_kmers_of_all_kmers": int((ref.tuple_kmers == km + 1).sum()), "inline_by_strand": np.bincount(I.strand, minlength=2).tolist(),
           "buckets_first_choice_of_2": {name: int((first_choices(ref, name) >= 2).sum()) for name in DENSITIES},
           "packed_buckets_first_choice_of_3": int((first_choices(ref, "packed") >= 3).sum()), "heavy_kmers": ref.sk_heavy_kmers}
    assert got["keys_with_4_tuples"] >= 1 and got["keys_with_5_tuples"] >= 1, got
    assert all(n >= 1 for n in got["keys_in_bins_1_2_3_and_5_to_8"]), got
    assert got["inline_occurrences_less_than_k_minus_L_bases_in"] >= 1 and int(I.p.min()) < km <= int(ref.string_lengths[0]), got
    assert got["strings_of_k_bases"] >= 1 and got["items_that_end_the_collection"] >= 1, got
    assert got["super_kmers_of_1_kmer"] >= 1 and got["super_kmers_of_all_kmers"] >= 1 and int(ref.tuple_kmers.max()) <= km + 1, got
    assert min(got["inline_by_strand"]) >= 1 and ref.sk_heavy_kmers >= 1, got
    assert min(got["buckets_first_choice_of_2"].values()) >= FLOOR and got["packed_buckets_first_choice_of_3"] >= FLOOR, got
    return got


def expected_numbers(ref, density):
    """-> (device_stats() entries, the 20 words of the histogram) that the build must publish"""
    lay = ref.layout(density)
    stats = {"sk_keys": ref.sk_keys, "sk_inline_keys": ref.sk_inline_keys, "sk_heavy_keys": ref.sk_heavy_keys, "sk_heavy_kmers": ref.sk_heavy_kmers,
             "sk_key_length": ref.L, "sk_slots": lay["sk_slots"], "sk_bytes": lay["sk_bytes"]}
    return stats, ref.histogram + [ref.tuples, ref.items]


# ---- the lookups ---------------------------------------------------------------------------------------------------------------------------
def border_windows(ref):
    """every window of k bases that holds the border of two neighbouring stored strings, packed -> (n * W words, n)"""
    k = ref.k
    starts = np.concatenate([np.arange(max(0, e - k + 1), e) for e in ref.offsets[1:-1]])
    starts = starts[starts + k <= ref.num_bases]
    codes = np.lib.stride_tricks.sliding_window_view(ref.bases.astype(np.uint64), k)[starts]
    return pack(codes, ref.W), int(starts.size)


def lookup_gate(pt, ref):
    """the queries of one flavour and their answers, on the CPU: every k-mer on both strands -> its id; the border windows and their
    reverse complements -> the oracle's answer, which is GroundTruth.lookup's"""
    k, W, case = ref.k, ref.W, pt.case
    n = case.gt.num_kmers
    assert ref.kmers.shape[0] == n and [int(x) for x in case.gt.endpoints] == [int(x) for x in ref.offsets]
    forward = np.ascontiguousarray(ref.kmers).reshape(-1)
    borders, n_borders = border_windows(ref)
    queries = np.concatenate([forward, packed_revcomp(forward, k, W), borders, packed_revcomp(borders, k, W)])
    want = case.oracle.lookup_ids(queries)
    truth = case.gt.lookup(queries)["kmer_id"]
    assert (want == truth).all(), "the oracle's ids against GroundTruth.lookup"
    ids = np.arange(n, dtype=np.uint64)
    assert (want[:n] == ids).all() and (want[n:2 * n] == ids).all()
    held = int((want[2 * n:] != INVALID).sum())
    return queries, want, {"kmers": n, "border_windows": n_borders, "border_windows_that_the_dictionary_holds": held}


# ---- the device ----------------------------------------------------------------------------------------------------------------------------
def upload_and_check(index_path, name, density, env, shards, shard_id, ref, queries, want):
    """one upload of a fresh handle -> what was measured"""
    import sshash_amd

    for var in ("SSHASH_AMD_TEST_HOOKS", "SSHASH_AMD_SK_DENSITY"):
        os.environ.pop(var, None)
    os.environ.update(env)
    try:
        d = sshash_amd.Dictionary.load(index_path)
        d.to_device(0, table_shards=shards, table_shard_id=shard_id)
        st, hist = d.device_stats(0), d.device_table_histogram(0)
        info, words = d.device_table(0)
        got = d.lookup(queries).kmer_id
        if name.endswith("default"):
            export_edges(d, info, words, index_path)
    finally:
        for var in env:
            os.environ.pop(var, None)
    d.close()
    what = f"{name}: "
    want_stats, want_hist = expected_numbers(ref, density)
    assert {x: st[x] for x in STAT_NAMES} == want_stats, (what + "device_stats()", {x: st[x] for x in STAT_NAMES}, want_stats)
    flat = list(hist["keys_by_occurrences"].values()) + list(hist["super_kmers_by_occurrences_of_their_key"].values()) + [hist["super_kmers"], hist["slots_asked_for"]]
    assert flat == want_hist, (what + "device_table_histogram()", flat, want_hist)
    assert st["sk_slots_used"] + st["sk_deferred_keys"] == ref.items, (what + "slots used and items without one", st, ref.items)
    assert info == ref.info_of(density), (what + "the info of the export", info, ref.info_of(density))
    assert info["bytes"] == st["sk_bytes"] == 4 * words.size
    counts = {}
    violations = verify(words, info, ref, stats=st, counts=counts)
    assert not violations, (what + "verify()", len(violations), violations[:12])
    assert counts["present"] == st["sk_slots_used"] and counts["absent"] == st["sk_deferred_keys"]
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (what + "lookups: (query, got, want)", [(int(i), int(got[i]), int(want[i])) for i in bad[:6]])
    return {"sk_deferred_keys": st["sk_deferred_keys"], "sk_slots_used": st["sk_slots_used"], "past_first_choice": counts["past_first_choice"],
            "in_slot_1_or_a_later_entry": counts["in_slot_1_or_a_later_entry"], "sk_keys": st["sk_keys"], "items": ref.items}


def export_edges(d, info, words, index_path):
    """the export's own contract on a replica: info alone, a buffer one byte too small (SSHASH_ERR_ARGUMENT, nothing written), a larger
    one (nothing written behind the table), and a replica without a table (all-zero info, nothing copied, OK -- as the histogram)"""
    import ctypes as C

    import sshash_amd
    from sshash_amd import _binding as B

    lib, raw, guard = B._load(), (C.c_uint64 * 8)(), np.uint32(0xA5A5A5A5)
    lib.sshash_last_error.restype = C.c_char_p
    assert lib.sshash_device_table_export(d._h, 0, C.byref(raw), None, 0) == 0 and [int(x) for x in raw] == list(info.values())
    room = np.full(words.size + 16, guard, dtype=np.uint32)
    assert lib.sshash_device_table_export(d._h, 0, C.byref(raw), room.ctypes.data_as(C.c_void_p), words.nbytes - 1) == 1
    assert b"smaller than the table" in lib.sshash_last_error() and (room == guard).all()
    assert lib.sshash_device_table_export(d._h, 0, C.byref(raw), room.ctypes.data_as(C.c_void_p), room.nbytes) == 0
    assert (room[:words.size] == words).all() and (room[words.size:] == guard).all()
    os.environ["SSHASH_AMD_SKTABLE"] = "0"
    try:
        bare = sshash_amd.Dictionary.load(index_path).to_device(0)
        st, (none, nothing) = bare.device_stats(0), bare.device_table(0)
        assert st["sk_slots"] == 0 and st["sk_absent_reason"] == "disabled" and set(none.values()) == {0} and nothing.size == 0, (st, none)
        assert lib.sshash_device_table_export(bare._h, 0, C.byref(raw), room.ctypes.data_as(C.c_void_p), room.nbytes) == 0 and not any(raw)
        assert set(bare.device_table_histogram(0)["keys_by_occurrences"].values()) == {0}
        bare.close()
    finally:
        del os.environ["SSHASH_AMD_SKTABLE"]


def shards_gate(whole, parts):
    """every key is owned exactly once; the keys and the items of the three shards are the whole table's"""
    owned = np.concatenate([r.keys for r in parts])
    # (a shard's keys are those of its tuples; the whole table's, those of every k-mer that has one)
    assert owned.size == np.unique(owned).size == whole.sk_keys and (np.sort(owned) == whole.keys).all(), "every key is owned exactly once"
    assert sum(r.sk_keys for r in parts) == whole.sk_keys
    # A tuple of the whole table is a tuple of its key's shard: its left neighbour elects another occurrence there as well, or has no key there
    assert sum(r.tuples for r in parts) == whole.tuples and sum(r.items for r in parts) == whole.items, ([r.items for r in parts], whole.items)


def main():
    import tempfile

    k, m, key_length, keys_exe, hashes_exe, scratch = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), sys.argv[4], sys.argv[5], sys.argv[6]
    cpu_only = "--cpu-only" in sys.argv[7:]
    assert (k, m, key_length) in POINTS
    L = key_length or key_length_of(k, m)
    assert os.environ.get("SSHASH_AMD_SK_M", "") == (str(key_length) if key_length else "")
    out, seconds = {}, {}
    with tempfile.TemporaryDirectory(dir=scratch) as tmp:
        for canonical in (False, True):
            name = "canonical" if canonical else "regular"
            t0 = time.time()
            pt = make_inputs(k, m, key_length, canonical, keys_exe, tmp, extend=table_extension(k, m, key_length, keys_exe, hashes_exe))
            refs = {(1, 0): Reference(pt.sequences, k, L, keys_exe, hashes_exe)}
            for s in range(SHARDS):
                refs[(SHARDS, s)] = Reference(pt.sequences, k, L, keys_exe, hashes_exe, SHARDS, s)
            out[name] = {"conditions": conditions(refs[(1, 0)])}
            shards_gate(refs[(1, 0)], [refs[(SHARDS, s)] for s in range(SHARDS)])
            if ("packed", k, m, key_length) in COLLIDING:
                out[name]["colliding_keys"] = colliding_gate(pt, key_length, COLLIDING[("packed", k, m, key_length)], keys_exe)
            queries, want, held = lookup_gate(pt, refs[(1, 0)])
            out[name]["lookups"] = held
            t1 = time.time()
            if not cpu_only:
                uploads = {}
                for upload, density, env, shards, shard_id in UPLOADS:
                    uploads[upload] = upload_and_check(pt.case.index_path, f"{name}, {upload}", density, env, shards, shard_id, refs[(shards, shard_id)], queries, want)
                parts = [uploads[f"shard {s}"] for s in range(SHARDS)]
                assert sum(p["sk_keys"] for p in parts) == uploads["default"]["sk_keys"] and sum(p["items"] for p in parts) == uploads["default"]["items"]
                out[name]["uploads"] = uploads
            seconds[name] = [round(t1 - t0, 2), round(time.time() - t1, 2)]  # (inputs and references on the CPU, the six uploads and their checks)
    print(json.dumps({"ok": True, "k": k, "m": m, "key_length": key_length, "cpu_only": cpu_only, "dictionaries": out, "seconds": seconds}))


if __name__ == "__main__":
    main()
