"""CPU: the reference and the verifier of tests/test_gpu_table_build.py, and the inputs of its points, before a device is involved.

The reference (tests/table_reference.py) reproduces, from the strings and tests/cpp/table_keys.cpp alone, the sk_heavy_kmers that
tests/test_gpu_streaming_walks.py records from an MI355X for the ten dictionaries of its packed layer. The verifier bites: a
sequential placer in this file -- first fit in choice order, the items in a shuffled order, its own encoding of slots and entries --
lays the reference's items out at every point and density and for a shard, verify() finds nothing on its tables, and names each of
thirteen corruptions of one place. The inputs reach the edges: gpu_table_worker.conditions(), per point and flavour."""
from __future__ import annotations

import numpy as np
import pytest

from gpu_even_m_worker import build_host_tool, key_length_of
from gpu_forms_worker import make_inputs
from gpu_table_worker import FLOOR, POINTS, SHARDS, conditions, expected_numbers, shards_gate, table_extension
from gpu_walks_worker import POINTS as WALKS_POINTS
from gpu_walks_worker import extension_of
from table_reference import (DENSITIES, SK_FILTER_BITS, SK_FILTER_SHIFT, SK_GO_ON, SK_INLINE_MAX, SK_LEFT_SHIFT, SK_MARKER, SK_RIGHT_SHIFT, SK_SECOND_FINGERPRINT_WORD,
                             SK_SECOND_USED, SK_STRAND, SK_VALID, Reference, table_hashes, verify)

RECORDED_HEAVY_KMERS = [836, 15018, 559, 2030, 33, 718, 42, 3627, 15, 868]  # tests/test_gpu_streaming_walks.py, the packed layer, in the order of its points
BUCKET_FLAGS = (31 << 3) | SK_SECOND_USED | (((1 << SK_FILTER_BITS) - 1) << SK_FILTER_SHIFT)


def case_id(k, m, key_length):
    return f"k{k}m{m}" + (f"key{key_length}" if key_length else "")


@pytest.fixture(scope="module")
def tools(tmp_path_factory):
    directory = tmp_path_factory.mktemp("table_tools")
    return build_host_tool("table_keys", directory), build_host_tool("table_hashes", directory)


_REFERENCES = {}


def reference_of(k, m, key_length, canonical, tools, tmp_path):
    """the reference of a point's dictionary; the strings of the two flavours are the same, so is the reference: one per point and process"""
    pt = make_inputs(k, m, key_length, canonical, tools[0], str(tmp_path), extend=table_extension(k, m, key_length, *tools))
    at = (k, m, key_length, hash(tuple(pt.sequences)))
    if at not in _REFERENCES:
        _REFERENCES[at] = Reference(pt.sequences, k, key_length or key_length_of(k, m), *tools)
    return pt, _REFERENCES[at]


def test_the_points_are_the_ones_the_test_promises():
    assert POINTS == [(21, 11, 0), (31, 7, 0), (31, 21, 17), (31, 27, 0), (33, 13, 0), (47, 15, 31), (63, 25, 12), (63, 31, 0)]
    assert set(POINTS) <= set(WALKS_POINTS["packed"]) and SK_INLINE_MAX == 4 and SHARDS == 3 and FLOOR == 8
    assert DENSITIES == {"default": ((2.5, 1.75), (3.0, 2.5)), "compact": ((1.6, 1.35), (2.0, 1.75)), "packed": ((1.2, 1.2), (1.2, 1.2))}


@pytest.mark.parametrize("point,recorded", list(zip(WALKS_POINTS["packed"], RECORDED_HEAVY_KMERS)), ids=[case_id(*p) for p in WALKS_POINTS["packed"]])
def test_the_reference_reproduces_the_recorded_heavy_kmers(point, recorded, tools, tmp_path):
    """the walks' own dictionaries (nothing planted for the table): what an MI355X counted is what the rules give"""
    k, m, key_length = point
    pt = make_inputs(k, m, key_length, False, tools[0], str(tmp_path), extend=extension_of(k, m, key_length, "packed", tools[0]))
    ref = Reference(pt.sequences, k, key_length or key_length_of(k, m), *tools)
    assert ref.sk_heavy_kmers == recorded, (point, ref.sk_heavy_kmers, recorded)
    assert ref.items == ref.key_items + ref.sk_heavy_kmers and sum(ref.histogram[9:]) == ref.tuples and sum(ref.histogram[:9]) == ref.sk_keys


# ---- a sequential placer -------------------------------------------------------------------------------------------------------------------
def _body_words(ref, first_base, n_bases):
    """(n, n_bases / 16) uint32: the bases of the collection from first_base on, 16 a word, zero outside it"""
    where = first_base[:, None] + np.arange(n_bases)[None, :]
    inside = (where >= 0) & (where < ref.num_bases)
    codes = np.where(inside, ref.bases[np.clip(where, 0, ref.num_bases - 1)], 0).astype(np.uint32)
    return (codes.reshape(codes.shape[0], n_bases // 16, 16) << (2 * np.arange(16, dtype=np.uint32))).sum(axis=2, dtype=np.uint32)


def inline_slot(ref, p, strand, fingerprint):
    """the slots of inline occurrences, written down from device_layout.hpp (5) and not from the verifier: (n, 8 W) uint32"""
    k, L, W = ref.k, ref.L, ref.W
    km = k - L
    sid = np.searchsorted(ref.offsets, p, side="right") - 1
    left, right = np.minimum(p - ref.offsets[sid], km), np.minimum(ref.offsets[sid + 1] - (p + L), km)
    out = np.zeros((p.size, 8 * W), dtype=np.uint32)
    out[:, 0] = SK_VALID | (strand * SK_STRAND) | (left << SK_LEFT_SHIFT) | (right << SK_RIGHT_SHIFT)
    out[:, 1] = sid
    out[:, 2] = p & 0xFFFFFFFF
    out[:, 3] = (p >> 32) | (fingerprint << 8)
    out[:, 4:4 + 4 * W] = _body_words(ref, p - km, 64 * W)
    return out


class Placed:
    pass


def place(ref, key_buckets, kmer_buckets, seed):
    """the reference's items, first fit in choice order, one after the other in a shuffled order -> the table and where everything went"""
    W = ref.W
    SW = 8 * W
    t = Placed()
    t.key_buckets, t.kmer_buckets, t.SW = key_buckets, kmer_buckets, SW
    t.words = np.zeros(key_buckets * 2 * SW + kmer_buckets * 16, dtype=np.uint32)
    K, R = t.keys_region(), t.kmers_region()
    inline_h, marker_h, heavy_h = ref.choices(key_buckets, kmer_buckets)
    I, H = ref.inline, ref.heavy
    slots = inline_slot(ref, I.p, I.strand, inline_h[:, 5])
    markers = np.zeros((ref.markers.n, SW), dtype=np.uint32)
    markers[:, 0] = SK_VALID | SK_MARKER
    markers[:, 3] = marker_h[:, 5] << 8
    rng = np.random.default_rng(seed)
    used = unplaced = 0
    t.inline_at, t.marker_at, t.kmer_at = [], [], []  # (item, bucket, slot)
    order = [(0, int(i)) for i in np.repeat(np.arange(I.n), I.mult)] + [(1, j) for j in range(ref.markers.n)]
    fill = [0] * key_buckets
    for kind, i in [order[int(x)] for x in rng.permutation(len(order))]:
        h = (marker_h if kind else inline_h)[i]
        for c in range(5):
            b = int(h[c])
            if fill[b] < 2:
                s = fill[b]
                fill[b] += 1
                row = (markers if kind else slots)[i]
                K[b, s, 0] |= row[0]
                K[b, s, 1:] = row[1:]
                if s == 1:
                    K[b, 0, 0] |= SK_SECOND_USED
                    if W == 2:
                        K[b, 0, SK_SECOND_FINGERPRINT_WORD] = h[5]
                (t.marker_at if kind else t.inline_at).append((i, b, s))
                used += 1
                break
            K[b, 0, 0] |= (SK_GO_ON << c) | ((1 << (SK_FILTER_SHIFT + int(h[6]))) if c == 0 else 0)
        else:
            unplaced += 1
    if kmer_buckets:
        per = 3 if W == 1 else 2
        if W == 1:
            lo, hi = (H.kmer[:, 0] & np.uint64(0xFFFFFFFF)).astype(np.int64), (H.kmer[:, 0] >> np.uint64(32)).astype(np.int64)
            entries = np.stack([lo, hi, H.start & 0xFFFFFFFF, H.sid, H.start >> 32], axis=1).astype(np.uint32)
        else:
            entries = np.zeros((H.n, 8), dtype=np.uint32)
            entries[:, 0], entries[:, 1], entries[:, 2], entries[:, 3] = SK_VALID, H.sid, H.start & 0xFFFFFFFF, (H.start >> 32) | (heavy_h[:, 5] << 8)
            entries[:, 4:8] = np.ascontiguousarray(H.kmer).view(np.uint32).reshape(H.n, 4)
        fill = [0] * kmer_buckets
        order = np.repeat(np.arange(H.n), H.mult)
        for i in order[rng.permutation(order.size)]:
            h = heavy_h[i]
            for c in range(5):
                b = int(h[c])
                if fill[b] < per:
                    e = fill[b]
                    fill[b] += 1
                    if W == 1:
                        R[b, 0] |= 1 << e
                        R[b, 1 + 5 * e:6 + 5 * e] = entries[i]
                    else:
                        R[b, 8 * e] |= entries[i, 0]
                        R[b, 8 * e + 1:8 * e + 8] = entries[i, 1:]
                        if e == 1:
                            R[b, 0] |= SK_SECOND_USED
                    t.kmer_at.append((int(i), b, e))
                    used += 1
                    break
                R[b, 0] |= (SK_GO_ON << c) | ((1 << (SK_FILTER_SHIFT + int(h[6]))) if c == 0 else 0)
            else:
                unplaced += 1
    t.stats = {"sk_slots_used": used, "sk_deferred_keys": unplaced}
    return t


def _keys_region(self):
    return self.words[:self.key_buckets * 2 * self.SW].reshape(self.key_buckets, 2, self.SW)


def _kmers_region(self):
    return self.words[self.key_buckets * 2 * self.SW:].reshape(self.kmer_buckets, 16)


def _copy(self):
    other = Placed()
    other.__dict__.update(self.__dict__)
    other.words = self.words.copy()
    return other


Placed.keys_region, Placed.kmers_region, Placed.copy = _keys_region, _kmers_region, _copy


def info_for(ref, t):
    return {"bytes": 4 * t.words.size, "key_buckets": t.key_buckets, "kmer_buckets": t.kmer_buckets, "key_bucket_bytes": 8 * t.SW, "kmer_bucket_bytes": 64,
            "key_length": ref.L, "table_shards": ref.shards, "table_shard_id": ref.shard_id}


# ---- the corruptions: each changes one place of a copy -> (the kinds verify() must name, the region, the bucket or None) -------------------
def _free_slot(t, bucket):
    K = t.keys_region()
    return next((s for s in (0, 1) if not K[bucket, s, 0] & SK_VALID), None)


def go_on_cleared(t, ref):
    K = t.keys_region()
    b = int(np.flatnonzero(K[:, 0, 0] & (31 << 3))[0])
    K[b, 0, 0] &= ~np.uint32(int(K[b, 0, 0]) & (31 << 3) & -(int(K[b, 0, 0]) & (31 << 3)))  # its lowest go-on bit
    return {"go-on missing"}, "keys", b


def go_on_set_where_nobody_left(t, ref):
    K = t.keys_region()
    full = ((K[:, 0, 0] & SK_VALID) != 0) & ((K[:, 1, 0] & SK_VALID) != 0)
    b = int(np.flatnonzero(full & ((K[:, 0, 0] & SK_GO_ON) == 0))[0])
    K[b, 0, 0] |= SK_GO_ON
    return {"go-on spurious"}, "keys", b


def filter_bit_moved(t, ref):
    K = t.keys_region()
    b = int(np.flatnonzero(K[:, 0, 0] >> SK_FILTER_SHIFT)[0])
    bits = int(K[b, 0, 0]) >> SK_FILTER_SHIFT
    i = (bits & -bits).bit_length() - 1
    j = next(x for x in range(SK_FILTER_BITS) if not (bits >> x) & 1)
    K[b, 0, 0] = (int(K[b, 0, 0]) & ~(1 << (SK_FILTER_SHIFT + i))) | (1 << (SK_FILTER_SHIFT + j))
    return {"filter missing", "filter spurious"}, "keys", b


def _an_inline(t, n=0):
    return t.inline_at[n * 7 % len(t.inline_at)]


def left_one_more(t, ref):
    i, b, s = next(x for x in t.inline_at if ref.inline.left[x[0]] < ref.k - ref.L)  # (an extent that the string cuts short: one more base is the neighbour's)
    t.keys_region()[b, s, 0] += 1 << SK_LEFT_SHIFT
    return {"left"}, "keys", b


def right_one_more(t, ref):
    i, b, s = next(x for x in t.inline_at if ref.inline.right[x[0]] < ref.k - ref.L)
    t.keys_region()[b, s, 0] += 1 << SK_RIGHT_SHIFT
    return {"right"}, "keys", b


def strand_flipped(t, ref):
    i, b, s = _an_inline(t, 1)
    t.keys_region()[b, s, 0] ^= SK_STRAND
    return {"strand"}, "keys", b


def second_fingerprint_changed(t, ref):
    if ref.W == 1:
        return None  # (k <= 31: slot 1 shares slot 0's line, there is no such word)
    K = t.keys_region()
    b = int(np.flatnonzero(K[:, 1, 0] & SK_VALID)[0])
    K[b, 0, SK_SECOND_FINGERPRINT_WORD] ^= 1 << 5
    return {"second fingerprint word"}, "keys", b


def item_dropped(t, ref):
    K = t.keys_region()
    i, b, s = next(x for x in t.inline_at if x[2] == 1)
    K[b, 1, :] = 0
    K[b, 0, 0] &= ~np.uint32(SK_SECOND_USED)
    if ref.W == 2:
        K[b, 0, SK_SECOND_FINGERPRINT_WORD] = 0
    return {"items present against sk_slots_used", "items absent against sk_deferred_keys", "go-on missing"}, "keys", None


def item_duplicated(t, ref):
    K = t.keys_region()
    inline_h = ref.choices(t.key_buckets, t.kmer_buckets)[0]
    for i, b, s in t.inline_at:
        for other in inline_h[i, :5]:
            other = int(other)
            free = _free_slot(t, other)
            if other != b and free is not None:
                K[other, free, 0] |= K[b, s, 0] & ~np.uint32(BUCKET_FLAGS)
                K[other, free, 1:4 + 4 * ref.W] = K[b, s, 1:4 + 4 * ref.W]
                if free == 1:
                    K[other, 0, 0] |= SK_SECOND_USED
                    if ref.W == 2:
                        K[other, 0, SK_SECOND_FINGERPRINT_WORD] = inline_h[i, 5]
                return {"item more often than the reference holds it"}, "keys", None
    raise AssertionError("no item with a free slot in another of its buckets")


def marker_for_a_key_of_four(t, ref):
    K = t.keys_region()
    inline_h, marker_h, _ = ref.choices(t.key_buckets, t.kmer_buckets)
    # (a key of four whose fingerprint is no heavy key's: at (33, 13) the walks plant a light key that shares fingerprint and bucket with a heavy one,
    # and a marker in its place reads as that key's marker a second time)
    of_four = np.isin(ref.inline.keys, ref.keys[ref.key_sizes == SK_INLINE_MAX]) & ~np.isin(inline_h[:, 5], marker_h[:, 5])
    i, b, s = next(x for x in t.inline_at if of_four[x[0]])
    fingerprint = int(K[b, s, 3]) >> 8
    K[b, s, 0] = (int(K[b, s, 0]) & BUCKET_FLAGS) | SK_VALID | SK_MARKER
    K[b, s, 1:4 + 4 * ref.W] = 0
    K[b, s, 3] = fingerprint << 8
    return {"marker of no heavy key"}, "keys", b


def inline_slot_for_a_key_of_five(t, ref):
    K = t.keys_region()
    key = ref.keys[ref.key_sizes == SK_INLINE_MAX + 1][0]
    j = int(np.flatnonzero(ref.markers.keys == key)[0])
    _, b, s = next(x for x in t.marker_at if x[0] == j)  # its marker makes room: an inline slot of one of its five tuples instead
    val = int(ref.tuple_val[ref.tuple_key == key][0])
    row = inline_slot(ref, np.array([val >> 1]), np.array([val & 1]), np.array([int(K[b, s, 3]) >> 8]))[0]
    K[b, s, 0] = (int(K[b, s, 0]) & BUCKET_FLAGS) | int(row[0])
    K[b, s, 1:] = row[1:]
    return {"inline slot for a heavy key's occurrence"}, "keys", b


def kmer_entry_position_high_bits(t, ref):
    R = t.kmers_region()
    i, b, e = t.kmer_at[len(t.kmer_at) // 2]
    if ref.W == 1:
        R[b, 1 + 5 * e + 4] |= 0x40
    else:
        R[b, 8 * e + 3] |= 0x40
    return {"k-mer entry of no heavy k-mer"}, "kmers", b


def body_base_changed(t, ref):
    i, b, s = _an_inline(t, 2)
    at = ref.k - ref.L + ref.L // 2  # a base of the key itself: inside every extent
    t.keys_region()[b, s, 4 + at // 16] ^= np.uint32(1 << (2 * (at % 16)))
    return {"body"}, "keys", b


CORRUPTIONS = [go_on_cleared, go_on_set_where_nobody_left, filter_bit_moved, left_one_more, right_one_more, strand_flipped, second_fingerprint_changed, item_dropped,
               item_duplicated, marker_for_a_key_of_four, inline_slot_for_a_key_of_five, kmer_entry_position_high_bits, body_base_changed]


# ---- the gate ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("canonical", [False, True], ids=["regular", "canonical"])
@pytest.mark.parametrize("k,m,key_length", POINTS, ids=[case_id(*p) for p in POINTS])
def test_the_inputs_reach_the_edges_and_the_verifier_passes_a_placed_table(k, m, key_length, canonical, tools, tmp_path):
    pt, ref = reference_of(k, m, key_length, canonical, tools, tmp_path)
    assert [int(x) for x in pt.case.gt.endpoints] == [int(x) for x in ref.offsets]
    got = conditions(ref)
    print(case_id(k, m, key_length), "canonical" if canonical else "regular", got)
    for density in DENSITIES:
        lay = ref.layout(density)
        stats, histogram = expected_numbers(ref, density)
        assert stats["sk_slots"] == 2 * lay["key_buckets"] + (3 if k <= 31 else 2) * lay["kmer_buckets"] and histogram[19] == ref.items and len(histogram) == 20
        t = place(ref, lay["key_buckets"], lay["kmer_buckets"], seed=k + m)
        counts = {}
        violations = verify(t.words, ref.info_of(density), ref, stats=t.stats, counts=counts)
        assert not violations, (density, len(violations), violations[:10])
        assert counts["present"] == t.stats["sk_slots_used"] and counts["absent"] == t.stats["sk_deferred_keys"] and counts["present"] + counts["absent"] == ref.items
        assert info_for(ref, t) == ref.info_of(density)
        if density == "packed":
            assert counts["absent"] > 0 and counts["past_first_choice"] > 0, counts
    if not canonical:
        parts = [Reference(pt.sequences, k, ref.L, *tools, SHARDS, s) for s in range(SHARDS)]
        shards_gate(ref, parts)
        owners = table_hashes(tools[1], ref.keys, 1, SHARDS)[:, 7]
        for s, part in enumerate(parts):
            assert (np.sort(part.keys) == ref.keys[owners == s]).all()
            lay = part.layout("default")
            t = place(part, lay["key_buckets"], lay["kmer_buckets"], seed=s)
            assert not verify(t.words, part.info_of("default"), part, stats=t.stats)


@pytest.mark.parametrize("k,m,key_length", POINTS, ids=[case_id(*p) for p in POINTS])
def test_the_verifier_names_every_corruption(k, m, key_length, tools, tmp_path):
    _, ref = reference_of(k, m, key_length, False, tools, tmp_path)
    lay = ref.layout("packed")
    clean = place(ref, lay["key_buckets"], lay["kmer_buckets"], seed=k + m)
    info = ref.info_of("packed")
    assert not verify(clean.words, info, ref, stats=clean.stats)
    named = 0
    for corrupt in CORRUPTIONS:
        t = clean.copy()
        expected = corrupt(t, ref)
        if expected is None:
            assert corrupt is second_fingerprint_changed and k <= 31
            continue
        kinds, region, bucket = expected
        assert (t.words != clean.words).any(), corrupt.__name__
        violations = verify(t.words, info, ref, stats=clean.stats)
        for kind in kinds:
            assert any(v[0] == kind and (bucket is None or (v[1], v[2]) == (region, bucket)) for v in violations), (corrupt.__name__, kind, region, bucket, violations[:8])
        named += 1
    assert named == len(CORRUPTIONS) - (1 if k <= 31 else 0)
    assert (clean.words == place(ref, lay["key_buckets"], lay["kmer_buckets"], seed=k + m).words).all(), "a corruption changed the clean table"
