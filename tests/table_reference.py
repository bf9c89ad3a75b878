"""What a replica's super-k-mer table must hold, restated in numpy from the comments of csrc/sktable.hip and csrc/device_layout.hpp (5),
and a verifier that holds an exported table (Dictionary.device_table) against it. Nothing of sktable.hip is in here. The reference works
from the dictionary's strings in stored order (their base positions on the concatenation) and from the per-k-mer records of
tests/cpp/table_keys.cpp (tie, strand, position, key). For the functions that the builder and the readers SHARE -- the bucket sequence
and the fingerprint (sk_hash), sk_filter_index, sk_kmer_key and sk_owner -- it calls a small host tool over device_layout.hpp,
tests/cpp/table_hashes.cpp, as table_keys.cpp and route_owners.cpp do (the other choice, restating them in numpy beside
gpu_walks_worker.table_hash, was not taken: tests/cpp/check_table_key.cpp already tests the header's own functions).

The rules (L = the length of the table's keys):
    occurrence   a k-mer start i inside a string that has a key (no tie; on a shard: the key is owned) elects (key, p, strand),
                 p = i + (rc ? k - L - pos : pos)
    tuples       a start whose left neighbour elects another occurrence, or none, begins a tuple (one super-k-mer); a multiset
    keys         a key with at most SK_INLINE_MAX = 4 tuples is inline, one item per tuple; a key with more is heavy: one marker
                 item, and every k-mer that elects the occurrence of one of its tuples is an item of the k-mers' region, per tuple
Which of its five buckets an item lands in depends on the order in which the build's threads arrive, so verify() checks invariants of
the layout and never bytes: every valid slot is one item of the reference in one of its buckets with every field right, no item is
there more often than the reference holds it, and the go-on flags and the first-choice filter say exactly what the items' places
require -- both ways."""
from __future__ import annotations

import subprocess

import numpy as np

from gpu_even_m_worker import kmers_of, table_keys

SK_VALID, SK_MARKER, SK_STRAND, SK_GO_ON, SK_CHOICES = 1, 2, 4, 8, 5
SK_LEFT_SHIFT, SK_RIGHT_SHIFT, SK_SECOND_USED, SK_FILTER_SHIFT, SK_FILTER_BITS = 8, 14, 1 << 20, 21, 11
SK_SECOND_FINGERPRINT_WORD, SK_INLINE_MAX = 12, 4
POSITION_MASK = (1 << 40) - 1
BINS = (1, 2, 3, 4, 8, 16, 64, 1024)  # the upper ends of the bins 1, 2, 3, 4, 5-8, 9-16, 17-64, 65-1024; above: the ninth
DENSITIES = {  # name -> ((slots per item of the keys' region, places per k-mer of the k-mers' region) at k <= 31, above)
    "default": ((2.5, 1.75), (3.0, 2.5)),
    "compact": ((1.6, 1.35), (2.0, 1.75)),
    "packed": ((1.2, 1.2), (1.2, 1.2)),
}


def table_hashes(exe, keys, num_buckets, num_shards=1):
    """-> (n, 8) uint32 per key: the five bucket choices, the fingerprint, its filter index, the owner among num_shards"""
    keys = np.ascontiguousarray(keys, dtype=np.uint64)
    p = subprocess.run([exe, "hash", str(max(1, int(num_buckets))), str(num_shards)], input=keys.tobytes(), capture_output=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    return np.frombuffer(p.stdout, dtype=np.uint32).reshape(keys.size, 8).astype(np.int64)


def kmer_keys(exe, kmers, k):
    p = subprocess.run([exe, "kmer_key", str(k)], input=np.ascontiguousarray(kmers, dtype=np.uint64).tobytes(), capture_output=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    return np.frombuffer(p.stdout, dtype=np.uint64)


class Items:
    """the items of one region: `n` distinct ones, each `mult` times"""

    def __init__(self, keys, mult):
        self.keys, self.mult, self.n = np.asarray(keys, dtype=np.uint64), np.asarray(mult, dtype=np.int64), len(keys)


class Reference:
    def __init__(self, sequences, k, key_length, keys_exe, hashes_exe, shards=1, shard_id=0):
        self.k, self.L, self.W, self.exe, self.shards, self.shard_id = k, key_length, 1 if k <= 31 else 2, hashes_exe, shards, shard_id
        W, L, km = self.W, key_length, k - key_length
        lens = np.array([len(s) for s in sequences], dtype=np.int64)
        self.offsets = np.concatenate([[0], np.cumsum(lens)])  # base positions of the strings on their concatenation
        self.num_bases = int(self.offsets[-1])
        raw = np.frombuffer("".join(sequences).encode("ascii"), dtype=np.uint8)
        self.bases = ((raw >> 1) & 3).astype(np.uint8)  # A0 C1 T2 G3
        per = lens - (k - 1)
        sid = np.repeat(np.arange(lens.size), per)
        first = np.concatenate([[0], np.cumsum(per)[:-1]])
        start = self.offsets[sid] + (np.arange(sid.size) - first[sid])  # where every k-mer starts
        self.kmers = kmers_of(sequences, k).reshape(-1, W)
        rec = table_keys(keys_exe, self.kmers, k, L)
        assert rec.size == start.size
        usable = rec["tie"] == 0
        self.all_keys = np.unique(rec["key"][usable])  # (of the whole table, whatever the shard)
        if shards > 1:
            usable &= table_hashes(hashes_exe, rec["key"], 1, shards)[:, 7] == shard_id
        rc, pos = rec["rc"].astype(np.int64), rec["pos"].astype(np.int64)
        p = start + np.where(rc == 1, km - pos, pos)
        val = np.where(usable, 2 * p + rc, -1)
        key = rec["key"]
        left_is_other = np.ones(start.size, dtype=bool)  # a string's first k-mer has no left neighbour inside a string
        inside = np.flatnonzero(start != self.offsets[sid])
        left_is_other[inside] = (val[inside - 1] != val[inside]) | (key[inside - 1] != key[inside])
        begins = usable & left_is_other
        self.kmer_start, self.kmer_sid, self.kmer_val, self.begins = start, sid, val, begins
        # ---- tuples, keys by their tuples
        t_key, t_val = key[begins], val[begins]
        self.tuples = int(t_key.size)
        self.tuple_kmers = np.bincount(np.cumsum(begins)[usable] - 1, minlength=self.tuples)  # (a k-mer with a key that begins no tuple is of its left neighbour's)
        self.string_lengths = lens
        keys, inverse, sizes = np.unique(t_key, return_inverse=True, return_counts=True)
        self.keys, self.key_sizes = keys, sizes
        heavy_key = sizes > SK_INLINE_MAX
        t_heavy = heavy_key[inverse]
        bin_of = np.searchsorted(np.array(BINS), sizes)
        self.histogram = [int(x) for x in np.bincount(bin_of, minlength=9)] + [int(x) for x in np.bincount(bin_of, weights=sizes, minlength=9)]
        # ---- the keys' region: one inline item per tuple of a light key (equal tuples: one item, as often), one marker per heavy key
        vals, one_of, mult = np.unique(t_val[~t_heavy], return_index=True, return_counts=True)
        self.inline = Items(t_key[~t_heavy][one_of], mult)  # (an occurrence is one key's: the m-mer at p on that strand)
        self.inline.p, self.inline.strand = vals >> 1, vals & 1
        s = np.searchsorted(self.offsets, self.inline.p, side="right") - 1
        self.inline.sid = s
        self.inline.left = np.minimum(self.inline.p - self.offsets[s], km)
        self.inline.right = np.minimum(self.offsets[s + 1] - (self.inline.p + L), km)
        self.markers = Items(keys[heavy_key], np.ones(int(heavy_key.sum()), dtype=np.int64))
        self.heavy_tuple_p = np.unique(t_val[t_heavy] >> 1)
        self.tuple_key, self.tuple_val, self.tuple_heavy = t_key, t_val, t_heavy
        # ---- the k-mers' region: per tuple of a heavy key, every k-mer that elects the tuple's occurrence
        hv, hmult = np.unique(t_val[t_heavy], return_counts=True)
        at = np.minimum(np.searchsorted(hv, val), max(0, hv.size - 1))
        mine = np.flatnonzero(usable & (hv[at] == val)) if hv.size else np.zeros(0, dtype=np.int64)
        self.heavy = Items(kmer_keys(hashes_exe, self.kmers[mine].reshape(-1), k) if mine.size else [], hmult[at[mine]] if mine.size else [])
        self.heavy.start, self.heavy.sid, self.heavy.kmer = start[mine], sid[mine], self.kmers[mine]
        # ---- the accounting
        self.sk_keys, self.sk_heavy_keys = int(keys.size), int(heavy_key.sum())
        self.sk_inline_keys = self.sk_keys - self.sk_heavy_keys
        self.sk_heavy_kmers = int(self.heavy.mult.sum())
        self.key_items = int(self.inline.mult.sum()) + self.sk_heavy_keys
        self.items = self.key_items + self.sk_heavy_kmers
        assert int((~t_heavy).sum()) == int(self.inline.mult.sum())
        self._choices = {}

    def layout(self, density):
        """-> what the build publishes for a density of DENSITIES: buckets of the two regions, sk_slots, sk_bytes"""
        spk, spm = DENSITIES[density][self.W - 1]
        entries = 3 if self.W == 1 else 2
        key_buckets = int(float(self.key_items) * spk / 2) + 8
        kmer_buckets = int(float(self.sk_heavy_kmers) * spm / float(entries)) + 8 if self.sk_heavy_kmers else 0
        return {"key_buckets": key_buckets, "kmer_buckets": kmer_buckets, "sk_slots": 2 * key_buckets + entries * kmer_buckets,
                "sk_bytes": key_buckets * 2 * 32 * self.W + kmer_buckets * 64}

    def info_of(self, density):
        lay = self.layout(density)
        return {"bytes": lay["sk_bytes"], "key_buckets": lay["key_buckets"], "kmer_buckets": lay["kmer_buckets"], "key_bucket_bytes": 64 * self.W,
                "kmer_bucket_bytes": 64, "key_length": self.L, "table_shards": self.shards, "table_shard_id": self.shard_id}

    def choices(self, key_buckets, kmer_buckets):
        """the bucket sequence, fingerprint and filter index of every item, for regions of that many buckets"""
        at = (key_buckets, kmer_buckets)
        if at not in self._choices:
            self._choices = {at: [table_hashes(self.exe, items.keys, n) for items, n in ((self.inline, key_buckets), (self.markers, key_buckets), (self.heavy, kmer_buckets))]}
        return self._choices[at]


# ---- the verifier ------------------------------------------------------------------------------------------------------------------------
def _unpack(words64, n_bases):
    """(n, words) uint64 -> (n, n_bases) 2-bit codes"""
    j = np.arange(n_bases)
    return ((words64[:, j // 32] >> (2 * (j % 32)).astype(np.uint64)) & np.uint64(3)).astype(np.uint8)


def _flags(say, region, n_buckets, word0, full, ch, fp_filter, mult, found_item, found_bucket):
    """go-on flags and the first-choice filter of one region, both ways. ch: (items, 5) bucket choices; found_*: one entry per slot
    that holds an item"""
    need = np.zeros((n_buckets, SK_CHOICES), dtype=bool)
    need_filter = np.zeros((n_buckets, SK_FILTER_BITS), dtype=bool)
    if ch.shape[0]:
        chosen = np.argmax(ch[found_item] == found_bucket[:, None], axis=1) if found_item.size else np.zeros(0, dtype=np.int64)
        absent = np.flatnonzero(mult - np.bincount(found_item, minlength=ch.shape[0]) > 0)
        items = np.concatenate([found_item, absent])
        upto = np.concatenate([chosen, np.full(absent.size, SK_CHOICES)])  # the choices an item left behind: 0 .. upto - 1
        for c in range(SK_CHOICES):
            gone = items[upto > c]
            need[ch[gone, c], c] = True
            if c == 0:
                need_filter[ch[gone, 0], fp_filter[gone]] = True
    have = ((word0[:, None] >> (3 + np.arange(SK_CHOICES))) & 1).astype(bool)
    have_filter = ((word0[:, None] >> (SK_FILTER_SHIFT + np.arange(SK_FILTER_BITS))) & 1).astype(bool)
    for b, c in np.argwhere(need & ~have):
        say("go-on missing", region, b, f"choice {c}: an item that went on from here, or found no slot")
    for b, c in np.argwhere(have & ~need):
        say("go-on spurious", region, b, f"choice {c}: no item went on from here")
    for b, i in np.argwhere(need_filter & ~have_filter):
        say("filter missing", region, b, f"filter bit {i}")
    for b, i in np.argwhere(have_filter & ~need_filter):
        say("filter spurious", region, b, f"filter bit {i}")
    for b in np.flatnonzero(have.any(axis=1) & ~full):
        say("go-on on a bucket that is not full", region, b, "")


def verify(words, info, ref, stats=None, counts=None):
    """-> the list of violations, (kind, region, bucket, detail) each. It reads the exported table, its info and the reference and
    nothing else; `stats` (sk_slots_used, sk_deferred_keys), where given, are held against the items present and absent; `counts`, a
    dict, receives what was counted."""
    out = []

    def say(kind, region, bucket, detail):
        out.append((kind, region, int(bucket), detail))

    k, L, W, km = ref.k, ref.L, ref.W, ref.k - ref.L
    NB, KB = info["key_buckets"], info["kmer_buckets"]
    words = np.asarray(words, dtype=np.uint32)
    SW = 8 * W
    if info["key_length"] != L or info["key_bucket_bytes"] != 8 * SW or info["kmer_bucket_bytes"] != 64 or words.size * 4 != info["bytes"] \
            or info["bytes"] != NB * 8 * SW + KB * 64:
        say("info", "table", 0, str(info))
        return out
    inline_h, marker_h, heavy_h = ref.choices(NB, KB)
    # ---- the keys' region
    S = words[:NB * 2 * SW].reshape(NB, 2, SW).astype(np.int64)
    d0 = S[:, :, 0]
    valid = (d0 & SK_VALID) != 0
    for b, s in np.argwhere(~valid & (S != 0).any(axis=2)):
        say("an invalid slot that is not zero", "keys", b, f"slot {s}")
    for b in np.flatnonzero(valid[:, 1] & ~valid[:, 0]):
        say("slot 1 valid without slot 0", "keys", b, "")
    for b in np.flatnonzero(valid[:, 1] != ((d0[:, 0] & SK_SECOND_USED) != 0)):
        say("second-used flag", "keys", b, "SK_SECOND_USED is set iff slot 1 is valid")
    own = SK_VALID | SK_MARKER | SK_STRAND | (63 << SK_LEFT_SHIFT) | (63 << SK_RIGHT_SHIFT)
    for b in np.flatnonzero(d0[:, 1] & ~own):
        say("bucket flags in slot 1", "keys", b, hex(int(d0[b, 1])))
    fp = S[:, :, 3] >> 8
    if W == 2:
        for b in np.flatnonzero(S[:, 0, SK_SECOND_FINGERPRINT_WORD] != fp[:, 1]):
            say("second fingerprint word", "keys", b, f"{int(S[b, 0, 12]):#x} against slot 1's {int(fp[b, 1]):#x}")
        for b, s in np.argwhere((S[:, :, 13:] != 0).any(axis=2) | ((S[:, :, 12] != 0) & (np.arange(2) == 1)[None, :])):
            say("spare words", "keys", b, f"slot {s}")
    bucket, slot = np.nonzero(valid)
    f0, sid = d0[bucket, slot], S[bucket, slot, 1]
    pos = S[bucket, slot, 2] | ((S[bucket, slot, 3] & 0xFF) << 32)
    fps = fp[bucket, slot]
    body = np.ascontiguousarray(S[bucket, slot, 4:4 + 4 * W].astype(np.uint32)).view(np.uint64).reshape(-1, 2 * W)
    strand, left, right = (f0 >> 2) & 1, (f0 >> SK_LEFT_SHIFT) & 63, (f0 >> SK_RIGHT_SHIFT) & 63
    is_marker = (f0 & SK_MARKER) != 0
    found_inline, found_inline_bucket, found_marker, found_marker_bucket = [], [], [], []
    # markers
    taken = np.zeros(ref.markers.n, dtype=np.int64)
    for j in np.flatnonzero(is_marker):
        b = int(bucket[j])
        if strand[j] or left[j] or right[j] or sid[j] or pos[j] or body[j].any():
            say("marker slot", "keys", b, f"slot {slot[j]}: flags, string id, position and body of a marker are zero")
        cand = np.flatnonzero((marker_h[:, 5] == fps[j]) & (marker_h[:, :5] == b).any(axis=1)) if ref.markers.n else np.zeros(0, dtype=np.int64)
        cand = [c for c in cand if taken[c] == 0] or list(cand)
        if not cand:
            say("marker of no heavy key", "keys", b, f"slot {slot[j]}, fingerprint {int(fps[j]):#x}")
            continue
        taken[cand[0]] += 1
        found_marker.append(cand[0])
        found_marker_bucket.append(b)
    for c in np.flatnonzero(taken > 1):
        say("item more often than the reference holds it", "keys", int(marker_h[c, 0]), f"the marker of key {int(ref.markers.keys[c]):#x}")
    # inline slots
    I = ref.inline
    j = np.flatnonzero(~is_marker)
    at = np.minimum(np.searchsorted(I.p, pos[j]), max(0, I.n - 1))
    known = (I.p[at] == pos[j]) if I.n else np.zeros(j.size, dtype=bool)
    for x in j[~known]:
        heavy = bool(np.isin(pos[x], ref.heavy_tuple_p))
        say("inline slot for a heavy key's occurrence" if heavy else "inline slot of no item", "keys", bucket[x], f"slot {slot[x]}, position {int(pos[x])}")
    j, at = j[known], at[known]
    b = bucket[j]
    for kind, bad in (("item in a bucket that is none of its choices", ~(inline_h[at, :5] == b[:, None]).any(axis=1)), ("fingerprint", inline_h[at, 5] != fps[j]),
                      ("strand", I.strand[at] != strand[j]), ("left", I.left[at] != left[j]), ("right", I.right[at] != right[j]), ("string id", I.sid[at] != sid[j])):
        for x in np.flatnonzero(bad):
            say(kind, "keys", b[x], f"slot {slot[j[x]]}, position {int(pos[j[x]])}")
    n_body = 64 * W
    where = (I.p[at] - km)[:, None] + np.arange(n_body)[None, :]  # the base of the collection that each base of the body holds
    padded = np.concatenate([ref.bases, np.zeros(n_body, dtype=np.uint8)])
    want = np.where(where >= 0, padded[np.clip(where, 0, ref.num_bases + n_body - 1)], 0)
    got = _unpack(body[j], n_body)
    compared = (where < 0) | ((where >= (I.p[at] - I.left[at])[:, None]) & (where < (I.p[at] + L + I.right[at])[:, None]))
    for x in np.flatnonzero(((want != got) & compared).any(axis=1)):
        say("body", "keys", b[x], f"slot {slot[j[x]]}, position {int(pos[j[x]])}, body bases {np.flatnonzero((want[x] != got[x]) & compared[x])[:4].tolist()}")
    ok = (inline_h[at, :5] == b[:, None]).any(axis=1)
    found_inline, found_inline_bucket = at[ok], b[ok]
    over = np.flatnonzero(np.bincount(found_inline, minlength=I.n) > I.mult) if I.n else []
    for c in over:
        say("item more often than the reference holds it", "keys", int(found_inline_bucket[found_inline == c][-1]), f"the occurrence at {int(I.p[c])}")
    # flags of the keys' region: inline items and markers together
    ch = np.concatenate([inline_h, marker_h])
    items = np.concatenate([found_inline, np.array(found_marker, dtype=np.int64) + I.n]).astype(np.int64)
    buckets = np.concatenate([found_inline_bucket, np.array(found_marker_bucket, dtype=np.int64)]).astype(np.int64)
    _flags(say, "keys", NB, d0[:, 0], valid.all(axis=1), ch[:, :5], ch[:, 6], np.concatenate([I.mult, ref.markers.mult]), items, buckets)
    present = int(valid.sum())
    past_first = int((ch[items, 0] != buckets).sum())
    second = int(valid[:, 1].sum())
    # ---- the k-mers' region
    H = ref.heavy
    if KB:
        R = words[NB * 2 * SW:].reshape(KB, 16).astype(np.int64)
        w0 = R[:, 0]
        if W == 1:
            in_use = w0 & 7
            for b in np.flatnonzero(~np.isin(in_use, (0, 1, 3, 7))):
                say("in-use bits are no prefix", "kmers", b, str(int(in_use[b])))
            for b in np.flatnonzero((w0 >> 8) & 0x1FFF):
                say("bits 8-20 of the flag word", "kmers", b, hex(int(w0[b])))
            E = R[:, 1:].reshape(KB, 3, 5)
            used = ((in_use[:, None] >> np.arange(3)) & 1).astype(bool)
            for b, e in np.argwhere(~used & (E != 0).any(axis=2)):
                say("an unused entry that is not zero", "kmers", b, f"entry {e}")
            bucket, entry = np.nonzero(used)
            e = E[bucket, entry]
            kmer = (e[:, 0] | (e[:, 1] << 32)).astype(np.uint64).reshape(-1, 1)
            start, esid, efp = e[:, 2] | (e[:, 4] << 32), e[:, 3], None
            full = in_use == 7
            second += int(used[:, 1:].sum())
        else:
            E = R.reshape(KB, 2, 8)
            e0 = E[:, :, 0]
            used = (e0 & SK_VALID) != 0
            for b, e in np.argwhere(~used & (E != 0).any(axis=2)):
                say("an unused entry that is not zero", "kmers", b, f"entry {e}")
            for b in np.flatnonzero(used[:, 1] & ~used[:, 0]):
                say("entry 1 used without entry 0", "kmers", b, "")
            for b in np.flatnonzero(used[:, 1] != ((e0[:, 0] & SK_SECOND_USED) != 0)):
                say("second-used flag", "kmers", b, "")
            for b in np.flatnonzero((e0[:, 0] & (SK_MARKER | SK_STRAND | (0xFFF << 8))) | (e0[:, 1] & ~SK_VALID)):
                say("entry flags", "kmers", b, f"{int(e0[b, 0]):#x} {int(e0[b, 1]):#x}")
            bucket, entry = np.nonzero(used)
            e = E[bucket, entry]
            start, esid, efp = e[:, 2] | ((e[:, 3] & 0xFF) << 32), e[:, 1], e[:, 3] >> 8
            kmer = np.ascontiguousarray(e[:, 4:8].astype(np.uint32)).view(np.uint64).reshape(-1, 2)
            full = used.all(axis=1)
            second += int(used[:, 1].sum())
        order = np.argsort(H.start, kind="stable")
        at = np.minimum(np.searchsorted(H.start[order], start), max(0, H.n - 1))
        at = order[at] if H.n else at
        known = (H.start[at] == start) if H.n else np.zeros(start.size, dtype=bool)
        for x in np.flatnonzero(~known):
            say("k-mer entry of no heavy k-mer", "kmers", bucket[x], f"entry {entry[x]}, start {int(start[x])}")
        bucket, entry, start, esid, kmer, at = bucket[known], entry[known], start[known], esid[known], kmer[known], at[known]
        checks = [("item in a bucket that is none of its choices", ~(heavy_h[at, :5] == bucket[:, None]).any(axis=1)), ("string id", H.sid[at] != esid),
                  ("k-mer", (H.kmer[at] != kmer).any(axis=1))]
        if efp is not None:
            checks.append(("fingerprint", heavy_h[at, 5] != efp[known]))
        for kind, bad in checks:
            for x in np.flatnonzero(bad):
                say(kind, "kmers", bucket[x], f"entry {entry[x]}, start {int(start[x])}")
        ok = (heavy_h[at, :5] == bucket[:, None]).any(axis=1)
        for c in (np.flatnonzero(np.bincount(at[ok], minlength=H.n) > H.mult) if H.n else []):
            say("item more often than the reference holds it", "kmers", int(bucket[ok][at[ok] == c][-1]), f"the k-mer at {int(H.start[c])}")
        _flags(say, "kmers", KB, w0, full, heavy_h[:, :5], heavy_h[:, 6], H.mult, at[ok], bucket[ok])
        present += int(used.sum())
        past_first += int((heavy_h[at[ok], 0] != bucket[ok]).sum())
    elif H.n:
        say("info", "table", 0, "heavy k-mers and no k-mers' region")
    absent = ref.items - present
    if stats is not None:
        if present != stats["sk_slots_used"]:
            say("items present against sk_slots_used", "table", 0, f"{present} against {stats['sk_slots_used']}")
        if absent != stats["sk_deferred_keys"]:
            say("items absent against sk_deferred_keys", "table", 0, f"{absent} against {stats['sk_deferred_keys']}")
    if counts is not None:
        counts.update({"present": present, "absent": absent, "past_first_choice": past_first, "in_slot_1_or_a_later_entry": second})
    return out
