#!/usr/bin/env python
"""Worker of tests/test_gpu_graph.py, and the input generator and ground truth it shares with tests/test_graph_inputs.py: the dictionary
as a graph -- string_neighbours on the device, the links between strings as CSR, the adjacency of every k-mer of an id range, the GFA --
at one k, m = min(k, 13), regular then canonical; or, as `salmonella`, on the stitched strings of the golden fixture.

make_graph() builds about 9 000 strings whose links are known by construction: a genome cut into overlapping pieces (every third stored
reverse-complemented; stretches of single-k-mer pieces, one at the very end), bubbles whose branch point lies at a piece end or inside
a long piece, a circular string, a hairpin, an isolated string. truth() is the ground truth: a plain Python dict from canonical k-mer to
(string, position, strand), asked for the eight neighbours of every k-mer; expected_links(), expected_masks() and
expected_string_neighbours() read the library's outputs off it. All comparisons are exact. Prints one JSON line; any mismatch is an
assertion error.

    python tests/gpu_graph_worker.py <k | salmonella> <scratch dir>"""
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

KS = (15, 31, 33, 63)
INVALID = 0xFFFFFFFFFFFFFFFF
SENTINEL = 0x5A5A5A5A5A5A5A5A
SCAN_TILE = 4096  # SCAN_TILE of csrc/streaming.hip: the prefix sum over link_offsets works in tiles of so many words
LINKS_CHUNKS = (None, 1, 7, 256, -1)  # links_chunk: unset, ..., and (-1) num_strings - 1
ADJACENCY_CHUNKS = (None, 1, 2047, 2049, -1)  # adjacency_chunk: unset, ..., and (-1) num_kmers - 1
SINGLES_IN_A_ROW, SINGLES_AT_THE_END = 5, 40
_COMP = str.maketrans("ACGT", "TGCA")
U64_FIELDS = ("kmer_id", "kmer_id_in_string", "kmer_offset", "string_id", "string_begin", "string_end")


def m_of(k):
    return min(k, 13)


def revcomp(s):
    return s.translate(_COMP)[::-1]


# ---- the dictionary's strings ------------------------------------------------------------------------------------------------------------
def make_graph(k, seed):
    """-> (strings, what): the strings in dictionary order -- bubbles, the circular string, the hairpin, the isolated string, then the
    chain, so that the dictionary ends inside a stretch of single-k-mer pieces -- and `what`, where the cases lie (string ids)"""
    from conftest import random_dna
    from gpu_forms_worker import _adder, canonical_strings

    rng = np.random.default_rng(seed)
    # sizes of the chain's pieces, in k-mers: 1 in stretches of 5, 2, k (the piece a bubble at a piece end runs beside), ragged
    n_ragged = 27000 // (5 * k // 2)
    body = [[1] * SINGLES_IN_A_ROW] * 700 + [[2]] * 1800 + [[1]] * 3000 + [[2, k]] * 60 + [[int(x)] for x in rng.integers(1, 5 * k + 1, n_ragged)] + [[3 * k + 9]] * 40
    order = rng.permutation(len(body))
    sizes = [3 * k] + [s for i in order for s in body[i]] + [4] + [1] * SINGLES_AT_THE_END  # (a tip of 3k k-mers, ..., the other tip: the last single)
    total = sum(sizes) + k - 1  # bases of the genome
    while True:
        genome = random_dna(rng, total)
        if len(canonical_strings(genome, k)) == total - k + 1:  # (at k = 15 random k-mers collide)
            break
    chain, at, begins = [], 0, []
    for j, size in enumerate(sizes):
        piece = genome[at:at + size + k - 1]  # overlaps the next piece by k - 1 bases
        begins.append(at)
        chain.append(revcomp(piece) if j % 3 == 2 else piece)
        at += size
    assert at + k - 1 == total

    pool = list(chain)
    add = _adder(pool, k)

    def snp(p):  # the k k-mers that hold base p of the genome, with another base there
        return genome[p - k + 1:p] + "ACGT"[("ACGT".index(genome[p]) + 1 + int(rng.integers(0, 3))) % 4] + genome[p + 1:p + k]

    at_piece_end, inside, at_the_other_end = [], [], []
    for j in range(1, len(sizes) - 1):
        if sizes[j] > 2 and sizes[j] not in (k, 3 * k + 9) and len(at_the_other_end) < 60:
            # the bubble's far side lands on the LAST k-mer of piece j, coming from the left: a link to a string end that is not end-to-end
            t = snp(begins[j] + sizes[j] - 2)
            if add(revcomp(t) if len(at_the_other_end) % 2 else t):
                at_the_other_end.append(j)
            continue
        if sizes[j] == k and sizes[j - 1] == 2:  # base p = the first base behind piece j - 1: piece j holds exactly the k-mers over it
            t = snp(begins[j] + k - 1)
            if add(revcomp(t) if len(at_piece_end) % 2 else t):
                at_piece_end.append(j)
        elif sizes[j] == 3 * k + 9:  # base p deep inside piece j: both k-mers beside the bubble are interior to it
            t = snp(begins[j] + 2 * k + 3)
            if add(revcomp(t) if len(inside) % 2 else t):
                inside.append(j)
    n_bubbles = len(pool) - len(chain)
    while True:  # circular: C + C[:k - 1]
        c = random_dna(rng, 2 * k + 3)
        if add(c + c[:k - 1]):
            break
    while True:  # hairpin: ... a + u + rc(u), the last k-mer's forward neighbour comp(a) is that k-mer reversed
        u = random_dna(rng, (k - 1) // 2)
        if add(random_dna(rng, k + 5) + u + revcomp(u)):
            break
    while not add(random_dna(rng, 2 * k)):  # isolated
        pass
    others = pool[len(chain):]
    first_of_chain = len(others)
    what = SimpleNamespace(bubbles=n_bubbles, loop=n_bubbles, hairpin=n_bubbles + 1, isolated=n_bubbles + 2, first_of_chain=first_of_chain,
                           pieces_beside_bubbles=[first_of_chain + j for j in at_piece_end], pieces_around_bubbles=[first_of_chain + j for j in inside],
                           singles_at_the_end=SINGLES_AT_THE_END)
    assert len(at_piece_end) >= 20 and len(inside) >= 20
    return others + chain, what


# ---- ground truth ------------------------------------------------------------------------------------------------------------------------
def truth(strings, k):
    """a dict from canonical k-mer to (string, position, stored as the canonical strand), asked for the eight neighbours of EVERY k-mer
    -> first (first k-mer id of every string, num_kmers behind them), begin (first base of every string, num_bases behind them),
    nb_id / nb_ori ((num_kmers, 8): the neighbour's id or -1, its orientation +1 / -1 or 0), `where`"""
    where = {}
    for s, t in enumerate(strings):
        for p in range(len(t) - k + 1):
            x = t[p:p + k]
            r = revcomp(x)
            assert min(x, r) not in where
            where[min(x, r)] = (s, p, x < r)
    first = np.concatenate([[0], np.cumsum([len(t) - k + 1 for t in strings])]).astype(np.int64)
    begin = np.concatenate([[0], np.cumsum([len(t) for t in strings])]).astype(np.int64)
    n = int(first[-1])
    nb_id, nb_ori = np.full((n, 8), -1, dtype=np.int64), np.zeros((n, 8), dtype=np.int8)
    for s, t in enumerate(strings):
        for p in range(len(t) - k + 1):
            x = t[p:p + k]
            for which in range(8):
                q = x[1:] + "ACTG"[which] if which < 4 else "ACTG"[which - 4] + x[:-1]
                r = revcomp(q)
                hit = where.get(min(q, r))
                if hit:
                    nb_id[first[s] + p, which] = first[hit[0]] + hit[1]
                    nb_ori[first[s] + p, which] = 1 if (q < r) == hit[2] else -1
    return SimpleNamespace(k=k, first=first, begin=begin, nb_id=nb_id, nb_ori=nb_ori, where=where, num_strings=len(strings), num_kmers=n)


def _found(T, both_strands):
    return T.nb_ori != 0 if both_strands else T.nb_ori == 1


def end_rows(T, sids):
    """(len(sids), 8) ids into nb_id / nb_ori: columns 0-3 the row of the string's last k-mer, 4-7 of its first"""
    sids = np.asarray(sids, dtype=np.int64)
    return np.concatenate([np.repeat((T.first[sids + 1] - 1)[:, None], 4, 1), np.repeat(T.first[sids][:, None], 4, 1)], 1)


def expected_string_neighbours(T, sids, both_strands):
    """every field of the eight lookups of the strings `sids` (all below num_strings) that the strings alone decide -> dict of flat arrays;
    kmer_orientation is given for the found ones only (0 elsewhere)"""
    rows, cols = end_rows(T, sids), np.arange(8)[None, :]
    found = _found(T, both_strands)[rows, cols].reshape(-1)
    ids = T.nb_id[rows, cols].reshape(-1)
    string = np.searchsorted(T.first, np.where(found, ids, 0), "right") - 1
    out = {"kmer_id": ids, "kmer_id_in_string": ids - T.first[string], "kmer_offset": ids - T.first[string] + T.begin[string], "string_id": string,
           "string_begin": T.begin[string], "string_end": T.begin[string + 1]}
    out = {f: np.where(found, v, -1).astype(np.int64).view(np.uint64) for f, v in out.items()}
    out["kmer_orientation"] = np.where(found, T.nb_ori[rows, cols].reshape(-1), 0).astype(np.int8)
    out["found"] = found
    return out


def expected_links(T, begin, end, both_strands):
    """-> (link_offsets, links) of the strings [begin, end) as sshash_string_links lays them out"""
    import sshash_amd

    sids = np.arange(begin, end, dtype=np.int64)
    e = expected_string_neighbours(T, sids, both_strands)
    found = e["found"].reshape(-1, 8)
    offsets = np.concatenate([[0], np.cumsum(found.sum(1))]).astype(np.uint64)
    at = np.flatnonzero(e["found"])
    links = np.zeros(at.size, dtype=sshash_amd.LINK_DTYPE)
    to = e["string_id"][at].astype(np.int64)
    in_string = e["kmer_id_in_string"][at].astype(np.int64)
    links["from_string"] = sids[at // 8]
    links["to_string"] = to
    links["to_kmer_id"] = e["kmer_id"][at]
    links["flags"] = (at % 8) | ((e["kmer_orientation"][at] < 0) << 3) | ((in_string == 0) << 4) | ((in_string == T.first[to + 1] - T.first[to] - 1) << 5)
    return offsets, links


def expected_masks(T, both_strands):
    return (_found(T, both_strands).astype(np.uint8) << np.arange(8, dtype=np.uint8)[None, :]).sum(1).astype(np.uint8)


def link_cases(T, what, both_strands=True):
    """what the fixture's links reach (tests/test_graph_inputs.py asserts each) -> counts"""
    import sshash_amd

    offsets, links = expected_links(T, 0, T.num_strings, both_strands)
    flags = links["flags"]
    end_to_end, from_sign, to_sign = sshash_amd.links_gfa(links)
    at_end, at_start = sshash_amd.link_degrees(offsets, links)
    loop = links[(links["from_string"] == what.loop) & (links["to_string"] == what.loop)]
    hairpin = links[(links["from_string"] == what.hairpin) & (links["to_string"] == what.hairpin)]
    return dict(strings=T.num_strings, kmers=T.num_kmers, links=int(links.size), combinations=sorted({int(f >> 2) for f in flags}),
                interior_targets=int(((flags & 48) == 0).sum()), end_to_end=int(end_to_end.sum()), ends_of_degree_2=int((at_end == 2).sum() + (at_start == 2).sum()),
                signs=sorted({(a + b).decode() for a, b in zip(from_sign[end_to_end], to_sign[end_to_end])}),
                loop_links=sorted(int(f) & 60 for f in loop["flags"]), hairpin_links=sorted(int(f) & 60 for f in hairpin["flags"]),
                strings_without_links=int((np.diff(offsets) == 0).sum()), isolated_has_no_links=bool(offsets[what.isolated] == offsets[what.isolated + 1]))


def sub_ranges(T, what):
    """ranges of strings: empty, one string, the first, the last, ranges that start around a tile edge of the prefix sum, one that ends inside
    the final stretch of single-k-mer strings"""
    n = T.num_strings
    assert n > 2 * SCAN_TILE + 100 and (np.diff(T.first)[-what.singles_at_the_end:] == 1).all()
    return [(0, 0), (n, n), (5, 5), (7, 8), (0, 1), (n - 1, n), (SCAN_TILE - 1, 2 * SCAN_TILE + 3), (SCAN_TILE, SCAN_TILE + 1), (SCAN_TILE + 1, n),
            (what.loop, what.isolated + 1), (n - what.singles_at_the_end - 50, n - what.singles_at_the_end // 2)]


def adjacency_ranges(T, what):
    """id ranges at the edges of the single-k-mer stretches: the final one, and the first stretch of the chain"""
    n, sizes = T.num_kmers, np.diff(T.first)
    run = next(s for s in range(what.first_of_chain, T.num_strings - 5) if (sizes[s:s + SINGLES_IN_A_ROW] == 1).all() and sizes[s - 1] > 1)
    a, e = int(T.first[run]), int(T.first[run + SINGLES_IN_A_ROW])
    z = n - what.singles_at_the_end
    return [(0, 0), (n, n), (0, 1), (n - 1, n), (a - 1, e + 1), (a, e), (a + 1, e - 1), (z - 3, n), (z, n), (z + 1, n - 1), (2047, 4097)]


def chunk_of(n, setting):
    return n - 1 if setting == -1 else setting


# ---- the ground truth of a dictionary of one-word k-mers too large for a Python dict (the golden fixture): a sorted array ----------------------
def truth_packed(gt, k, rows):
    """GroundTruth (input order, numpy) -> the nb_id / nb_ori of the k-mer ids `rows`, by binary search over the sorted canonical k-mers"""
    from oracle.ground_truth import _revcomp_u64

    assert k <= 31
    n = gt.num_kmers
    x = gt.kmers(np.arange(n, dtype=np.uint64))
    r = _revcomp_u64(x, k)
    canon = np.minimum(x, r)
    order = np.argsort(canon, kind="stable")
    keys, stored_canonical = canon[order], (x <= r)[order]
    assert (keys[1:] != keys[:-1]).all()
    rows = np.asarray(rows, dtype=np.int64)
    nb_id, nb_ori = np.full((rows.size, 8), -1, dtype=np.int64), np.zeros((rows.size, 8), dtype=np.int8)
    mask = np.uint64((1 << (2 * k)) - 1)
    for which in range(8):
        c = np.uint64(which & 3)
        q = (x[rows] >> np.uint64(2)) | (c << np.uint64(2 * (k - 1))) if which < 4 else ((x[rows] << np.uint64(2)) & mask) | c
        qr = _revcomp_u64(q, k)
        qc = np.minimum(q, qr)
        at = np.minimum(np.searchsorted(keys, qc), n - 1)
        hit = keys[at] == qc
        nb_id[:, which] = np.where(hit, order[at], -1)
        nb_ori[:, which] = np.where(hit, np.where((q <= qr) == stored_canonical[at], 1, -1), 0)
    return nb_id, nb_ori


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


def _stream():
    import torch

    return torch.cuda.current_stream().cuda_stream


def links_on_device(d, begin, end, capacity, both_strands=True, margin=64):
    """string_links_device into sentinel-filled arrays -> (link_offsets, the `capacity` records, whether everything around them is untouched)"""
    import torch

    import sshash_amd

    n = end - begin
    off = torch.full((n + 1 + 2 * margin,), SENTINEL, dtype=torch.int64, device="cuda")
    rec = torch.full((4 * (capacity + 2 * margin),), SENTINEL, dtype=torch.int64, device="cuda")
    d.string_links_device(0, begin, end, off.data_ptr() + 8 * margin, rec.data_ptr() + 32 * margin if capacity else 0, capacity,
                          check_reverse_complement=both_strands, stream=_stream())
    torch.cuda.synchronize()
    h_off, h_rec = off.cpu().numpy().view(np.uint64), rec.cpu().numpy().view(np.uint64)
    untouched = bool((h_off[:margin] == SENTINEL).all() and (h_off[-margin:] == SENTINEL).all() and (h_rec[:4 * margin] == SENTINEL).all() and (h_rec[4 * (margin + capacity):] == SENTINEL).all())
    return h_off[margin:-margin].copy(), h_rec[4 * margin:4 * (margin + capacity)].copy().view(sshash_amd.LINK_DTYPE), untouched


def adjacency_on_device(d, begin, end, both_strands=True, margin=256):
    import torch

    out = torch.full((end - begin + 2 * margin,), 0xA5, dtype=torch.uint8, device="cuda")
    d.kmer_adjacency_device(0, begin, end, out.data_ptr() + margin if end > begin else 0, check_reverse_complement=both_strands, stream=_stream())
    torch.cuda.synchronize()
    h = out.cpu().numpy()
    return h[margin:h.size - margin].copy(), bool((h[:margin] == 0xA5).all() and (h[h.size - margin:] == 0xA5).all())


def check_string_neighbours(T, d, canonical, what):
    import torch

    n = T.num_strings
    rng = np.random.default_rng(T.k)
    sids = rng.permutation(n).astype(np.uint64)
    host = d.string_neighbours(sids)
    # the ids form: shuffled ids and one id past the end, ids only; against the host's string_neighbours
    with_one_past = np.concatenate([sids[:1000], [n], sids[1000:]]).astype(np.uint64)
    d_ids = torch.from_numpy(with_one_past.view(np.int64)).cuda()
    out = torch.full((8 * (n + 1) + 128,), SENTINEL, dtype=torch.int64, device="cuda")
    d.string_neighbours_device(0, d_ids.data_ptr(), n + 1, out.data_ptr() + 512, stream=_stream())
    torch.cuda.synchronize()
    got = out.cpu().numpy().view(np.uint64)
    assert (got[:64] == SENTINEL).all() and (got[-64:] == SENTINEL).all(), f"{what}: string_neighbours_device wrote outside its output"
    got = got[64:-64].reshape(-1, 8)
    assert (got[1000] == np.uint64(INVALID)).all(), f"{what}: string_neighbours_device, the id past the end"
    assert np.array_equal(np.delete(got, 1000, 0).reshape(-1), host), f"{what}: string_neighbours_device (ids) against the host's string_neighbours"
    # the range form, every field, both settings of check_reverse_complement; against the ground truth and the host's kmer neighbours
    in_order = d.string_neighbours(np.arange(n, dtype=np.uint64))
    for check_rc in (True, False):
        want = expected_string_neighbours(T, np.arange(n), canonical or check_rc)
        fields = {f: torch.full((8 * n,), SENTINEL, dtype=torch.int64, device="cuda") for f in U64_FIELDS}
        ori = torch.full((8 * n,), 77, dtype=torch.int8, device="cuda")
        flag = torch.full((8 * n,), 77, dtype=torch.uint8, device="cuda")
        extra = {f: t.data_ptr() for f, t in fields.items() if f != "kmer_id"}
        first, count = (0, n) if check_rc else (3, n - 3)  # (a range that does not begin at string 0)
        d.string_neighbours_device(0, 0, count, fields["kmer_id"].data_ptr(), check_reverse_complement=check_rc, stream=_stream(), first_string=first,
                                   kmer_orientation=ori.data_ptr(), minimizer_found=flag.data_ptr(), **extra)
        torch.cuda.synchronize()
        for f in U64_FIELDS:
            g = fields[f].cpu().numpy().view(np.uint64)[:8 * count]
            assert np.array_equal(g, want[f][8 * first:]), f"{what}: string_neighbours_device(full), check_rc={check_rc}: {f}"
        g = ori.cpu().numpy()[:8 * count]
        found = want["found"][8 * first:]
        assert np.array_equal(g[found], want["kmer_orientation"][8 * first:][found]), f"{what}: string_neighbours_device(full), check_rc={check_rc}: kmer_orientation"
        if check_rc:
            assert np.array_equal(fields["kmer_id"].cpu().numpy().view(np.uint64), in_order), f"{what}: string_neighbours_device (range) against the host's string_neighbours"
            # the fields the strings alone do not decide (the orientation and the minimizer flag of a miss): the host's kmer_neighbours of the end k-mers
            W = d.words_per_kmer()
            ends = d.access_packed(np.stack([T.first[1:] - 1, T.first[:-1]], 1).reshape(-1).astype(np.uint64)).reshape(-1, W)
            nb = d.neighbours(ends.reshape(-1), full=True)
            pick = (np.arange(n)[:, None] * 16 + np.concatenate([np.arange(4), 8 + 4 + np.arange(4)])[None, :]).reshape(-1)
            assert np.array_equal(g, nb.kmer_orientation[pick]) and np.array_equal(flag.cpu().numpy(), nb.minimizer_found[pick]), f"{what}: string_neighbours_device(full) against neighbours(full)"
    return int(want["found"].sum())


def check_links(T, d, canonical, what, cases):
    n = T.num_strings
    full_off, full_links = expected_links(T, 0, n, True)
    total = int(full_off[-1])
    for setting in LINKS_CHUNKS:
        chunk = chunk_of(n, setting)
        with hooks(f"links_chunk={chunk}" if chunk else None):
            h_off, h_links = d.string_links()
            assert np.array_equal(h_off, full_off) and h_links.tobytes() == full_links.tobytes(), f"{what}: string_links, links_chunk={chunk}: differs from the ground truth"
            if setting in (None, 7, -1):
                d_off, d_links, untouched = links_on_device(d, 0, n, total)
                assert untouched, f"{what}: string_links_device, links_chunk={chunk}: wrote outside its arrays"
                assert np.array_equal(d_off, h_off) and d_links.tobytes() == h_links.tobytes(), f"{what}: string_links_device against string_links, links_chunk={chunk}"
            if setting in (None, 256):
                for b, e in sub_ranges(T, cases):
                    w_off, w_links = expected_links(T, b, e, True)
                    h_off, h_links = d.string_links(b, e)
                    assert np.array_equal(h_off, w_off) and h_links.tobytes() == w_links.tobytes(), f"{what}: string_links({b}, {e}), links_chunk={chunk}"
                    d_off, d_links, untouched = links_on_device(d, b, e, int(w_off[-1]))
                    assert untouched and np.array_equal(d_off, w_off) and d_links.tobytes() == w_links.tobytes(), f"{what}: string_links_device({b}, {e}), links_chunk={chunk}"
    # one strand only
    w_off, w_links = expected_links(T, 0, n, canonical)
    h_off, h_links = d.string_links(check_reverse_complement=False)
    assert np.array_equal(h_off, w_off) and h_links.tobytes() == w_links.tobytes(), f"{what}: string_links, one strand"
    # capacities: the offsets are always those of the whole, the records below the capacity those of the whole, nothing behind them is touched
    for chunk in (None, 1000):
        with hooks(f"links_chunk={chunk}" if chunk else None):
            for capacity in (0, total, total - 1, total // 2, 1):
                d_off, d_links, untouched = links_on_device(d, 0, n, capacity)
                assert untouched, f"{what}: string_links_device, capacity {capacity}: wrote at or beyond links + links_capacity"
                assert np.array_equal(d_off, full_off), f"{what}: string_links_device, capacity {capacity}: link_offsets"
                assert d_links.tobytes() == full_links[:capacity].tobytes(), f"{what}: string_links_device, capacity {capacity}: the records below it"
    return total, full_off, full_links


def check_adjacency(T, d, canonical, what, cases, full_off, full_links):
    import sshash_amd

    n = T.num_kmers
    want = expected_masks(T, True)
    for setting in ADJACENCY_CHUNKS:
        chunk = chunk_of(n, setting)
        ranges = [(0, n)] + (adjacency_ranges(T, cases) if setting in (None, 1, 2047) else [])
        with hooks(f"adjacency_chunk={chunk}" if chunk else None):
            for b, e in ranges:
                got = d.kmer_adjacency(b, e)
                assert np.array_equal(got, want[b:e]), f"{what}: kmer_adjacency({b}, {e}), adjacency_chunk={chunk}: differs from the ground truth"
                if setting == 1 and e - b > 4096:  # (rounds of one k-mer over the whole range: once, through the host form)
                    continue
                on_device, untouched = adjacency_on_device(d, b, e)
                assert untouched and np.array_equal(on_device, got), f"{what}: kmer_adjacency_device({b}, {e}), adjacency_chunk={chunk}"
    assert np.array_equal(d.kmer_adjacency(check_reverse_complement=False), expected_masks(T, canonical)), f"{what}: kmer_adjacency, one strand"
    # the masks of every string's end k-mers agree with the degrees of its links
    forward, backward = sshash_amd.adjacency_degrees(want)
    at_end, at_start = sshash_amd.link_degrees(full_off, full_links)
    assert np.array_equal(forward[T.first[1:] - 1], at_end) and np.array_equal(backward[T.first[:-1]], at_start), f"{what}: the masks of the end k-mers against link_degrees"
    inner = np.ones(n, dtype=bool)
    inner[T.first[1:] - 1] = inner[T.first[:-1]] = False
    return int(((forward > 1) | (backward > 1))[inner].sum())


def check_shards(T, strings, fasta, index_path, canonical, what, full_off, full_links):
    import torch

    import sshash_amd

    shard = sshash_amd.Dictionary.build(fasta, k=T.k, m=m_of(T.k), canonical=canonical, num_threads=4, num_shards=2, shard_id=0).to_device(0)
    off = torch.zeros(T.num_strings + 1, dtype=torch.int64, device="cuda")
    masks = torch.zeros(T.num_kmers, dtype=torch.uint8, device="cuda")
    for call in (lambda: shard.string_links(), lambda: shard.string_links_device(0, 0, T.num_strings, off.data_ptr(), stream=_stream()), lambda: shard.kmer_adjacency(),
                 lambda: shard.kmer_adjacency_device(0, 0, T.num_kmers, masks.data_ptr(), stream=_stream())):
        try:
            call()
        except sshash_amd.SSHashError as e:
            assert e.status == 1, f"{what}: a minimizer shard: status {e.status}"
        else:
            raise AssertionError(f"{what}: a minimizer shard answered a graph call")
    shard.close()
    for shard_id in (0, 1):  # table shards: a replica that holds half of the table's keys answers every query
        part = sshash_amd.Dictionary.load(index_path).to_device(0, table_shards=2, table_shard_id=shard_id)
        off_p, links_p = part.string_links()
        assert np.array_equal(off_p, full_off) and links_p.tobytes() == full_links.tobytes(), f"{what}: string_links of table shard {shard_id} of 2"
        part.close()


def read_gfa(path):
    seqs, links = {}, []
    with open(path) as f:
        assert f.readline().startswith("H\t")
        for line in f:
            t = line.rstrip("\n").split("\t")
            if t[0] == "S":
                seqs[int(t[1])] = t[2]
            else:
                assert t[0] == "L"
                links.append((int(t[1]), t[2], int(t[3]), t[4], t[5]))
    return seqs, links


def expected_gfa_links(T, links):
    """the end-to-end links of the ground truth, by the rule of include/sshash_amd.h spelled out link by link"""
    out = []
    for r in links:
        f = int(r["flags"])
        at_start, rc, first, last = bool(f & 4), bool(f & 8), bool(f & 16), bool(f & 32)
        if (not at_start and ((not rc and first) or (rc and last))) or (at_start and ((not rc and last) or (rc and first))):
            out.append((int(r["from_string"]), "-" if at_start else "+", int(r["to_string"]), "+" if rc == at_start else "-", f"{T.k - 1}M"))
    return out


def check_gfa(T, d, strings, tmp, what, full_off, full_links):
    import sshash_amd

    path = os.path.join(tmp, "graph.gfa")
    sshash_amd.write_gfa(d, path)
    seqs, links = read_gfa(path)
    assert [seqs[s] for s in range(len(strings))] == list(strings), f"{what}: the S lines of write_gfa"
    want = expected_gfa_links(T, full_links)
    assert links == want and len(links) == int(sshash_amd.links_gfa(full_links)[0].sum()), f"{what}: the L lines of write_gfa"
    return len(links)


def check_flavour(T, strings, cases, canonical, tmp):
    import sshash_amd

    k = T.k
    what = f"k={k} m={m_of(k)} {'canonical' if canonical else 'regular'}"
    fasta = os.path.join(tmp, f"graph_{int(canonical)}.fa")
    with open(fasta, "w") as f:
        for s in strings:
            f.write(">\n" + s + "\n")
    d = sshash_amd.Dictionary.build(fasta, k=k, m=m_of(k), canonical=canonical, num_threads=4)
    assert d.num_strings() == T.num_strings and d.num_kmers() == T.num_kmers
    index_path = os.path.join(tmp, f"graph_{int(canonical)}.sshash")
    d.save(index_path)
    d.to_device(0)
    out = {"neighbours_found": check_string_neighbours(T, d, canonical, what)}
    out["links"], full_off, full_links = check_links(T, d, canonical, what, cases)
    out["junctions_inside_strings"] = check_adjacency(T, d, canonical, what, cases, full_off, full_links)
    out["gfa_links"] = check_gfa(T, d, strings, tmp, what, full_off, full_links)
    d.close()
    check_shards(T, strings, fasta, index_path, canonical, what, full_off, full_links)
    return out


def salmonella(tmp):
    """the stitched strings of the golden fixture (647 strings, k = 31, m = 13, regular): string_links over all strings and a window of 200 000 ids
    of kmer_adjacency against the ground truth (a sorted array: 4.8 M k-mers are too many for the Python dict)"""
    import sshash_amd
    from conftest import SE_FASTA
    from oracle.ground_truth import GroundTruth, read_fasta_sequences

    k = 31
    strings = read_fasta_sequences(SE_FASTA, k)
    gt = GroundTruth(strings, k)
    first = np.concatenate([[0], np.cumsum([len(t) - k + 1 for t in strings])]).astype(np.int64)
    begin = np.concatenate([[0], np.cumsum([len(t) for t in strings])]).astype(np.int64)
    n, S = int(first[-1]), len(strings)
    lo = int(first[S // 2]) - 100000
    window = np.arange(lo, lo + 200000)
    rows = np.concatenate([first[1:] - 1, first[:-1], window])  # the end k-mers of every string, then the window
    nb_id, nb_ori = truth_packed(gt, k, rows)
    T = SimpleNamespace(k=k, first=first, begin=begin, num_strings=S, num_kmers=n)
    # nb_id / nb_ori as expected_string_neighbours indexes them: by k-mer id -- sparse here, the rows that were asked for
    T.nb_id, T.nb_ori = _Sparse(rows, nb_id), _Sparse(rows, nb_ori)
    d = sshash_amd.Dictionary.build(SE_FASTA, k=k, m=13, num_threads=4).to_device(0)
    assert d.num_strings() == S and d.num_kmers() == n
    w_off, w_links = expected_links(T, 0, S, True)
    h_off, h_links = d.string_links()
    assert np.array_equal(h_off, w_off) and h_links.tobytes() == w_links.tobytes(), "salmonella: string_links differs from the ground truth"
    masks = d.kmer_adjacency(lo, lo + 200000)
    want = ((nb_ori[2 * S:] != 0).astype(np.uint8) << np.arange(8, dtype=np.uint8)[None, :]).sum(1).astype(np.uint8)
    assert np.array_equal(masks, want), "salmonella: kmer_adjacency differs from the ground truth"
    forward, backward = sshash_amd.adjacency_degrees(masks)
    inner = ~np.isin(window, first[1:] - 1) & ~np.isin(window, first[:-1])
    d.close()
    return {"strings": S, "kmers": n, "links": int(h_links.size), "end_to_end": int(sshash_amd.links_gfa(h_links)[0].sum()),
            "junctions_inside_strings": int(((forward > 1) | (backward > 1))[inner].sum())}


class _Sparse:
    """rows of a (num_kmers, 8) array that was computed for some k-mer ids only, indexed [ids, columns] as the whole would be"""

    def __init__(self, ids, values):
        order = np.argsort(ids, kind="stable")
        self.ids, self.values = np.asarray(ids)[order], values[order]

    def __getitem__(self, key):
        ids, cols = key
        at = np.searchsorted(self.ids, ids)
        assert (self.ids[at] == ids).all()
        return self.values[at, cols]

    def __ne__(self, other):
        return _Sparse(self.ids, self.values != other)

    def __eq__(self, other):
        return _Sparse(self.ids, self.values == other)


def main():
    import tempfile

    which, scratch = sys.argv[1], sys.argv[2]
    os.environ.pop("SSHASH_AMD_TEST_HOOKS", None)
    t0 = time.time()
    with tempfile.TemporaryDirectory(dir=scratch) as tmp:
        if which == "salmonella":
            out = salmonella(tmp)
            print(json.dumps({"ok": True, "salmonella": out, "seconds": round(time.time() - t0, 2)}))
            return
        k = int(which)
        assert k in KS
        strings, cases = make_graph(k, 6000 + k)
        T = truth(strings, k)
        reached = link_cases(T, cases)
        t1 = time.time()
        seconds, dictionaries = {"inputs": round(t1 - t0, 2)}, {}
        for canonical in (False, True):
            name = "canonical" if canonical else "regular"
            t1 = time.time()
            dictionaries[name] = check_flavour(T, strings, cases, canonical, tmp)
            seconds[name] = round(time.time() - t1, 2)
    print(json.dumps({"ok": True, "k": k, "m": m_of(k), "reached": reached, "dictionaries": dictionaries, "seconds": seconds}))


if __name__ == "__main__":
    main()
