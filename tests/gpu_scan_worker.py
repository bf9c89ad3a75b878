#!/usr/bin/env python
"""Worker of tests/test_gpu_scan_edges.py, and the inputs it shares with that file's CPU test: the two scans behind the depth and the
sums -- sshash_depth_finish_device, an inclusive scan over num_kmers words of 32 bits, and sshash_value_prefix_device, an exclusive scan
over num_kmers + 1 words of 64 bits -- at sizes that put n and n + 1 on, one below and one above the boundary of a lane's 16 words and
of a tile's 4096 words. Both scans work in tiles of 4096 words, 16 consecutive words a lane; the 32-bit scan moves a lane's words as
four 16-byte pieces where the arrays are 16-byte aligned and all 16 lie below n, word by word otherwise. A dictionary of exactly N
k-mers is one seeded random string of N + k - 1 bases (k = 31, m = 13). One process builds and uploads all of them; every comparison is
exact, against numpy.cumsum, and every device array lies between guard words. Prints one JSON line; any mismatch is an assertion error.

    python tests/gpu_scan_worker.py <scratch directory>"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import numpy as np

from gpu_per_read_worker import random_dna, revcomp

K, M = 31, 13
LANE, TILE = 16, 4096
# n (the depth's scan) and n + 1 (the prefix's) on, below and above: a lane boundary in the first tile (256), the last lane boundary of the
# first tile (4080), the tile boundary (4096), the first lane boundary of the second tile (4112), the second tile boundary (8192)
SIZES = [255, 256, 257, 4079, 4080, 4081, 4094, 4095, 4096, 4097, 4111, 4112, 4113, 8191, 8192, 8193]
ALL_ONES = 0xFFFFFFFF


def string_of(n_kmers):
    return random_dna(np.random.default_rng(52000 + n_kmers), n_kmers + K - 1)


def build(n_kmers, scratch):
    """-> (dictionary of exactly n_kmers k-mers in one string, the string)"""
    import sshash_amd

    s = string_of(n_kmers)
    fasta = os.path.join(scratch, f"scan_{n_kmers}.fa")
    with open(fasta, "w") as f:
        f.write(">\n" + s + "\n")
    return sshash_amd.Dictionary.build(fasta, k=K, m=M, canonical=False, num_threads=4), s


def popcount(words):
    return int(np.unpackbits(words.view(np.uint8)).sum())


def check_size(n, scratch):
    from gpu_cover_worker import device_string_counts
    from gpu_depth_worker import device_finish, device_string_sums
    from gpu_sums_worker import device_prefix, device_sums

    d, s = build(n, scratch)
    assert d.num_kmers() == n and d.num_strings() == 1, (n, d.num_kmers(), d.num_strings())
    d.to_device(0)
    rng = np.random.default_rng(n)
    # ---- the prefix: n + 1 words of 64 bits ----
    noise = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    edges = noise.copy()  # a quarter zeros, a quarter 0xFFFFFFFF: what the two thresholds turn on
    pick = rng.integers(0, 4, n)
    edges[pick == 0], edges[pick == 1] = 0, ALL_ONES
    assert int(noise.sum(dtype=np.uint64)) > (1 << 32)
    for name, values, at_least in (("random", noise, 0), ("all ones", np.full(n, ALL_ONES, dtype=np.uint32), 0), ("at least 1", edges, 1),
                                   ("at least all ones", edges, ALL_ONES)):
        t_prefix, p_prefix = device_prefix(d, values, at_least)  # (asserts the prefix against numpy.cumsum in 64 bits, the guards and the values)
        if name == "random":  # the whole string on either strand: one run over every id, which reads word n of the prefix
            rows, rep = device_sums(d, [s, revcomp(s)], p_prefix, report=[0] * 6)
            assert rows["sum"].tolist() == [int(noise.sum(dtype=np.uint64))] * 2 and rows["positive_kmers"].tolist() == [n, n], (n, rows)
            assert int(rep[1]) == 2 * n and int(rep[4]) == 2, (n, rep)
        del t_prefix
    # ---- the finish: n words of 32 bits ----
    want = np.cumsum(noise, dtype=np.uint32)
    for in_place in (True, False):
        for skew in (0, 1, 3):
            got = device_finish(d, noise, in_place, skew)  # (asserts the guards, and the input of an out-of-place finish)
            bad = np.flatnonzero(got != want)
            assert bad.size == 0, (n, "finish", in_place, skew, bad[:5].tolist(), got[bad[:5]].tolist(), want[bad[:5]].tolist())
    # ---- per string, over the one string ----
    total = int(noise.sum(dtype=np.uint64))
    for sums, got_total in (d.depth_string_sums(noise), device_string_sums(d, noise)):
        assert sums.shape == (1,) and int(sums[0]) == total == got_total, (n, "depth_string_sums", sums, got_total, total)
    words = d.cover_words()
    assert words == (n + 63) // 64
    cover = rng.integers(0, 1 << 63, words, dtype=np.uint64) | (rng.integers(0, 2, words, dtype=np.uint64) << np.uint64(63))
    valid = cover.copy()
    if n % 64:  # (bits at and above num_kmers are no k-mers: set here, and not counted)
        cover[-1] |= ~np.uint64((1 << (n % 64)) - 1)
        valid[-1] &= np.uint64((1 << (n % 64)) - 1)
    for cover_words, name in ((cover, "random"), (np.full(words, ~np.uint64(0), dtype=np.uint64), "ones")):
        bits = popcount(valid) if name == "random" else n
        for counts, got_total in (d.cover_string_counts(cover_words), device_string_counts(d, cover_words)):
            assert counts.shape == (1,) and int(counts[0]) == bits == got_total, (n, "cover_string_counts", name, counts, got_total, bits)
    d.close()


def main():
    import tempfile

    scratch = sys.argv[1]
    t0 = time.time()
    with tempfile.TemporaryDirectory(dir=scratch) as tmp:
        for n in SIZES:
            check_size(n, tmp)
    print(json.dumps({"ok": True, "sizes": SIZES, "seconds": round(time.time() - t0, 2)}))


if __name__ == "__main__":
    main()
