"""The scans behind the depth and the sums at the edges of their geometry. sshash_depth_finish_device (an inclusive scan over num_kmers
words of 32 bits) and sshash_value_prefix_device (an exclusive scan over num_kmers + 1 words of 64 bits) work in tiles of 4096 words, 16
words a lane, and had only run over whatever num_kmers the test dictionaries happen to have. Here num_kmers is chosen: 16 dictionaries
of exactly N k-mers, one seeded random string of N + k - 1 bases each, with N and N + 1 on, one below and one above a lane boundary and
a tile boundary (tests/gpu_scan_worker.py: SIZES).

CPU, no device: all 16 build, and their sizes come out exact (the host build refused none of them).

GPU, one worker process with a time limit of its own, per size: value_prefix_device against numpy.cumsum in 64 bits for full-range
random values, all 0xFFFFFFFF, and the thresholds 1 and 0xFFFFFFFF over values a quarter of which are 0 and a quarter 0xFFFFFFFF;
streaming_sums_device over the whole string on either strand (one run over every id: it reads word N of the prefix);
depth_finish_device against numpy.cumsum(dtype=uint32) in place and out of place at skews of 0, 1 and 3 words (0: the 16-byte path);
depth_string_sums and cover_string_counts, host and device, against depth.sum() and the bitmap's popcount below N. Guard words lie
around every device array. The worker took 12 s on one MI355X and 5 s on another (the first upload of a process, as in every
worker, varies that much); the 16 sizes with their builds, uploads and some thirty device calls each are a few seconds of it.

GPU, in this process: the prefix scan above one round of its middle launch. scan_sums_kernel takes 256 tile sums a round and carries
their total into the next; the depth's scan had run over that many tiles, the prefix's had not. The session's k = 31 dictionary holds
4.8 million k-mers, five rounds: value_prefix_device against numpy for full-range random values (every tile sum above 2^32, the carry
above 2^44) and all 0xFFFFFFFF, then streaming_sums_device over 300 reads cut from its strings on both strands, up to the last id,
against values[ids].sum() over the CPU oracle's point lookups."""
from __future__ import annotations

import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from gpu_scan_worker import K, LANE, SIZES, TILE, build

TIME_LIMIT = 180  # seconds, as the other workers


def test_the_sizes_sit_on_either_side_of_every_boundary():
    for edge in (LANE * 16, TILE - LANE, TILE, TILE + LANE, 2 * TILE):
        assert edge % LANE == 0
        for n in (edge - 1, edge, edge + 1):  # the depth's scan runs over n words, the prefix's over n + 1
            assert n in SIZES, n
    assert {TILE - 2, TILE - 1, TILE} <= set(SIZES), "n + 1 on either side of the tile boundary"
    assert len(SIZES) == len(set(SIZES)) == 16


def test_every_size_builds_exact(tmp_path):
    from gpu_even_m_worker import canonical_strings

    for n in SIZES:
        d, s = build(n, str(tmp_path))
        assert len(s) == n + K - 1 and len(canonical_strings(s, K)) == n, (n, "the string holds a k-mer twice")
        assert d.num_kmers() == n and d.num_strings() == 1 and d.cover_words() == (n + 63) // 64, (n, d.num_kmers(), d.num_strings())


@pytest.mark.gpu
def test_scans_at_lane_and_tile_edges(tmp_path):
    env = {name: value for name, value in os.environ.items() if not name.startswith("SSHASH_AMD_")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "gpu_scan_worker.py"), str(tmp_path)], capture_output=True, text=True, timeout=TIME_LIMIT,
                       env=env)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-6000:]
    got = json.loads(p.stdout.strip().splitlines()[-1])
    print(got)
    assert got["ok"] and got["sizes"] == SIZES


@pytest.mark.gpu
def test_prefix_scan_above_one_round(case_se_regular):
    from gpu_depth_worker import oracle_ids
    from gpu_per_read_worker import revcomp
    from gpu_sums_worker import device_prefix, device_sums, flat_ids, rows_of, same

    case, k = case_se_regular, case_se_regular.k
    d = case.dict.to_device(0)
    n = d.num_kmers()
    assert n == case.gt.num_kmers and n > (1 << 20) and (n + 1 + TILE - 1) // TILE > 2 * 256, "more than two rounds of 256 tile sums"
    # reads from strings spread over the whole index, the first and the last among them, on both strands
    rng = np.random.default_rng(61)
    seqs = case.sequences
    reads = [seqs[0][:k + 60], seqs[-1][-(k + 60):]]
    for i in np.linspace(0, len(seqs) - 1, 149).astype(np.int64):
        s = seqs[int(i)]
        size = min(len(s), int(rng.integers(100, 301)))
        at = int(rng.integers(0, len(s) - size + 1))
        reads.append(s[at:at + size])
    reads += [revcomp(r) for r in reads]
    assert len(reads) == 302
    ids = oracle_ids(case.oracle, reads, k)
    flat = flat_ids(ids)
    assert flat[1].size == sum(len(r) - k + 1 for r in reads), "every k-mer of the dictionary's own strings is found"
    assert int(flat[1].min()) == 0 and int(flat[1].max()) == n - 1 and int((flat[1] > (1 << 22)).sum()) > 1000
    values = np.random.default_rng(67).integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    for name, v in (("random", values), ("all ones", np.full(n, 0xFFFFFFFF, dtype=np.uint32))):
        t_prefix, p_prefix = device_prefix(d, v)  # (asserts the prefix against numpy.cumsum in 64 bits, the guard words and the values)
        want = rows_of(flat, len(reads), v)
        assert int(want["sum"].max()) > (1 << 32)
        rows, rep = device_sums(d, reads, p_prefix, report=[0] * 6)
        same(rows, want, f"{name}: streaming_sums_device over ids up to {n - 1}")
        assert int(rep[1]) == flat[1].size
        del t_prefix
