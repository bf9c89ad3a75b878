"""GPU: every output form of the streaming run kernel over the tables on which the kernel's own walk is common. streaming_run_kernel
keeps a walk state machine of its own (csrc/streaming.hip, from "a seed whose probe has to go on past its key's first bucket is WALKING"
down to "the complete seed()"): sk_walk_step of the lookup kernels inlined by hand, one bucket a turn, with the state carried from turn
to turn, plus `lasts` (the minimum over every bucket of the key's sequence: how many following k-mers a miss may declare negative
without a probe), the remembered heavy key, the way back from the k-mers' region to choice `back` of the key's sequence, and `defer`
for a key or k-mer that found no slot in five choices. All ten output forms hang on what that machine leaves behind when a walk
settles. The suite ran the run kernel on the default density over a complete table only (2.5 slots per item, 3.0 at k > 31), where
0.05 % of the keys find no slot and small dictionaries hold almost no unplaced item; the packed table, SSHASH_AMD_SK_DENSITY=compact
and a table shard had been through lookups and never through a streaming call.

Eighteen workers (tests/gpu_walks_worker.py), one process per point and layer, regular then canonical, each with the sweep's time limit;
once a worker faults, aborts or runs out of time no further worker of this file or of tests/test_gpu_forms_sweep.py is started. The
worker asserts from device_stats(), after the upload and before the first streaming call, per flavour:

    packed    SSHASH_AMD_TEST_HOOKS=slots_per_key=1.2,slots_per_kmer=1.2   sk_load_factor > 0.75, sk_deferred_keys >= 8, sk_heavy_kmers > 0
    compact   SSHASH_AMD_SK_DENSITY=compact                                sk_slots > 0, sk_deferred_keys >= 1, a load factor above that of a
                                                                           second handle of the same index file uploaded without the switch
    shard     to_device(0, table_shards=3, table_shard_id=1)               sk_keys between 0.15 and 0.6 of a whole upload's

Then everything the forms sweep does at the point (make_inputs, gate, check_flavour: all ten forms, host and device call, uncut,
S = 1, 7, 64, uncut again, the reads above 2^16 bases, one read 4096 times) on that replica, and two probe sets that make every item of
the table a seed -- every k-mer of the dictionary as a read of its own, the odd ids reverse-complemented; 1500 to 3000 windows of
2k + 8 bases with one substitution at base k + 3 -- through a slimmer pass: counters, rows, run offsets and records, cover, depth, sums,
classes, best run and the ids of streaming_lookup, host and device call, uncut, and the windows once more at S = 7 for rows, run records
and classes. References: the oracle's restated state machine and GroundTruth.lookup of every k-mer, asserted equal on the CPU first
(tests/test_walks_inputs.py does the same without a device), numpy over the oracle's results for the rest. All comparisons are exact.

Measured on one MI355X, sk_deferred_keys / sk_heavy_kmers / sk_load_factor, regular | canonical (which items find no slot depends on
the order in which the build's threads arrive: the counts move by a few per cent from upload to upload):

    packed   (21, 11)          192 / 836 / 0.80     | 183 / 836 / 0.80
    packed   (31, 7)           433 / 15018 / 0.81   | 418 / 15018 / 0.81
    packed   (31, 27)          386 / 559 / 0.80     | 389 / 559 / 0.80
    packed   (31, 21, key 17)  225 / 2030 / 0.80    | 251 / 2030 / 0.80
    packed   (31, 8)           60 / 33 / 0.78       | 58 / 33 / 0.78
    packed   (33, 13)          149 / 718 / 0.80     | 138 / 718 / 0.80    (2009 buckets in the keys' region)
    packed   (47, 15, key 31)  221 / 42 / 0.80      | 195 / 42 / 0.80
    packed   (63, 25, key 12)  184 / 3627 / 0.80    | 181 / 3627 / 0.80
    packed   (63, 30)          44 / 15 / 0.79       | 40 / 15 / 0.79
    packed   (63, 31)          107 / 868 / 0.80     | 105 / 868 / 0.80
    compact  (31, 7)           173 / 15018 / 0.72 (a default upload: 0.55) | 152 / 15018 / 0.72 (0.55)
    compact  (31, 21, key 17)  42 / 2030 / 0.65 (0.43)                     | 35 / 2030 / 0.65 (0.43)
    compact  (33, 13)          10 / 710 / 0.50 (0.34)                      | 9 / 710 / 0.50 (0.34)
    compact  (63, 31)          7 / 868 / 0.51 (0.34)                       | 10 / 868 / 0.50 (0.34)
    shard    (31, 27)          0 / 156 / 0.40, 3523 of 10384 keys, both flavours
    shard    (31, 8)           0 / 0 / 0.40, 407 of 1186 keys, both flavours
    shard    (47, 15, key 31)  0 / 0 / 0.33, 1923 of 5718 keys, both flavours
    shard    (63, 25, key 12)  1 / 2851 / 0.38, 713 of 2142 keys, both flavours

At k > 31 the compact density is 2.0 slots per item, a load factor of 0.5: the sweep's dictionaries of 34 314 and 41 171 k-mers left 3
items without a slot in either flavour, which meets the floor of 1 and would not on every upload. For the compact layer only, these two
points hold 60 000 and 90 000 bases of plain random strings more (91 567 and 122 254 k-mers): 7 to 12 items without a slot over two uploads of each flavour.

The packed point (33, 13) plants two table keys with equal 24-bit fingerprints and the same first bucket, one light (four occurrences)
and one heavy (gpu_walks_worker.COLLIDING): a seed on an occurrence of the light key that went on from that bucket meets the heavy
key's marker and the go-on flag, finds nothing under the k-mer's own key and has to come back to choice `back` of the key's sequence.
No dictionary of this size holds such a pair by chance, and without it nothing the kernel computes depends on `back`.

That the tests bite: three deliberate changes to streaming.hip, each built on its own and run once through this file's worker packed
(33, 13) and through test_gpu_forms_sweep.py::test_forms[table-k33m13] (the default density).
  1. This bucket's `lasts` kept instead of the minimum with `before`: the worker failed in its first check (streaming_query, the
     batch counters, regular) -- and so did the sweep at the default density: a second bucket is common enough at 34 314 k-mers for
     that one.
  2. back = WALK_NO_RETURN at a heavy key's marker whatever go_on says: the sweep passed; the worker passed as well until the two
     colliding keys were planted, and then failed in its first check (streaming_query, regular: the planted strings are reads).
  3. A key that runs out of choices settled as a miss instead of deferred: the sweep passed, the worker failed in its first check
     (streaming_query, regular).
None of the three faulted or hung. Changes 2 and 3 are the gap: the suite at the default density did not see either.

Time on one MI355X: the eighteen workers 3 min 25 s together, 7.7 to 15.6 s a worker (the sum of what the workers report: 191 s) -- 1.4 to
4.5 s a flavour for the inputs and references on the CPU, 4.3 to 6.8 s for the first flavour's device calls (the start of the process
and the first upload among them; 11.7 s in the session's first worker), 0.6 to 3.3 s for the second flavour's. The slowest are the
shards at k = 47 and 63 (the reads above 2^16 bases, two thirds of whose seeds take the complete path) and the two enlarged compact
points (set 1 has 91 567 and 122 254 reads there)."""
from __future__ import annotations

import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT
from gpu_even_m_worker import build_host_tool, key_length_of
from gpu_forms_worker import SEGMENT_SIZES
from gpu_walks_worker import DEFERRED_FLOOR, MATRIX, WINDOWS, environment_of
from test_gpu_forms_sweep import _STOPPED, TIME_LIMIT  # (one list: a worker of either sweep that faulted, aborted or ran out of time stops both)


def case_id(k, m, key_length, layer):
    return f"{layer}-k{k}m{m}" + (f"key{key_length}" if key_length else "")


@pytest.fixture(scope="module")
def table_keys_exe(tmp_path_factory):
    return build_host_tool("table_keys", tmp_path_factory.mktemp("walks_tools"))


@pytest.mark.gpu
@pytest.mark.parametrize("k,m,key_length,layer", MATRIX, ids=[case_id(*row) for row in MATRIX])
def test_walks(k, m, key_length, layer, table_keys_exe, tmp_path):
    assert not _STOPPED, "not started: " + _STOPPED[0]
    env = {name: value for name, value in os.environ.items() if not name.startswith("SSHASH_AMD_")}
    env.update(environment_of(key_length, layer))
    what = case_id(k, m, key_length, layer)
    try:
        p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "gpu_walks_worker.py"), str(k), str(m), str(key_length), layer, table_keys_exe,
                            str(tmp_path)], capture_output=True, text=True, timeout=TIME_LIMIT, env=env)
    except subprocess.TimeoutExpired:
        _STOPPED.append(f"the worker of {what} ran into its time limit")
        raise
    if p.returncode < 0 or p.returncode in (134, 139) or "illegal memory access" in p.stderr:  # a signal, an abort, a GPU fault: no further worker
        _STOPPED.append(f"the worker of {what} ended with status {p.returncode}")
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-6000:]
    got = json.loads(p.stdout.strip().splitlines()[-1])
    print({name: got[name] for name in ("k", "m", "key_length", "layer", "seconds")},
          {name: {"kmers": st["kmers"], "stats": st["stats"], "probes": st["probes"]} for name, st in got["dictionaries"].items()})
    assert got["ok"] and not got["cpu_only"] and (got["k"], got["m"], got["key_length"], got["layer"]) == (k, m, key_length, layer)
    assert set(got["dictionaries"]) == {"regular", "canonical"}
    for flavour, st in got["dictionaries"].items():
        stats, probes = st["stats"], st["probes"]
        assert st["sk_slots"] > 0 and st["sk_key_length"] == (key_length or key_length_of(k, m)), (flavour, st["sk_slots"], st["sk_key_length"])
        if layer == "packed":
            assert stats["sk_load_factor"] > 0.75 and stats["sk_deferred_keys"] >= DEFERRED_FLOOR[layer] == 8 and stats["sk_heavy_kmers"] > 0, (flavour, stats)
        elif layer == "compact":
            assert stats["sk_deferred_keys"] >= DEFERRED_FLOOR[layer] == 1 and stats["sk_load_factor"] > stats["default_load_factor"] > 0, (flavour, stats)
        else:
            assert 0.15 * stats["whole_sk_keys"] <= stats["sk_keys"] <= 0.6 * stats["whole_sk_keys"], (flavour, stats)
        assert probes["kmer_reads"] == st["kmers"] and WINDOWS[0] <= probes["windows"] <= WINDOWS[1], (flavour, probes)
        assert all(st["seams_joined"][str(S)] > 0 and st["segmented_launches"][str(S)] > 0 for S in SEGMENT_SIZES), (flavour, st)
