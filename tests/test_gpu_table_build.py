"""GPU: the super-k-mer table that a replica builds at upload (csrc/sktable.hip), held against the strings. Every lookup and every form
of the streaming run kernel reads that table, and the suite saw its builder through answers only -- and the table is built so that
answers survive its mistakes: an item that was dropped or misfiled is answered by the complete path as long as a go-on flag points past
it, a spurious flag or filter bit costs a line and no answer, so does a key made heavy at four occurrences, so do counters that drift;
an extent one base too long changes an answer only for a query that equals a window across two neighbouring strings. The numbers the
build publishes (sshash_device_stats [4..13], the 20 words of sshash_device_table_histogram; bench.py writes them into every record)
were held against `> 0`, floors and ratios.

Eight workers (tests/gpu_table_worker.py), one process per point (k, m, key length) of the walks' list, regular then canonical, each
under the sweeps' time limit and their one list of stopped workers: (21, 11), (31, 7) -- m < 12, most k-mers under heavy keys --,
(31, 21, key 17), (31, 27), (33, 13) -- with the walks' two colliding keys --, (47, 15, key 31), (63, 25, key 12), (63, 31); 30 000 to
52 000 k-mers each. The dictionary is the walks' (make_inputs with extension_of) plus what gpu_table_worker.with_table_edges plants so
that every point holds a key with exactly 4 tuples and one with exactly 5, an inline occurrence less than k - L bases into the first
string, an item that ends the collection (tests/test_table_inputs.py asserts these and the rest of the conditions on the CPU). Per
flavour six uploads of fresh handles of one index file -- default, packed (SSHASH_AMD_TEST_HOOKS=slots_per_key=1.2,slots_per_kmer=1.2),
SSHASH_AMD_SK_DENSITY=compact, shards 0, 1, 2 of 3 --, the worker setting the two variables between the uploads: sktable.hip reads
the density at every build and the hooks are read at every call of the C ABI, and the published sizes, compared exactly with the
reference's for that density, say that each took. Per upload: device_stats() and device_table_histogram() against
tests/table_reference.py, exact; the info of Dictionary.device_table() against both; verify() of the exported table without a
violation; items present == sk_slots_used, absent == sk_deferred_keys; every k-mer of the dictionary on both strands returns its id,
and every window of k bases across the border of two neighbouring stored strings (5 660 to 21 638 a point; none is a k-mer of these
dictionaries), and its reverse complement, gets the oracle's answer, which is GroundTruth.lookup's. On the default upload also the
export's own edges: info alone, a capacity one byte short (SSHASH_ERR_ARGUMENT, nothing written), a larger buffer (nothing written
behind the table), a replica without a table (all-zero info, OK). Over the three shards every key is owned exactly once and the keys
and items add up to the whole table's. All comparisons are exact.

Measured on one MI355X, items without a slot (sk_deferred_keys) / items found past their first choice / items in slot 1 or in a later
entry of their bucket; default, packed, compact, shard 0, 1, 2; regular | canonical (which items go where depends on the order in which
the build's threads arrive: the counts move from upload to upload):

    (21, 11)          5 954 items   2/447/1848  192/1028/2644  34/829/2344  0/182/771  1/124/518  0/148/547
                                  | 3/446/1846  192/1028/2641  36/827/2339  0/182/770  1/124/517  0/148/549
    (31, 7)          16 827 items   17/1754/8259  429/2718/9683  152/2508/9345  8/564/2620  3/555/2522  3/588/3061
                                  | 14/1757/8247  449/2698/9670  165/2495/9336  6/566/2632  0/558/2526  3/588/3058
    (31, 21, key 17)  7 527 items   1/588/2524  226/1329/3509  33/1049/3160  1/171/770  0/188/831  2/219/938
                                  | 1/588/2524  232/1323/3501  33/1049/3169  0/172/771  0/188/826  0/221/936
    (31, 27)         11 060 items   3/867/3199  377/2006/4715  57/1591/4188  0/296/1017  0/276/1043  1/284/1101
                                  | 4/866/3193  372/2011/4721  59/1589/4174  0/296/1013  0/276/1043  0/285/1102
    (33, 13)          4 070 items   0/252/1012  134/763/1709  2/452/1324  0/66/255  0/76/314  0/91/418
                                  | 0/252/1011  131/766/1709  1/453/1324  0/66/252  0/76/316  0/91/417
    (47, 15, key 31)  5 777 items   2/330/1403  186/1058/2428  9/588/1805  0/104/437  0/122/473  0/100/476
                                  | 0/332/1399  185/1059/2432  7/590/1808  0/104/435  0/122/474  0/100/475
    (63, 25, key 12)  5 816 items   0/401/1540  207/1012/2421  8/685/1940  0/62/215  2/252/963  2/78/343
                                  | 0/401/1539  195/1024/2434  11/682/1951  0/62/217  0/254/962  1/79/343
    (63, 31)          3 489 items   0/225/858  115/613/1453  6/401/1133  0/67/288  0/70/313  0/61/253
                                  | 0/225/855  114/614/1454  3/404/1134  0/67/288  0/70/308  0/61/255

That the test bites: three deliberate changes to sktable.hip, each a stored value or a count (no address, loop bound or launch), each
built on its own and run once through this file's worker (33, 13), through tests/test_gpu_km_sweep.py at k33m13 (both flavours) and
through the forms sweep's worker table-k33m13.
  1. `heavy = size >= SK_INLINE_MAX` in sk_classify_kernel: the worker failed in its first check (device_stats(), regular, default: 12
     heavy keys and 748 k-mers entered one by one against the reference's 9 and 723). The km sweep and the forms sweep passed.
  2. `left` one too large where it is below k - L, in sk_place_kernel: the worker failed in verify() (regular, default: 337 slots named
     `left`). The km sweep passed; the forms sweep failed (the batch counters of its long reads, which run across string borders).
  3. `used` counted for SK_ITEM_NONE tuples too: the worker failed at sk_slots_used + sk_deferred_keys == items (4118 against 4070).
     The km sweep and the forms sweep passed.
None of the three faulted or hung. The builder as it is passed at all 8 x 2 x 6 uploads: the test found no fault in it.

Time on one MI355X: the whole file 15.8 s, 1.2 to 2.9 s a worker -- 0.6 to 1.6 s for the first flavour's inputs and references on the
CPU and 0.1 to 0.8 s for the second's, 0.21 to 0.28 s for the first flavour's six uploads with all their checks (the first upload of the
process among them) and 0.06 to 0.09 s for the second's."""
from __future__ import annotations

import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT
from gpu_even_m_worker import build_host_tool, key_length_of
from gpu_table_worker import POINTS, UPLOADS, environment_of
from test_gpu_forms_sweep import _STOPPED, TIME_LIMIT  # (one list: a worker of any sweep that faulted, aborted or ran out of time stops them all)


def case_id(k, m, key_length):
    return f"k{k}m{m}" + (f"key{key_length}" if key_length else "")


@pytest.fixture(scope="module")
def host_tools(tmp_path_factory):
    directory = tmp_path_factory.mktemp("table_tools")
    return build_host_tool("table_keys", directory), build_host_tool("table_hashes", directory)


@pytest.mark.gpu
@pytest.mark.parametrize("k,m,key_length", POINTS, ids=[case_id(*row) for row in POINTS])
def test_table(k, m, key_length, host_tools, tmp_path):
    assert not _STOPPED, "not started: " + _STOPPED[0]
    env = {name: value for name, value in os.environ.items() if not name.startswith("SSHASH_AMD_")}
    env.update(environment_of(key_length))
    what = case_id(k, m, key_length)
    try:
        p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "gpu_table_worker.py"), str(k), str(m), str(key_length), *host_tools, str(tmp_path)],
                           capture_output=True, text=True, timeout=TIME_LIMIT, env=env)
    except subprocess.TimeoutExpired:
        _STOPPED.append(f"the worker of {what} ran into its time limit")
        raise
    if p.returncode < 0 or p.returncode in (134, 139) or "illegal memory access" in p.stderr:  # a signal, an abort, a GPU fault: no further worker
        _STOPPED.append(f"the worker of {what} ended with status {p.returncode}")
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-6000:]
    got = json.loads(p.stdout.strip().splitlines()[-1])
    print(p.stdout.strip().splitlines()[-1])
    assert got["ok"] and not got["cpu_only"] and (got["k"], got["m"], got["key_length"]) == (k, m, key_length)
    assert set(got["dictionaries"]) == {"regular", "canonical"}
    for flavour, st in got["dictionaries"].items():
        assert list(st["uploads"]) == [name for name, *_ in UPLOADS] and len(UPLOADS) == 6, (flavour, list(st["uploads"]))
        assert st["lookups"]["kmers"] > 0 and st["lookups"]["border_windows"] > 0 and st["conditions"]["heavy_kmers"] > 0, (flavour, st)
        for name, up in st["uploads"].items():
            assert up["sk_slots_used"] + up["sk_deferred_keys"] == up["items"] > 0, (flavour, name, up)
        # the packed layer is where the flags are certain, whatever the order of arrival (conditions(): buckets that are the first choice of three items)
        assert st["uploads"]["packed"]["past_first_choice"] > 0 and st["uploads"]["packed"]["in_slot_1_or_a_later_entry"] > 0, (flavour, st["uploads"]["packed"])
    assert key_length_of(k, m) > 0
