"""GPU: all ten output forms of the streaming run kernel -- counters, per-read rows, run counts and records, cover, depth, per-read
sums, per-read classes, per-read best run, run records over segments -- and the segments for long reads, swept over (k, m, length of
the table's keys, replica layer). The per-k-mer forms were swept
before (test_gpu_km_sweep.py, test_gpu_even_m.py); rows and runs ran on the fixture dictionaries, cover, depth and segments on the golden files only, none of them at
an even m, and no streaming call ran with a key length that is not the default. Every case is one run of tests/gpu_forms_worker.py in
a fresh process (the layer and the key length are read from the environment when a replica is uploaded) with a time limit of its own:
the 14 odd-m points of test_gpu_km_sweep.py and the 12 even-m points of gpu_even_m_worker.py on the table layer, 12 points with
SSHASH_AMD_SK_M on either side of m, and 6 points on the directory layer (no table: the complete seed path). The sums came a commit
after the sweep and had run at k = 31, m = 11 and k = 63, m = 25 only, never with a key length of the caller's and never on the directory
layer: here their host call, and value_prefix_device followed by the device call with and without a report, give byte for byte
values[ids].sum() and the number of ids per read over the oracle's ids -- uncut, in segments of 1, 7 and 64 k-mers, uncut again, over
the two reads above 2^16 bases (the host call's per-k-mer route with segments off) and over one read 4096 times -- for full-range random
values, whether they reach 2^31, and all 0xFFFFFFFF. The worker checks its reads and references on the CPU before anything is uploaded
(tests/test_forms_sweep_inputs.py does the same without a device); all comparisons are exact. A worker takes 5 to 16 s on an MI355X (most of it the start of the process and the first upload; the second
flavour's device calls take 0.2 to 0.3 s), the 44 together 5 min 22 s -- that was the sweep of six forms. With the sums, on one machine
in one session: 5 min 13 s for the 44 workers of the six forms, 5 min 22 s for the 44 of the seven (6 to 14 s a worker). Per worker the
references on the CPU take 0.09 s a flavour more, the device calls 0.05 to 0.1 s a flavour more (the second flavour's: 0.2 to 0.3 s
before, 0.2 to 0.5 s now), except on the directory layer at k = 55 and k = 63, 0.6 and 0.8 s a flavour more: there the uncut device call
over the two reads above 2^16 bases, which one lane each walks, takes 0.11 s whatever the form (seven such calls before, 0.8 s; six more
for the sums, 0.67 s) -- the sums' launches cost what the depth's cost.

The classes, the best run and the run records over segments came after that sweep and had run on the two golden dictionaries only,
(k = 31, m = 13) and (k = 63, m = 25 or 21), with the default key length, with and without the table: never at an even m, at m = k, at
another k, with a key length of the caller's, or on the directory layer. The sweep now holds all ten forms (tests/gpu_forms_later.py).
Uncut: the best run of the reads by host call and by device call, with a report -- which must be the batch's counters -- and without,
into records that held garbage between guard records, and runs_best on the host and on the device over the records of streaming_runs;
the classes for 3 and for 65 classes, under string id % C and under random labels a third of which are no class, host and device, with
and without a report, guard words around the rows; class_totals and class_best of one set of rows; one read 4096 times, 4096 equal
records and 4096 equal rows; the two reads above 2^16 bases by the host calls of all three forms (the position-parallel route: the run
marks, classes_add_ids_kernel, the finish over that CSR) and by the device calls of the classes and the best run (one lane a read).
For S of 1, 7 and 64 k-mers, device calls included: the run records by host call, and by device call with room for no record, for all
but the last and for all, sentinels behind the room untouched, one launch over segments counted per device call; the classes, host and
device, every device call one launch; the best run, host and device, the counter standing still. At the default S the reads above 2^16
bases: run records by host and device call, classes by host and device call, the best run by host call. Uncut again: all three, and
the counter stands still. Each of three deliberate changes to the library made the worker of (k = 33, m = 13) fail in these checks and
nowhere before them: the last of equal runs winning in best_run_store (uncut: best run, host call), a run's length less one in
classes_add (uncut: classes mod / 3, host call), one more than cont[g] in stream_segment_run_merge_kernel (run records, S = 1, host
records). Measured on one MI355X in one session: the 44 workers of the seven forms 5 min 25 s, the slowest 11.7 s (directory layer,
k = 63, m = 16); the 44 of the ten forms 6 min 2 s, the slowest 15.1 s (the first worker of the session, k = 21, m = 11: 6.5 s before;
behind it the directory layer at k = 63, m = 16 with 14.1 s, and at k = 55, m = 19 with 12.3 s against 10.4 s) -- 0.85 s a worker more on
average: the references on the CPU take 0.2 to 0.3 s a flavour more, the second flavour's device calls 0.1 s more on the table layer
(k = 33, m = 13: 0.34 s against 0.25 s) and 0.7 to 1.0 s a flavour more on the directory layer at k = 55 (6.3 and 2.4 s against 5.3 and
1.6 s), where the calls over the two long reads cost most."""
from __future__ import annotations

import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT
from gpu_even_m_worker import build_host_tool, key_length_of
from gpu_forms_worker import MATRIX, SEGMENT_SIZES, environment_of

_STOPPED = []  # why no further worker is started: one of them faulted, aborted or ran out of time
TIME_LIMIT = 180  # seconds, as tests/test_gpu_even_m.py


def case_id(k, m, key_length, layer):
    return f"{layer}-k{k}m{m}" + (f"key{key_length}" if key_length else "")


@pytest.fixture(scope="module")
def table_keys_exe(tmp_path_factory):
    return build_host_tool("table_keys", tmp_path_factory.mktemp("forms_tools"))


@pytest.mark.gpu
@pytest.mark.parametrize("k,m,key_length,layer", MATRIX, ids=[case_id(*row) for row in MATRIX])
def test_forms(k, m, key_length, layer, table_keys_exe, tmp_path):
    assert not _STOPPED, "not started: " + _STOPPED[0]
    env = {name: value for name, value in os.environ.items() if not name.startswith("SSHASH_AMD_")}
    env.update(environment_of(key_length, layer))
    what = case_id(k, m, key_length, layer)
    try:
        p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "gpu_forms_worker.py"), str(k), str(m), str(key_length), layer, table_keys_exe,
                            str(tmp_path)], capture_output=True, text=True, timeout=TIME_LIMIT, env=env)
    except subprocess.TimeoutExpired:
        _STOPPED.append(f"the worker of {what} ran into its time limit")
        raise
    if p.returncode < 0 or p.returncode in (134, 139) or "illegal memory access" in p.stderr:  # a signal, an abort, a GPU fault: no further worker
        _STOPPED.append(f"the worker of {what} ended with status {p.returncode}")
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-6000:]
    got = json.loads(p.stdout.strip().splitlines()[-1])
    print({name: got[name] for name in ("k", "m", "key_length", "layer", "seconds")},
          {name: {x: st[x] for x in ("kmers", "runs", "seams_joined", "sk_heavy_kmers", "segmented_launches", "sums", "best_run", "classes", "runs_over_three_segments",
                                       "segmented_launches_of_run_records", "segmented_launches_of_classes")} for name, st in got["dictionaries"].items()})
    assert got["ok"] and not got["cpu_only"] and (got["k"], got["m"], got["key_length"], got["layer"]) == (k, m, key_length, layer)
    assert set(got["dictionaries"]) == {"regular", "canonical"}
    for flavour, st in got["dictionaries"].items():
        assert (st["sk_slots"] > 0) == (layer == "table"), (flavour, st["sk_slots"])
        assert st["sk_key_length"] == (key_length or key_length_of(k, m)), (flavour, st["sk_key_length"])
        assert all(st["seams_joined"][str(S)] > 0 and st["segmented_launches"][str(S)] > 0 for S in SEGMENT_SIZES), (flavour, st)
        assert st["sums"]["positive_kmers"] > 0 and st["sums"]["largest_row_sum"] > (1 << 32), (flavour, st["sums"])
        assert st["sums"]["runs_without_an_id_below"] > 0 and st["sums"]["runs_without_an_id_above"] > 0, (flavour, st["sums"])
        # the classes, the best run, the run records over segments: what the reads hold for them, and that their calls went over segments
        assert len(st["best_run"]) == 5 and len(st["classes"]) == 4 and len(st["runs_over_three_segments"]) == len(SEGMENT_SIZES) + 1, (flavour, st)
        assert all(v > 0 for name in ("best_run", "classes", "runs_over_three_segments") for v in st[name].values()), (flavour, st)
        # (per S: the host call of the run records and its device call at three capacities; the host and the device call of the classes under four labellings)
        assert all(st["segmented_launches_of_run_records"][str(S)] >= 4 and st["segmented_launches_of_classes"][str(S)] >= 8 for S in SEGMENT_SIZES), (flavour, st)
