"""GPU: all seven output forms of the streaming run kernel -- counters, per-read rows, run counts and records, cover, depth, per-read
sums -- and the segments for long reads, swept over (k, m, length of the table's keys, replica layer). The per-k-mer forms were swept
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
for the sums, 0.67 s) -- the sums' launches cost what the depth's cost."""
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
          {name: {x: st[x] for x in ("kmers", "runs", "seams_joined", "sk_heavy_kmers", "segmented_launches", "sums")} for name, st in got["dictionaries"].items()})
    assert got["ok"] and not got["cpu_only"] and (got["k"], got["m"], got["key_length"], got["layer"]) == (k, m, key_length, layer)
    assert set(got["dictionaries"]) == {"regular", "canonical"}
    for flavour, st in got["dictionaries"].items():
        assert (st["sk_slots"] > 0) == (layer == "table"), (flavour, st["sk_slots"])
        assert st["sk_key_length"] == (key_length or key_length_of(k, m)), (flavour, st["sk_key_length"])
        assert all(st["seams_joined"][str(S)] > 0 and st["segmented_launches"][str(S)] > 0 for S in SEGMENT_SIZES), (flavour, st)
        assert st["sums"]["positive_kmers"] > 0 and st["sums"]["largest_row_sum"] > (1 << 32), (flavour, st["sums"])
        assert st["sums"]["runs_without_an_id_below"] > 0 and st["sums"]["runs_without_an_id_above"] > 0, (flavour, st["sums"])
