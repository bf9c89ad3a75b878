"""GPU: the id -> k-mer side -- iterate_kernel, access_kernel, weight_kernel, expand_neighbours_kernel, revcomp_kernel and
check_compare_kernel behind sshash_check_device, the host's string_neighbours -- at k = 15, 17, 31, 33, 35, 47, 61 and 63 (m = min(k, 13)),
regular and canonical, on a dictionary that is dense in strings: thousands of strings of ONE k-mer in a row, twice, the second time at
the end. The k-mer -> id side was swept over (k, m, key length, layer) before; this side had run on the fixtures only (k = 15, 21, 31,
63; dozens to thousands of k-mers a string; under 5 M k-mers), where on an MI355X no block of iterate_kernel owns a second tile, no tile
stages more than its first 256 string starts and the check takes one round. Here the hooks iterate_blocks and check_chunk make blocks
own up to all tiles of a range and the check take up to two dozen rounds; tests/test_idside_inputs.py asserts on the CPU that the
launches reach the hand-over between the tiles of a block, every round of the staging loop, a full stage of 2304 entries, entries past
num_strings, partial last tiles and rounds of the check that begin at an id other than 0. Every case is one run of
tests/gpu_idside_worker.py in a fresh process with a time limit of its own; all comparisons are exact, against the input strings and
the CPU oracle.

Measured on an MI355X, the eight workers one after the other: 60 s together, 6.1 to 6.9 s a worker (14 s the first, on a machine that
had not run the library before). Of that the inputs and references on the CPU -- two dictionaries of 10 246 strings, the one with a
string twice, two weighted rebuilds -- take 0.7 s (k = 15) to 2.0 s (k = 63), the device calls of the regular flavour 3.7 to 4.3 s (the
start of the runtime, the first upload and the two weighted replicas; 12 s in the first worker) and the device calls of the canonical
flavour, about 1800 launches of the iterator, the checks in up to 24 rounds, access, neighbours and string neighbours, 0.14 to 0.18 s:
k -> seconds on the device (regular, canonical): 15 -> (12.19, 0.14), 17 -> (4.32, 0.14), 31 -> (3.91, 0.16), 33 -> (4.30, 0.16),
35 -> (3.69, 0.16), 47 -> (4.10, 0.16), 61 -> (3.70, 0.17), 63 -> (3.68, 0.18)."""
from __future__ import annotations

import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT
from gpu_idside_worker import CHECK_CHUNKS, KS, m_of

_STOPPED = []  # why no further worker is started: one of them faulted, aborted or ran out of time
TIME_LIMIT = 180  # seconds, as tests/test_gpu_forms_sweep.py


@pytest.mark.gpu
@pytest.mark.parametrize("k", KS, ids=[f"k{k}" for k in KS])
def test_id_side(k, tmp_path):
    assert not _STOPPED, "not started: " + _STOPPED[0]
    env = {name: value for name, value in os.environ.items() if not name.startswith("SSHASH_AMD_")}
    try:
        p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "gpu_idside_worker.py"), str(k), str(tmp_path)], capture_output=True, text=True,
                           timeout=TIME_LIMIT, env=env)
    except subprocess.TimeoutExpired:
        _STOPPED.append(f"the worker of k = {k} ran into its time limit")
        raise
    if p.returncode < 0 or p.returncode in (134, 139) or "illegal memory access" in p.stderr:  # a signal, an abort, a GPU fault: no further worker
        _STOPPED.append(f"the worker of k = {k} ended with status {p.returncode}")
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-6000:]
    got = json.loads(p.stdout.strip().splitlines()[-1])
    print({name: got[name] for name in ("k", "m", "seconds")}, got["dictionaries"]["regular"])
    assert got["ok"] and not got["cpu_only"] and (got["k"], got["m"]) == (k, m_of(k))
    assert set(got["dictionaries"]) == {"regular", "canonical"}
    for flavour, st in got["dictionaries"].items():
        assert st["strings"] == 10246 and 20000 <= st["kmers"] <= 50000, (flavour, st)
        assert st["most_tiles_per_block"] >= 10 and st["tiles_of_2049_strings"] > 0 and st["blocks_of_3_tiles_and_more_than_one_stage"] > 0, (flavour, st)
        assert len(st["check_rounds"]) == len(CHECK_CHUNKS) - 1 and max(st["check_rounds"].values()) >= 10, (flavour, st)
        assert st["neighbours_found"] > 1000, (flavour, st)
