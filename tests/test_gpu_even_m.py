"""GPU: even minimizer lengths. Every other dictionary the suite puts on a device has an odd m, and only an even-length m-mer can be
its own reverse complement -- the condition of the library's tie branches: a canonical dictionary whose strands elect the same minimizer
(the first pass defers the query, the deferred pass tries both alignments, `minimizer_found` of a miss is the second probe's), and a
k-mer whose strands elect equal table-key hashes (no table key: left out of the table, answered by the complete path in the lookup and
the streaming kernels, routed by the first word of its smaller strand). Every case is one run of tests/gpu_even_m_worker.py in a fresh
process (the replica layer is read from the environment when a replica is uploaded) with a time limit of its own: one layer x one point
(k, m), regular and canonical, on inputs with planted self-complementary m-mers whose ties are measured on the CPU before anything is
uploaded (tests/test_even_m_inputs.py checks the same inputs and references without a device). The worker's line reports how many ties
each call was sent; a run that lost its ties fails here."""
from __future__ import annotations

import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT
from gpu_even_m_worker import FLOOR, LAYERS, POINTS, build_host_tool

_STOPPED = []  # why no further worker is started: one of them faulted, aborted or ran out of time
LOOKUP_CALLS = ("lookup_host", "lookup_device", "route_device", "route_bucket", "route_bucket_by_key")
STREAMING_CALLS = ("streaming_query", "streaming_lookup", "streaming_query_per_read", "streaming_runs", "streaming_cover")
TIME_LIMIT = 180  # seconds; a worker takes 2.5 to 4.6 on an MI355X, most of it the start of the process and of the device


@pytest.fixture(scope="module")
def host_tools(tmp_path_factory):
    """tests/cpp/table_keys.cpp and tests/cpp/route_owners.cpp by plain g++: the host's election of a k-mer's table key and of its owner"""
    directory = tmp_path_factory.mktemp("even_m_tools")
    return build_host_tool("table_keys", directory), build_host_tool("route_owners", directory)


@pytest.mark.gpu
@pytest.mark.parametrize("k,m", POINTS, ids=[f"k{k}m{m}" for k, m in POINTS])
@pytest.mark.parametrize("layer", list(LAYERS))
def test_even_m(layer, k, m, host_tools, tmp_path):
    assert not _STOPPED, "not started: " + _STOPPED[0]
    env = dict(os.environ)
    for name in ("SSHASH_AMD_TEST_HOOKS", "SSHASH_AMD_SKTABLE", "SSHASH_AMD_DIRECTORY", "SSHASH_AMD_SK_M", "SSHASH_AMD_HBM_BUDGET"):
        env.pop(name, None)
    env.update(LAYERS[layer][0])
    try:
        p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "gpu_even_m_worker.py"), layer, str(k), str(m), host_tools[0], host_tools[1],
                            str(tmp_path)], capture_output=True, text=True, timeout=TIME_LIMIT, env=env)
    except subprocess.TimeoutExpired:
        _STOPPED.append(f"the worker of {layer}, k = {k}, m = {m} ran into its time limit")
        raise
    if p.returncode < 0 or p.returncode in (134, 139) or "illegal memory access" in p.stderr:  # a signal, an abort, a GPU fault: no further worker
        _STOPPED.append(f"the worker of {layer}, k = {k}, m = {m} ended with status {p.returncode}")
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-6000:]
    got = json.loads(p.stdout.strip().splitlines()[-1])
    print(got)
    assert got["ok"] and (got["layer"], got["k"], got["m"]) == (layer, k, m) and set(got["dictionaries"]) == {"regular", "canonical"}
    for flavour, st in got["dictionaries"].items():
        kinds = {"table", "minimizer"} if flavour == "canonical" else {"table"}
        assert (st["sk_slots"] > 0) == layer.startswith("table"), (flavour, st)
        assert set(st["dictionary_ties"]) == kinds and all(v >= FLOOR for v in st["dictionary_ties"].values()), (flavour, st["dictionary_ties"])
        assert set(st["sent"]) == set(LOOKUP_CALLS + STREAMING_CALLS)
        for call in LOOKUP_CALLS:  # k-mers of the dictionary that tie, and absent k-mers that tie
            assert set(st["sent"][call]) == kinds and all(min(v) >= FLOOR for v in st["sent"][call].values()), (flavour, call, st["sent"][call])
        for call in STREAMING_CALLS:  # k-mers of the reads that tie and are in the dictionary
            assert set(st["sent"][call]) == kinds and all(v[0] >= FLOOR for v in st["sent"][call].values()), (flavour, call, st["sent"][call])
