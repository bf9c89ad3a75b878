"""CPU: the inputs of tests/test_gpu_streaming_walks.py and the references it trusts, before a device is involved -- what
tests/gpu_walks_worker.py runs ahead of its first device call, for every point of its matrix and both flavours. The matrix is the
eighteen rows the test promises: ten points on the packed table, four under the compact density, four on a table shard; every point of
the packed table is one where the table holds k-mers under heavy keys (gpu_forms_worker.HEAVY) or where the dictionary plants table
keys. Probe set 1 is every k-mer of the dictionary as a read of its own -- read i is k-mer i, one search, the odd ids found backward --;
probe set 2 is 1500 to 3000 windows of 2k + 8 bases with one substitution at base k + 3, at least four in five of them four positive
k-mers, k negative ones and five positive ones in two runs (a substitution can land on another k-mer of the dictionary: those windows
are counted and printed). On both sets the ids of the oracle's restated state machine, read by read, equal GroundTruth.lookup of every
k-mer, and the numpy references of the sums, the classes and the best run agree between the per-k-mer ids and the run records
(gpu_walks_worker.make_probe asserts all of that). A point that holds more strings than the forms sweep's dictionary goes through the
sweep's own gate here as well (tests/test_forms_sweep_inputs.py has gated the others)."""
from __future__ import annotations

import pytest

from gpu_even_m_worker import build_host_tool, key_length_of
from gpu_forms_worker import HEAVY, ROOM, gate, make_inputs
from gpu_forms_worker import MATRIX as FORMS_MATRIX
from gpu_walks_worker import COLLIDING, MATRIX, PATTERN_SHARE, PLAIN_BASES, POINTS, WINDOWS, colliding_gate, extension_of, probe_gate


def _own(k, m, L, layer):
    """the layer where it puts strings of its own behind the point's, or "" (a point of two layers is one dictionary unless one of them does)"""
    return layer if (layer, k, m, L) in PLAIN_BASES or (layer, k, m, L) in COLLIDING else ""


DICTIONARIES = sorted({(k, m, L, _own(k, m, L, layer)) for k, m, L, layer in MATRIX})


@pytest.fixture(scope="module")
def table_keys_exe(tmp_path_factory):
    return build_host_tool("table_keys", tmp_path_factory.mktemp("table_keys"))


def test_the_matrix_is_the_one_the_test_promises():
    assert len(MATRIX) == len(set(MATRIX)) == 18
    assert {layer: len(points) for layer, points in POINTS.items()} == {"packed": 10, "compact": 4, "shard": 4}
    assert POINTS["packed"] == [(21, 11, 0), (31, 7, 0), (31, 27, 0), (31, 21, 17), (31, 8, 0), (33, 13, 0), (47, 15, 31), (63, 25, 12), (63, 30, 0), (63, 31, 0)]
    assert POINTS["compact"] == [(31, 7, 0), (31, 21, 17), (33, 13, 0), (63, 31, 0)]
    assert POINTS["shard"] == [(31, 27, 0), (31, 8, 0), (47, 15, 31), (63, 25, 12)]
    assert all((k, m, L, "table") in FORMS_MATRIX for k, m, L, _ in MATRIX), "every point is one of the forms sweep's"
    assert set(PLAIN_BASES) | set(COLLIDING) <= {(layer, k, m, L) for k, m, L, layer in MATRIX} and ("packed", 33, 13, 0) in COLLIDING
    for k, m, L in POINTS["packed"]:
        key = L or key_length_of(k, m)
        plants_table_keys = m % 2 == 1 and key != m and k - key >= ROOM  # (gpu_forms_worker.odd_sequences)
        assert (k, m, L) in HEAVY or plants_table_keys, (k, m, L)


@pytest.mark.parametrize("canonical", [False, True], ids=["regular", "canonical"])
@pytest.mark.parametrize("k,m,key_length,own", DICTIONARIES, ids=[f"k{k}m{m}" + (f"key{L}" if L else "") + (f"-{own}" if own else "") for k, m, L, own in DICTIONARIES])
def test_probes(k, m, key_length, own, canonical, table_keys_exe, tmp_path):
    pt = make_inputs(k, m, key_length, canonical, table_keys_exe, str(tmp_path), extend=extension_of(k, m, key_length, own, table_keys_exe))
    if own:
        gate(pt)  # (asserts every kind of read, run and seam and both references over the larger dictionary)
    if (own, k, m, key_length) in COLLIDING:
        print("the planted keys:", colliding_gate(pt, key_length, COLLIDING[(own, k, m, key_length)], table_keys_exe))
    got = probe_gate(pt)  # (asserts the two references equal on both sets, and the references of every form)
    print(f"k={k} m={m} key={key_length} own strings={own or 'none'} canonical={canonical}: {got}")
    n = pt.case.gt.num_kmers
    assert got["kmer_reads"] == n == len(pt.kmer_probe.reads) and got["kmer_reads_backward"] == n // 2
    assert (pt.kmer_probe.rows[:, 4] == 1).all() and (pt.kmer_probe.rows[:, 0] == 1).all()
    assert 1500 == WINDOWS[0] <= got["windows"] <= WINDOWS[1] and got["windows_as_expected"] >= PATTERN_SHARE * got["windows"] and PATTERN_SHARE == 0.8
    assert got["window_negatives"] >= k * got["windows_as_expected"] and got["window_runs"] >= 2 * got["windows_as_expected"]
    print("windows whose substitution lands on another k-mer of the dictionary, or that are not 4 / k / 5:", got["windows"] - got["windows_as_expected"],
          "with more than nine positive k-mers:", got["windows_with_another_kmer_of_the_dictionary"])
