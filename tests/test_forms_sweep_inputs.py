"""CPU: the inputs of tests/test_gpu_forms_sweep.py and the references it trusts, before a device is involved -- the gate that
tests/gpu_forms_worker.py runs ahead of its first device call, for every row of the matrix and both flavours: the reads hold every kind
of read and of run (forward, backward, of one k-mer, of 64 and more, from id 0, to the last id, reads shorter than k, empty, without a
hit, with N's), seams of every kind fall where segments of 1, 2, 7 and 64 k-mers are cut, the ids of the oracle's restated state machine
equal GroundTruth.lookup of every valid k-mer of every read (the long reads above 2^16 bases among them), the repeated read is one run,
and at an even m the reads walk over at least FLOOR tying k-mers of the dictionary. The sweep holds all ten forms of the run kernel.
For the sums the gate computes, per read, values[ids].sum() and the number of ids over those oracle ids, and once more the kernel's
own formula over the oracle's run records -- P[hi] - P[lo] over P = numpy.cumsum(values) in 64 bits, [lo, hi) from the record's kmer_id,
its length and its backward bit -- and asserts the two equal, for full-range random values, for whether they reach 2^31, and for all
0xFFFFFFFF; under the random values a run moved by one id, at either end or both, sums to something else, except where there is no
such id: runs from id 0 and runs to the last id, of which there are some at every point. For the classes, the best run and the run
records over segments (tests/gpu_forms_later.py) the gate computes two references each and asserts them equal: the best run as the
argmax with the tie rule (the largest num_kmers & 0x7FFFFFFF, the first of equals, 32 zero bytes without a hit) over the oracle's run
records and over the run rule applied to its per-k-mer results; the rows of 3 and of 65 classes, under string id % C and under random
labels a third of which are no class, from the per-k-mer ids through id -> string -> label and from the run records,
rows[read, labels[string_id]] += length; the run records over segments are the uncut records. At every point the reads hold reads with
two and more runs of the maximal length (the four jump reads by construction), reads whose best run is not their first, is backward,
reads without a hit, reads with two and more non-zero columns, k-mers that a masked label drops, rows whose columns sum to the read's
positive k-mers where no label is masked, and runs that span three whole segments of 1, 7 and 64 k-mers and more -- of 256 in the reads
above 2^16 bases."""
from __future__ import annotations

import pytest

from gpu_even_m_worker import FLOOR, build_host_tool
from gpu_forms_worker import MATRIX, SEGMENT_SIZES, gate, make_inputs


@pytest.fixture(scope="module")
def table_keys_exe(tmp_path_factory):
    return build_host_tool("table_keys", tmp_path_factory.mktemp("table_keys"))


def test_the_matrix_is_the_one_the_sweep_promises():
    assert len(MATRIX) == len(set(MATRIX)) == 44
    assert sum(layer == "directory" for _, _, _, layer in MATRIX) == 6 and sum(L != 0 for _, _, L, _ in MATRIX) == 12
    assert all(L == 0 or layer == "table" for _, _, L, layer in MATRIX)


@pytest.mark.parametrize("canonical", [False, True], ids=["regular", "canonical"])
@pytest.mark.parametrize("k,m,key_length,layer", MATRIX, ids=[f"{layer}-k{k}m{m}" + (f"key{L}" if L else "") for k, m, L, layer in MATRIX])
def test_gate(k, m, key_length, layer, canonical, table_keys_exe, tmp_path):
    pt = make_inputs(k, m, key_length, canonical, table_keys_exe, str(tmp_path))
    got = gate(pt)  # (asserts every kind and both references)
    print(f"k={k} m={m} key={key_length} canonical={canonical}: {got['kmers']} k-mers in {got['strings']} strings, {got['reads']} reads, {got['runs']} runs, "
          f"seams joined {got['seams_joined']}, sums {got['sums']}")
    assert 5000 <= got["kmers"] <= 80000 and all(got["seams_joined"][str(S)] > 0 for S in SEGMENT_SIZES)
    assert all(len(r) > (1 << 16) for r in pt.long_reads) and len(pt.repeated) == 4096
    sums = got["sums"]
    assert sums["runs"] == got["runs"] and sums["runs_without_an_id_below"] > 0 and sums["runs_without_an_id_above"] > 0
    assert sums["positive_kmers"] > 0 and sums["largest_row_sum"] > (1 << 32) and sums["largest_row_sum_of_the_long_reads"] > 20000 * 0xFFFFFFFF
    assert set(pt.want_sums) == set(pt.want_batch_sums) == {"random", "at least 2^31", "all ones"}
    # the three forms that came after the sweep of seven: what a wrong kernel needs to show is in the reads, at every point
    best, classes, spanning = got["best_run"], got["classes"], got["runs_over_three_segments"]
    print(f"best run {best}, classes {classes}, runs over three segments and more {spanning}")
    assert best["ties_for_the_longest"] >= 4 and best["longest_is_not_the_first"] > 0 and best["longest_is_backward"] > 0 and best["reads_without_a_hit"] > 0
    assert best["longest_of_the_long_reads"] > 600
    assert set(classes) == {f"{name} / {C}" for name in ("reads_with_two_columns", "kmers_of_a_masked_label") for C in (3, 65)} and all(v > 0 for v in classes.values())
    assert set(spanning) == {str(S) for S in SEGMENT_SIZES} | {"long reads, default S"} and all(v > 0 for v in spanning.values())
    assert pt.want_best.size == len(pt.reads) and pt.want_batch_best.size == len(pt.batch) == 43
    assert set(pt.want_classes) == set(pt.want_batch_classes) == {"mod / 3", "random / 3", "mod / 65", "random / 65"}
    if m % 2 == 0:
        assert all(c["read_kmers_found"] >= FLOOR for c in got["floors"].values()), got["floors"]
    else:
        assert got["floors"] is None
