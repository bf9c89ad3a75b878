"""CPU: the inputs of tests/test_gpu_idside.py reach what that test is for, at every k -- from the tile arithmetic of
iterate_packed_device alone, restated by gpu_idside_worker.describe over the launches of gpu_idside_worker.plan: a tile that needs all
2049 entries the stage was sized for, tiles that need a second to eighth round of the staging loop, tiles that stage entries past
num_strings, blocks of three and more tiles whose strings do not fit one stage (a block that kept the string index of its first tile
could not reach its last), blocks that end in a partial tile, launches with fewer blocks than iterate_blocks allows, and rounds of the
check that begin behind id 0 with a shorter last one. And the dictionary itself: its host iterator, its host access and the oracle
agree with the input strings on every id, so the worker's references are references."""
from __future__ import annotations

import numpy as np
import pytest

from conftest import Case
from gpu_idside_worker import (BLOCKS, CHECK_CHUNKS, DUP_CHUNK, KS, LENGTHS, PAIRS, RAGGED, SHIFTS, SINGLES, SINGLES_AT_THE_END, STAGE, TILE, check_rounds, chunk_of,
                               describe, dup_expectations, first_ids_of, gate, make_dense, make_dup, make_inputs, plan, stretches, string_picks, summary,
                               weight_depths)


def test_the_points_are_the_ones_the_sweep_promises():
    assert KS == (15, 17, 31, 33, 35, 47, 61, 63) and BLOCKS == (None, 1, 2, 3, 7) and CHECK_CHUNKS == (None, 2048, 3 * 2048 + 5, -1)
    assert LENGTHS == (2047, 2048, 2049, 3 * 2048 + 5) and SHIFTS == (-1, 0, 1, 2047, 2048) and (TILE, STAGE) == (2048, 2304)


def test_describe_on_strings_counted_by_hand():
    """five strings of 1, 3000, 1, 1 and 2000 k-mers: ids 0 | 1 .. 3000 | 3001 | 3002 | 3003 .. 5002"""
    first = np.array([0, 1, 3001, 3002, 3003, 5003])
    (whole,) = describe([(0, 5003, 1)], first)
    assert (whole["tiles"], whole["tiles_per_block"], whole["grid"]) == (3, 3, 1)
    # tile 0 = ids [0, 2048): strings 0 and 1, closed by string 2 (first id 3001 >= 2048); tile 1 = [2048, 4096): strings 1 .. 4, closed by
    # entry 5, which holds num_kmers; tile 2 = [4096, 5003): string 4 and the same entry
    assert whole["string_lo"].tolist() == [0, 1, 4] and whole["needs"].tolist() == [3, 5, 2] and whole["staged"].tolist() == [256] * 3
    assert whole["past_the_strings"].tolist() == [True] * 3  # (256 entries from string 0, 1 or 4 on: past entry 5)
    (two,) = describe([(1, 4100, 2)], first)
    assert (two["tiles"], two["tiles_per_block"], two["grid"]) == (3, 2, 2) and two["needs"].tolist() == [2, 5, 2]
    (free,) = describe([(1, 4100, None)], first)
    assert (free["tiles_per_block"], free["grid"]) == (1, 3)
    assert describe([(7, 7, 3)], first) == []
    c = summary([whole, two, free])
    assert c["most_tiles_per_block"] == 3 and c["blocks_ending_in_a_partial_tile"] == 1 and c["launches_with_fewer_blocks_than_allowed"] == 0
    assert c["blocks_of_3_tiles_and_more_than_one_stage"] == 0 and c["tiles"] == 9
    singles = np.arange(0, 3 * TILE + 1)  # 3 x 2048 strings of one k-mer
    (dense,) = describe([(0, 3 * TILE, 1)], singles)
    assert dense["needs"].tolist() == [TILE + 1] * 3 and dense["staged"].tolist() == [STAGE] * 3 and dense["past_the_strings"].tolist() == [False, False, True]
    assert summary([dense])["blocks_of_3_tiles_and_more_than_one_stage"] == 1 and summary([dense])["tiles_of_2049_strings"] == 3
    assert check_rounds(5003, 2048) == [2048, 2048, 907] and check_rounds(5003, 5002) == [5002, 1] and check_rounds(10, 1 << 25) == [10]


@pytest.mark.parametrize("k", KS, ids=[f"k{k}" for k in KS])
def test_the_launches_reach_the_gaps(k, tmp_path):
    sequences = make_dense(k, 4000 + k)
    assert [len(s) for s in sequences[:2]] == [k + 700, k] and len(sequences) == 2 + SINGLES + PAIRS + RAGGED + SINGLES_AT_THE_END == 10246
    first = first_ids_of(sequences, k)
    n = int(first[-1])
    (a1, e1), (a2, e2) = stretches(first)
    assert e1 - a1 == SINGLES and (a2, e2) == (n - SINGLES_AT_THE_END, n)
    triples = plan(first, k)
    ranges = {(b, e) for b, e, _ in triples}
    for blocks in BLOCKS:  # the named ranges under every setting
        mine = {(b, e) for b, e, x in triples if x == blocks}
        assert (0, n) in mine and all((a1 + shift, a1 + shift + L) in mine for shift in SHIFTS for L in LENGTHS) and all((n - L, n) in mine for L in LENGTHS)
        assert all((a2 + shift, n) in mine for shift in SHIFTS)
    assert (n, n) in ranges and (0, 0) in ranges and (n - 1, n) in ranges and len(triples) < 3000
    launches = describe(triples, first)
    c = summary(launches)
    print(k, n, c)
    assert c["tiles_of_2049_strings"] > 0, "some tile needs all 2049 entries"
    assert c["tiles_of_257_to_2048_strings"] > 0, "some tile needs a second to eighth round"
    assert {int(x) for d in launches for x in d["staged"]} == set(range(256, STAGE + 1, 256)), "every number of rounds of the staging loop, 1 to 9"
    assert c["tiles_staging_past_the_strings"] > 0, "some tile stages entries past num_strings"
    assert any((d["past_the_strings"] & (d["staged"] > 256)).any() for d in launches), "... also in a round that is not the first"
    assert c["blocks_of_3_tiles_and_more_than_one_stage"] > 0, "some block owns three tiles and more, over more strings than one stage holds"
    assert c["blocks_ending_in_a_partial_tile"] > 0 and c["launches_with_fewer_blocks_than_allowed"] > 0
    assert all(d["tiles_per_block"] == 1 for d in launches if d["blocks"] is None), "with the hook unset every block owns one tile"
    assert {d["tiles_per_block"] for d in launches if d["blocks"] == 1} >= {1, 2, 4, n // TILE + 1}
    for setting in CHECK_CHUNKS[1:3]:
        rounds = check_rounds(n, chunk_of(n, setting))
        assert len(rounds) >= 3 and rounds[-1] < rounds[0] and set(rounds[:-1]) == {rounds[0]}, (setting, rounds)
    assert check_rounds(n, chunk_of(n, -1)) == [n - 1, 1]
    # the other calls' inputs
    depths = weight_depths(first)  # (asserts what its docstring says)
    assert set(depths) == {"constant", "edges"} and len(set(depths["constant"].tolist())) == 1
    picks = string_picks(first, 900 + k)
    assert {0, len(sequences) - 1} <= set(picks.tolist())
    # the dictionary: host iterator, host access and oracle against the input strings, both flavours; the dictionary with one string twice
    dup_strings, at_a, at_b = make_dup(k, 5000 + k)
    for canonical in (False, True):
        pt = make_inputs(k, canonical, str(tmp_path), sequences)
        assert gate(pt) == c
        exp = dup_expectations(Case(f"dup{int(canonical)}", dup_strings, k, pt.m, canonical, str(tmp_path)), at_a, at_b)  # (asserts the oracle's picture)
        assert min(exp.copies) >= DUP_CHUNK and exp.want[2] == exp.want[3] == 7
