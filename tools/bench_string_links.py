#!/usr/bin/env python
"""The dictionary's graph on one MI355X: the links of all strings, the adjacency of all k-mers, and the route the parent commit had for the
first. Prints one JSON line per configuration:

    python tools/bench_string_links.py c2 [--reps 5] [--warmup 1] [--bases B] [--cache-dir DIR]

  L    links      sshash_string_links_device over all strings with every record: the counting pass (the ends' neighbours, an ids-only
                  lookup, a count per string), the prefix sum, the writing pass (the neighbours again, a lookup of four fields, the scatter)
  L0   count      the same with capacity 0: the counting pass and the prefix sum alone
  A    adjacency  sshash_kmer_adjacency_device over all ids: per round the iterator, the 8 neighbours, an ids-only lookup, the fold
  N    neighbours sshash_string_neighbours_device over all strings, ids only: the expansion and one lookup
  H    host route Dictionary.string_neighbours(all ids): what a caller had before -- the end k-mers decoded one at a time on the CPU, the
                  lookups through the host-buffer path, ids only (no strings, no orientations, no CSR); wall clock

The device forms alternate inside one loop; every figure is the median of --reps event-timed calls after --warmup rounds, lowest and highest
beside it. `glookups_per_s`: the lookups a call makes (8 per string and pass, 8 per k-mer) over its time. In the first round the records
are checked against H's ids and against the adjacency masks of the strings' end k-mers."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def log(msg):
    print(f"[bench_string_links] {msg}", file=sys.stderr, flush=True)


def run_config(name, args):
    import numpy as np
    import torch

    import bench
    import sshash_amd
    from sshash_amd.repeats import load_recipe

    bases, recipe, _, _ = bench.WORKLOADS[name]
    r = load_recipe(recipe)
    ns = argparse.Namespace(bases=args.bases or bases, k=int(r["k"]), m=int(r["m"]), canonical=False, seed=0x5555AAAA,
                            recipe=recipe, repeat_scale=1.0, cache_dir=args.cache_dir, verbose=False)
    d, _ = bench.get_index(ns, 0, 1, lambda: None)
    t0 = time.time()
    d.to_device(0)
    log(f"{name}: uploaded in {time.time() - t0:.1f}s")
    dev = torch.device("cuda", 0)
    S, n = d.num_strings(), d.num_kmers()
    stream = torch.cuda.current_stream().cuda_stream
    offsets = torch.zeros(S + 1, dtype=torch.int64, device=dev)
    d.string_links_device(0, 0, S, offsets.data_ptr(), stream=stream)
    torch.cuda.synchronize()
    total = int(offsets[S].item())
    links = torch.zeros(4 * total + 4, dtype=torch.int64, device=dev)
    masks = torch.zeros(n, dtype=torch.uint8, device=dev)
    ids = torch.zeros(8 * S, dtype=torch.int64, device=dev)
    rec = {"config": name, "k": d.k(), "m": d.m(), "num_strings": S, "num_kmers": n, "num_links": total, "reps": args.reps, "warmup": args.warmup}

    forms = {
        "links": (lambda: d.string_links_device(0, 0, S, offsets.data_ptr(), links.data_ptr(), total, stream=stream), 16 * S),
        "count": (lambda: d.string_links_device(0, 0, S, offsets.data_ptr(), stream=stream), 8 * S),
        "adjacency": (lambda: d.kmer_adjacency_device(0, 0, n, masks.data_ptr(), stream=stream), 8 * n),
        "neighbours": (lambda: d.string_neighbours_device(0, 0, S, ids.data_ptr(), stream=stream), 8 * S),
    }
    times = {f: [] for f in forms}
    for i in range(args.warmup + args.reps):
        for f, (fn, _) in forms.items():
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if i >= args.warmup:
                times[f].append(e0.elapsed_time(e1))
    for f, (_, lookups) in forms.items():
        ms = statistics.median(times[f])
        rec[f] = {"ms": ms, "lowest_ms": min(times[f]), "highest_ms": max(times[f]), "all_ms": times[f], "lookups": lookups, "glookups_per_s": lookups / ms / 1e6}

    all_ids = np.arange(S, dtype=np.uint64)
    host = []
    for _ in range(max(1, min(args.reps, 3))):
        t0 = time.time()
        host_ids = d.string_neighbours(all_ids)
        host.append((time.time() - t0) * 1e3)
    ms = statistics.median(host)
    rec["host_route"] = {"ms": ms, "lowest_ms": min(host), "highest_ms": max(host), "all_ms": host, "lookups": 8 * S, "glookups_per_s": 8 * S / ms / 1e6}

    # the records against the host route's ids, the masks of the end k-mers against the degrees of the links
    h_links = links[:4 * total].cpu().numpy().view(np.uint64).view(sshash_amd.LINK_DTYPE)
    h_offsets = offsets.cpu().numpy().view(np.uint64)
    found = host_ids != np.uint64(sshash_amd.INVALID_U64)
    assert np.array_equal(ids.cpu().numpy().view(np.uint64), host_ids), "string_neighbours_device against the host's string_neighbours"
    assert int(found.sum()) == total and np.array_equal(h_links["to_kmer_id"], host_ids[found]), "the links against the host's string_neighbours"
    assert np.array_equal(h_links["flags"] & 7, (np.flatnonzero(found) % 8).astype(np.uint32))
    begin, end = d.string_offsets(all_ids)
    first = (begin - all_ids * np.uint64(d.k() - 1)).astype(np.int64)
    last = (end - (all_ids + np.uint64(1)) * np.uint64(d.k() - 1)).astype(np.int64) - 1
    h_masks = masks.cpu().numpy()
    forward, backward = sshash_amd.adjacency_degrees(np.concatenate([h_masks[last], h_masks[first]]))
    at_end, at_start = sshash_amd.link_degrees(h_offsets, h_links)
    assert np.array_equal(forward[:S], at_end) and np.array_equal(backward[S:], at_start), "the masks of the end k-mers against link_degrees"
    end_to_end = sshash_amd.links_gfa(h_links)[0]
    deg_f, deg_b = sshash_amd.adjacency_degrees(h_masks)
    rec.update(end_to_end_links=int(end_to_end.sum()), links_into_strings=int(total - end_to_end.sum()), kmers_with_a_branch=int(((deg_f > 1) | (deg_b > 1)).sum()),
               links_over_host_route=rec["host_route"]["ms"] / rec["links"]["ms"])
    span = lambda e: f"{e['ms']:.2f} [{e['lowest_ms']:.2f}-{e['highest_ms']:.2f}] ms, {e['glookups_per_s']:.2f} G lookups/s"
    log(f"{name}: {S} strings, {n} k-mers, {total} links | L {span(rec['links'])} | L0 {span(rec['count'])} | A {span(rec['adjacency'])} | N {span(rec['neighbours'])} | H {span(rec['host_route'])}")
    d.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("configs", nargs="+", choices=["c2", "c3", "c4"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--bases", type=int, default=None, help="default: the workload's (bench.WORKLOADS)")
    ap.add_argument("--cache-dir", default=os.environ.get("SSHASH_BENCH_CACHE", "/tmp"))
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bench_string_links needs a GPU")
    for name in args.configs:
        print(json.dumps(run_config(name, args)), flush=True)


if __name__ == "__main__":
    main()
