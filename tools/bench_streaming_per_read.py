#!/usr/bin/env python
"""The per-read streaming query on one MI355X beside the batch's six counters and beside the route to per-read numbers that
needs no per-read kernel. Prints one JSON line per configuration:

    python tools/bench_streaming_per_read.py c3 c4 [--reps 10] [--reads N] [--cache-dir DIR] [--tree DIR --label parent]

  counters        sshash_streaming_query_device: six counters for the batch (the yardstick)
  per_read        sshash_streaming_query_per_read_device: one row of six counters per read, with and without the batch's report
                  (absent when the library has no such call: a build of an earlier commit)
  lookup_reduce   sshash_streaming_lookup_device with kmer_id only, then the positives per read by a segmented reduction in torch
                  (ids != INVALID over the places of a read that hold a k-mer, summed along the read): what a caller had to do without per_read

Every figure: median of --reps event-timed calls after --warmup, k-mers/s = the reads' k-mers / that. The read sets are the ones
bench.py's streaming lines use (sshash_amd.synthetic.make_reads_device, same seed): c3 = the k = 31 stand-in with 95 % of the reads
from the dictionary ("high-hit"), c4 = the k = 63 stand-in with 50 %; dictionaries as bench.py builds and caches them.
--tree DIR imports the package (and its library) from another checkout -- the build of the commit to compare with --, so that both
are measured by this one file, on one box, in one session; --label names the lines."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POSITIVE = {"c3": 0.95, "c4": 0.5}


def log(msg):
    print(f"[bench_streaming_per_read] {msg}", file=sys.stderr, flush=True)


def timed(fn, reps, warmup):
    """median and all of `reps` event-timed calls (ms), after `warmup` untimed ones"""
    import torch

    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    return statistics.median(times), times


def run_config(name, args):
    import torch

    import bench
    from sshash_amd.repeats import load_recipe
    from sshash_amd.synthetic import make_reads_device

    bases, recipe, _, _ = bench.WORKLOADS[name]
    r = load_recipe(recipe)
    ns = argparse.Namespace(bases=args.bases or bases, k=int(r["k"]), m=int(r["m"]), canonical=False, seed=0x5555AAAA,
                            recipe=recipe, repeat_scale=1.0, cache_dir=args.cache_dir, verbose=False)
    d, _ = bench.get_index(ns, 0, 1, lambda: None)
    t0 = time.time()
    d.to_device(0)
    log(f"{name}: uploaded in {time.time() - t0:.1f}s")
    dev = torch.device("cuda", 0)
    n, L, k = args.reads, args.read_len, d.k()
    reads = make_reads_device(d, 0, n, L, positive_fraction=POSITIVE[name], seed=ns.seed)
    offsets = torch.arange(n + 1, dtype=torch.int64, device=dev) * L
    report = torch.zeros(6, dtype=torch.int64, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    kmers = n * (L - k + 1)
    rec = {"config": name, "label": args.label, "k": k, "num_kmers_of_the_dictionary": d.num_kmers(), "reads": n, "read_len": L,
           "positive_fraction_of_reads": POSITIVE[name], "kmers_per_call": kmers, "reps": args.reps}

    def entry(ms, all_ms):
        return {"ms": ms, "all_ms": all_ms, "gkmers_per_s": kmers / ms / 1e6, "spread": (max(all_ms) - min(all_ms)) / ms}

    def counters():
        report.zero_()
        d.streaming_query_device(0, reads.data_ptr(), offsets.data_ptr(), n, report.data_ptr(), stream=stream, total_bases=n * L)

    rec["counters"] = entry(*timed(counters, args.reps, args.warmup))
    totals = report.clone()
    rec["report"] = [int(v) for v in totals.cpu().tolist()]
    log(f"{name}: counters {rec['counters']['ms']:.2f} ms")

    if hasattr(d, "streaming_query_per_read_device") and "per_read" in args.only:
        rows = torch.full((n, 6), -1, dtype=torch.int64, device=dev)

        def per_read():
            report.zero_()
            d.streaming_query_per_read_device(0, reads.data_ptr(), offsets.data_ptr(), n, rows.data_ptr(), d_report=report.data_ptr(),
                                              stream=stream, total_bases=n * L)

        def per_read_rows_only():
            d.streaming_query_per_read_device(0, reads.data_ptr(), offsets.data_ptr(), n, rows.data_ptr(), stream=stream, total_bases=n * L)

        rec["per_read"] = entry(*timed(per_read, args.reps, args.warmup))
        assert torch.equal(rows.sum(0), totals) and torch.equal(report, totals), (rows.sum(0), report, totals)
        rows.fill_(-1)
        rec["per_read_rows_only"] = entry(*timed(per_read_rows_only, args.reps, args.warmup))
        assert torch.equal(rows.sum(0), totals)
        positives = rows[:, 1].clone()
        del rows
        log(f"{name}: per_read {rec['per_read']['ms']:.2f} ms, rows only {rec['per_read_rows_only']['ms']:.2f} ms")
    else:
        positives = None

    if "lookup_reduce" not in args.only:
        d.close()
        return rec
    ids = torch.empty(n * L, dtype=torch.int64, device=dev)
    per_read_positives = [None]

    def lookup_reduce():
        d.streaming_lookup_device(0, reads.data_ptr(), offsets.data_ptr(), n, n * L, ids.data_ptr(), stream=stream)
        per_read_positives[0] = (ids.view(n, L)[:, :L - k + 1] != -1).sum(1)  # (the last k - 1 places of a read hold no k-mer and are not written)

    rec["lookup_reduce"] = entry(*timed(lookup_reduce, args.reps, args.warmup))
    assert int(per_read_positives[0].sum().item()) == rec["report"][1]
    if positives is not None:
        assert torch.equal(per_read_positives[0], positives), "positives per read: the two routes disagree"
        rec["per_read_over_counters"] = rec["per_read"]["gkmers_per_s"] / rec["counters"]["gkmers_per_s"]
        rec["per_read_over_lookup_reduce"] = rec["per_read"]["gkmers_per_s"] / rec["lookup_reduce"]["gkmers_per_s"]
    log(f"{name}: lookup + reduce {rec['lookup_reduce']['ms']:.2f} ms")
    del ids, reads
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    d.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("configs", nargs="+", choices=["c3", "c4"])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reads", type=int, default=20_000_000, help="reads in the set (bench.py's streaming lines: 2 x 10^7)")
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--bases", type=int, default=None, help="default: the workload's (bench.WORKLOADS)")
    ap.add_argument("--cache-dir", default=os.environ.get("SSHASH_BENCH_CACHE", "/tmp"))
    ap.add_argument("--tree", default=ROOT, help="the checkout whose sshash_amd package and library are measured (default: this one)")
    ap.add_argument("--label", default="this", help="names the lines of this run")
    ap.add_argument("--only", default="per_read,lookup_reduce", help="which of per_read, lookup_reduce to measure beside counters (a profiler's run: one)")
    args = ap.parse_args()
    args.only = args.only.split(",")
    sys.path.insert(0, os.path.abspath(args.tree))
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bench_streaming_per_read needs a GPU")
    import sshash_amd

    log(f"package: {os.path.dirname(sshash_amd.__file__)}")
    for name in args.configs:
        print(json.dumps(run_config(name, args)), flush=True)


if __name__ == "__main__":
    main()
