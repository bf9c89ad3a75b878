#!/usr/bin/env python
"""The streaming depth (sshash_streaming_depth_device + sshash_depth_finish_device: how often a read set holds each k-mer of the
dictionary) on one MI355X beside the forms of the run kernel it is made from, and beside the route a caller had to take before it.
Prints one JSON line per configuration:

    python tools/bench_streaming_depth.py c3 c4 [--reps 10] [--reads N] [--host-reads N] [--cache-dir DIR]

  A  counters   sshash_streaming_query_device: six counters for the batch
  V  cover      sshash_streaming_cover_device into a ZEROED bitmap: bitmap + totals
  D  depth      sshash_streaming_depth_device into ZEROED deltas: deltas + totals (no finish)
  F  finish     sshash_depth_finish_device over those deltas, in place on a copy: the prefix sum over num_kmers words
  S  string_sums  sshash_depth_string_sums_device over the depths
  H  histogram on the host, the route replaced, over the first --host-reads reads: sshash_streaming_lookup_device (one id per base), the
     ids copied to the host, counted there (numpy.unique with counts); and D + F over the same reads beside it

A, V, D and F ALTERNATE inside one loop of one process (A V D F, A V D F, ...), so that a drift of the machine falls on all of them alike;
the zeroing and the copy are outside the timed regions. Every figure: median of --reps event-timed calls after --warmup rounds, with all
of them listed; k-mers/s = the reads' k-mers / that. Read sets and dictionaries: those of tools/bench_streaming_cover.py."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_streaming_per_read import POSITIVE, timed  # noqa: E402


def log(msg):
    print(f"[bench_streaming_depth] {msg}", file=sys.stderr, flush=True)


def run_config(name, args):
    import numpy as np
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
    n, L, k, n_kmers = args.reads, args.read_len, d.k(), d.num_kmers()
    reads = make_reads_device(d, 0, n, L, positive_fraction=POSITIVE[name], seed=ns.seed)
    offsets = torch.arange(n + 1, dtype=torch.int64, device=dev) * L
    report = torch.zeros(6, dtype=torch.int64, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    kmers = n * (L - k + 1)
    rec = {"config": name, "k": k, "num_kmers_of_the_dictionary": n_kmers, "num_strings": d.num_strings(), "reads": n, "read_len": L,
           "positive_fraction_of_reads": POSITIVE[name], "kmers_per_call": kmers, "reps": args.reps, "delta_bytes": 4 * n_kmers}

    def entry(all_ms, per=kmers):
        ms = statistics.median(all_ms)
        return {"ms": ms, "all_ms": all_ms, "gkmers_per_s": per / ms / 1e6, "spread": (max(all_ms) - min(all_ms)) / ms}

    cover = torch.zeros(d.cover_words() + 1, dtype=torch.int64, device=dev)
    deltas = torch.zeros(n_kmers + 1, dtype=torch.int32, device=dev)  # (a guard word behind the last)
    depth = torch.zeros(n_kmers + 1, dtype=torch.int32, device=dev)

    def counters():
        d.streaming_query_device(0, reads.data_ptr(), offsets.data_ptr(), n, report.data_ptr(), stream=stream, total_bases=n * L)

    def cover_form():
        d.streaming_cover_device(0, reads.data_ptr(), offsets.data_ptr(), n, cover.data_ptr(), d_report=report.data_ptr(), stream=stream, total_bases=n * L)

    def depth_form():
        d.streaming_depth_device(0, reads.data_ptr(), offsets.data_ptr(), n, deltas.data_ptr(), d_report=report.data_ptr(), stream=stream, total_bases=n * L)

    def finish():
        d.depth_finish_device(0, depth.data_ptr(), depth.data_ptr(), stream=stream)

    forms = [("counters", counters, lambda: None), ("cover", cover_form, cover.zero_), ("depth", depth_form, deltas.zero_),
             ("finish", finish, lambda: depth.copy_(deltas))]
    times = {name_: [] for name_, _, _ in forms}
    totals = None
    for i in range(args.warmup + args.reps):
        for name_, fn, before in forms:
            before()
            report.zero_()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if i >= args.warmup:
                times[name_].append(e0.elapsed_time(e1))
            if name_ == "counters":
                totals = report.clone() if totals is None else totals
            if name_ != "finish":
                assert torch.equal(report, totals), name_
    for name_ in times:
        rec[name_] = entry(times[name_], n_kmers if name_ == "finish" else kmers)
    rec["report"] = [int(v) for v in totals.cpu().tolist()]
    rec["finish"]["ms_per_1e9_kmers"] = rec["finish"]["ms"] * 1e9 / n_kmers
    rec["finish"]["gb_per_s_read_twice_written_once"] = 12 * n_kmers / rec["finish"]["ms"] / 1e6
    rec["depth_over_cover"] = rec["depth"]["ms"] / rec["cover"]["ms"]
    rec["depth_inside_the_spread_of_cover"] = min(rec["cover"]["all_ms"]) <= rec["depth"]["ms"] <= max(rec["cover"]["all_ms"])
    # what came out: guards, the sum, the cover's bits
    assert int(deltas[-1].item()) == 0 and int(depth[-1].item()) == 0 and int(cover[-1].item()) == 0
    assert int(depth[:n_kmers].sum(dtype=torch.int64).item()) == rec["report"][1], "the depths sum to the positive k-mers"
    held = int((depth[:n_kmers] != 0).sum().item())
    rec["kmers_held"] = held
    rec["deepest"] = int(depth[:n_kmers].max().item())
    rec["nonzero_deltas"] = int((deltas[:n_kmers] != 0).sum().item())
    log(f"{name}: A {rec['counters']['ms']:.2f}  V {rec['cover']['ms']:.2f}  D {rec['depth']['ms']:.2f}  F {rec['finish']['ms']:.2f} ms; "
        f"{held} k-mers held, the deepest {rec['deepest']} times")

    sums = torch.full((d.num_strings() + 1,), -1, dtype=torch.int64, device=dev)

    def string_sums():
        d.depth_string_sums_device(0, depth.data_ptr(), sums.data_ptr(), sums.data_ptr() + 8 * d.num_strings(), stream=stream)

    rec["string_sums"] = entry(timed(string_sums, args.reps, args.warmup)[1], n_kmers)
    assert int(sums[-1].item()) == int(sums[:-1].sum().item()) == rec["report"][1]
    del cover, sums

    # ---- the route replaced, on the first `host_reads` reads: one id per base to the host, histogram there ----
    h = min(args.host_reads, n)
    if h:
        ids = torch.empty(h * L, dtype=torch.int64, device=dev)
        host_ids = torch.empty(h * L, dtype=torch.int64).pin_memory()
        all_ms = []
        held_ids = counts = None
        for i in range(1 + args.host_reps):
            ids.fill_(-1)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            d.streaming_lookup_device(0, reads.data_ptr(), offsets.data_ptr(), h, h * L, ids.data_ptr(), stream=stream)
            host_ids.copy_(ids)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            a = host_ids.numpy()
            held_ids, counts = np.unique(a[a >= 0], return_counts=True)  # (the histogram, sparse: an array of num_kmers counters would be 4 bytes a k-mer of host memory more)
            t2 = time.perf_counter()
            if i:
                all_ms.append({"lookup_and_copy_ms": (t1 - t0) * 1e3, "histogram_ms": (t2 - t1) * 1e3, "ms": (t2 - t0) * 1e3})
        deltas.zero_()

        def depth_and_finish():
            d.streaming_depth_device(0, reads.data_ptr(), offsets.data_ptr(), h, deltas.data_ptr(), stream=stream, total_bases=h * L)
            d.depth_finish_device(0, deltas.data_ptr(), depth.data_ptr(), stream=stream)

        depth_and_finish()
        torch.cuda.synchronize()
        at = torch.from_numpy(held_ids).to(dev)
        assert torch.equal(depth[at].to(torch.int64), torch.from_numpy(counts).to(dev)) and int(depth[:n_kmers].sum(dtype=torch.int64).item()) == int(counts.sum()), \
            "the histogram on the host against the depth"
        del at

        def from_zero():
            deltas.zero_()
            depth_and_finish()

        ms, all_device = timed(from_zero, args.host_reps, 1)  # (the zeroing of 4 bytes a k-mer is inside here: the host route's histogram is sparse and pays none)
        med = statistics.median(x["ms"] for x in all_ms)
        rec["host_histogram"] = {"reads": h, "kmers": h * (L - k + 1), "ms": med, "all": all_ms, "depth_zero_count_finish_ms": ms,
                                 "depth_zero_count_finish_all_ms": all_device, "speedup": med / ms}
        log(f"{name}: H over {h} reads: ids to the host and numpy.unique {med:.1f} ms; zero + depth + finish {ms:.2f} ms")
    del reads
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
    ap.add_argument("--host-reads", type=int, default=1_000_000, help="reads of the histogram-on-host route (0: skip it)")
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--bases", type=int, default=None, help="default: the workload's (bench.WORKLOADS)")
    ap.add_argument("--cache-dir", default=os.environ.get("SSHASH_BENCH_CACHE", "/tmp"))
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bench_streaming_depth needs a GPU")
    for name in args.configs:
        print(json.dumps(run_config(name, args)), flush=True)


if __name__ == "__main__":
    main()
