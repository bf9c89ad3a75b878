#!/usr/bin/env python
"""The streaming runs (sshash_streaming_runs_device: one record per search and the extensions behind it) on one MI355X beside the
calls it is built from and beside the only other route to the same information. Prints one JSON line per configuration:

    python tools/bench_streaming_runs.py c3 c4 [--reps 10] [--reads N] [--cache-dir DIR] [--tree DIR --label parent]

  A  counters     sshash_streaming_query_device: six counters for the batch
  C  per_read     sshash_streaming_query_per_read_device: rows + totals
  R0 runs_count   sshash_streaming_runs_device, the counting call (runs = NULL): run_offsets + totals
  R  runs         sshash_streaming_runs_device, capacity sufficient: run_offsets + records + totals; records written and their bytes
  D  lookup_full  sshash_streaming_lookup_device asking for kmer_id, string_id, kmer_id_in_string, kmer_orientation: one result per base,
                  without the compaction a caller would still have to do

A and C exist in a build of the commit before the runs too (--tree DIR --label parent: the package and its library are imported from
that checkout), R0 and R only where the library has the call. Every figure: median of --reps event-timed calls after --warmup, with
all of them listed; k-mers/s = the reads' k-mers / that. Read sets and dictionaries: those of tools/bench_streaming_per_read.py."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_streaming_per_read import POSITIVE, timed  # noqa: E402


def log(msg):
    print(f"[bench_streaming_runs] {msg}", file=sys.stderr, flush=True)


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
    log(f"{name}: A counters {rec['counters']['ms']:.2f} ms")

    searches = None
    if "per_read" in args.only:
        rows = torch.full((n, 6), -1, dtype=torch.int64, device=dev)

        def per_read():
            report.zero_()
            d.streaming_query_per_read_device(0, reads.data_ptr(), offsets.data_ptr(), n, rows.data_ptr(), d_report=report.data_ptr(),
                                              stream=stream, total_bases=n * L)

        rec["per_read"] = entry(*timed(per_read, args.reps, args.warmup))
        assert torch.equal(rows.sum(0), totals) and torch.equal(report, totals)
        searches = rows[:, 4].clone()
        del rows
        log(f"{name}: C per_read {rec['per_read']['ms']:.2f} ms")

    if hasattr(d, "streaming_runs_device") and "runs" in args.only:
        run_offsets = torch.full((n + 1,), -1, dtype=torch.int64, device=dev)

        def runs_count():
            report.zero_()
            d.streaming_runs_device(0, reads.data_ptr(), offsets.data_ptr(), n, run_offsets.data_ptr(), 0, 0, d_report=report.data_ptr(),
                                    stream=stream, total_bases=n * L)

        rec["runs_count"] = entry(*timed(runs_count, args.reps, args.warmup))
        total_runs = int(run_offsets[-1].item())
        assert torch.equal(report, totals) and total_runs == rec["report"][4]
        if searches is not None:
            assert torch.equal(run_offsets[1:] - run_offsets[:-1], searches), "runs per read != num_searches of the per-read rows"
        log(f"{name}: R0 runs, counting call {rec['runs_count']['ms']:.2f} ms; {total_runs} runs, {total_runs / n:.2f} a read")
        records = torch.zeros((total_runs + 1, 4), dtype=torch.int64, device=dev)
        run_offsets.fill_(-1)

        def runs():
            report.zero_()
            d.streaming_runs_device(0, reads.data_ptr(), offsets.data_ptr(), n, run_offsets.data_ptr(), records.data_ptr(), total_runs,
                                    d_report=report.data_ptr(), stream=stream, total_bases=n * L)

        rec["runs"] = entry(*timed(runs, args.reps, args.warmup))
        lengths = (records[:total_runs, 3] >> 32) & 0x7FFFFFFF
        assert torch.equal(report, totals) and int(run_offsets[-1].item()) == total_runs and int(lengths.sum().item()) == rec["report"][1]
        rec["records"] = total_runs
        rec["record_bytes"] = 32 * total_runs
        rec["runs_per_read"] = total_runs / n
        log(f"{name}: R runs {rec['runs']['ms']:.2f} ms, {32 * total_runs / 1e9:.2f} GB of records")
        del records, run_offsets, lengths

    if "lookup_full" in args.only:
        ids = torch.empty(n * L, dtype=torch.int64, device=dev)
        sid = torch.empty(n * L, dtype=torch.int64, device=dev)
        kis = torch.empty(n * L, dtype=torch.int64, device=dev)
        ori = torch.empty(n * L, dtype=torch.int8, device=dev)

        def lookup_full():
            d.streaming_lookup_device(0, reads.data_ptr(), offsets.data_ptr(), n, n * L, ids.data_ptr(), stream=stream, string_id=sid.data_ptr(),
                                      kmer_id_in_string=kis.data_ptr(), kmer_orientation=ori.data_ptr())

        rec["lookup_full"] = entry(*timed(lookup_full, args.reps, args.warmup))
        assert int((ids.view(n, L)[:, :L - k + 1] != -1).sum().item()) == rec["report"][1]
        log(f"{name}: D lookup, four fields {rec['lookup_full']['ms']:.2f} ms")
        del ids, sid, kis, ori
        if "runs" in rec:
            rec["runs_over_lookup_full"] = rec["lookup_full"]["ms"] / rec["runs"]["ms"]
    if "runs" in rec and "per_read" in rec:
        rec["runs_over_per_read"] = rec["runs"]["ms"] / rec["per_read"]["ms"]
        rec["runs_count_over_per_read"] = rec["runs_count"]["ms"] / rec["per_read"]["ms"]
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
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--bases", type=int, default=None, help="default: the workload's (bench.WORKLOADS)")
    ap.add_argument("--cache-dir", default=os.environ.get("SSHASH_BENCH_CACHE", "/tmp"))
    ap.add_argument("--tree", default=ROOT, help="the checkout whose sshash_amd package and library are measured (default: this one)")
    ap.add_argument("--label", default="this", help="names the lines of this run")
    ap.add_argument("--only", default="per_read,runs,lookup_full", help="which of per_read, runs, lookup_full to measure beside counters")
    args = ap.parse_args()
    args.only = args.only.split(",")
    sys.path.insert(0, os.path.abspath(args.tree))
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bench_streaming_runs needs a GPU")
    import sshash_amd

    log(f"package: {os.path.dirname(sshash_amd.__file__)}")
    for name in args.configs:
        print(json.dumps(run_config(name, args)), flush=True)


if __name__ == "__main__":
    main()
