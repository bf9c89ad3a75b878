#!/usr/bin/env python
"""The streaming cover (sshash_streaming_cover_device: which k-mers of the dictionary a read set holds, as a bitmap) on one MI355X beside
the calls a caller had to take for the same answer before it. Prints one JSON line per configuration:

    python tools/bench_streaming_cover.py c3 c4 [--reps 10] [--reads N] [--cache-dir DIR] [--tree DIR --label parent]

  A  counters       sshash_streaming_query_device: six counters for the batch
  C  per_read       sshash_streaming_query_per_read_device: rows + totals
  R  runs           sshash_streaming_runs_device, capacity sufficient: run_offsets + records + totals -- the least a caller paid before
                    it could mark a single bit
  V  cover          sshash_streaming_cover_device into a ZEROED bitmap (the zeroing is outside the timed region): bitmap + totals
  V2 cover_again    the same call into the bitmap V left: every bit it would set is set already -- the deep-sample case
  S  string_counts  sshash_cover_string_counts_device over that bitmap: covered k-mers per string and in all

A, C and R exist in a build of the commit before the cover too (--tree DIR --label parent: the package and its library are imported from
that checkout), V, V2 and S only where the library has the calls. Every figure: median of --reps event-timed calls after --warmup, with
all of them listed; k-mers/s = the reads' k-mers / that. Read sets and dictionaries: those of tools/bench_streaming_runs.py."""
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
    print(f"[bench_streaming_cover] {msg}", file=sys.stderr, flush=True)


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
    rec = {"config": name, "label": args.label, "k": k, "num_kmers_of_the_dictionary": d.num_kmers(), "num_strings": d.num_strings(), "reads": n,
           "read_len": L, "positive_fraction_of_reads": POSITIVE[name], "kmers_per_call": kmers, "reps": args.reps}

    def entry(ms, all_ms):
        return {"ms": ms, "all_ms": all_ms, "gkmers_per_s": kmers / ms / 1e6, "spread": (max(all_ms) - min(all_ms)) / ms}

    def counters():
        report.zero_()
        d.streaming_query_device(0, reads.data_ptr(), offsets.data_ptr(), n, report.data_ptr(), stream=stream, total_bases=n * L)

    rec["counters"] = entry(*timed(counters, args.reps, args.warmup))
    totals = report.clone()
    rec["report"] = [int(v) for v in totals.cpu().tolist()]
    log(f"{name}: A counters {rec['counters']['ms']:.2f} ms")

    if "per_read" in args.only:
        rows = torch.full((n, 6), -1, dtype=torch.int64, device=dev)

        def per_read():
            report.zero_()
            d.streaming_query_per_read_device(0, reads.data_ptr(), offsets.data_ptr(), n, rows.data_ptr(), d_report=report.data_ptr(),
                                              stream=stream, total_bases=n * L)

        rec["per_read"] = entry(*timed(per_read, args.reps, args.warmup))
        assert torch.equal(rows.sum(0), totals) and torch.equal(report, totals)
        del rows
        log(f"{name}: C per_read {rec['per_read']['ms']:.2f} ms")

    total_runs = rec["report"][4]  # (a run is a search and the extensions behind it)
    if "runs" in args.only:
        run_offsets = torch.full((n + 1,), -1, dtype=torch.int64, device=dev)
        records = torch.zeros((total_runs + 1, 4), dtype=torch.int64, device=dev)

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
        # the words a cover call touches with an atomic (a run's first and last word) and with a plain store (those in between)
        ids = records[:total_runs, 0]
        count = lengths
        backward = (records[:total_runs, 3] >> 63) != 0
        lo = torch.where(backward, ids + 1 - count, ids)
        spanned = ((lo + count - 1) >> 6) - (lo >> 6) + 1
        rec["cover_words_per_run"] = float(spanned.double().mean().item())
        rec["cover_atomics_per_run"] = float(spanned.clamp(max=2).double().mean().item())
        log(f"{name}: R runs {rec['runs']['ms']:.2f} ms, {total_runs} runs ({total_runs / n:.2f} a read), {rec['cover_words_per_run']:.2f} bitmap words a run")
        del records, run_offsets, lengths, ids, count, backward, lo, spanned

    if hasattr(d, "streaming_cover_device") and "cover" in args.only:
        words = d.cover_words()
        cover = torch.zeros(words + 1, dtype=torch.int64, device=dev)  # (a guard word behind the last)
        rec["cover_bytes"] = 8 * words

        def timed_from_zero(reps, warmup):
            """`timed`, with the bitmap zeroed before every call, outside the events"""
            times = []
            for i in range(warmup + reps):
                cover.zero_()
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                report.zero_()  # (inside the timed region, as in the other rows)
                d.streaming_cover_device(0, reads.data_ptr(), offsets.data_ptr(), n, cover.data_ptr(), d_report=report.data_ptr(), stream=stream,
                                         total_bases=n * L)
                e1.record()
                e1.synchronize()
                if i >= warmup:
                    times.append(e0.elapsed_time(e1))
            return statistics.median(times), times

        rec["cover"] = entry(*timed_from_zero(args.reps, args.warmup))
        assert torch.equal(report, totals) and int(cover[-1].item()) == 0
        first = cover.clone()
        log(f"{name}: V cover {rec['cover']['ms']:.2f} ms into {8 * words / 1e6:.0f} MB")

        def cover_again():
            report.zero_()
            d.streaming_cover_device(0, reads.data_ptr(), offsets.data_ptr(), n, cover.data_ptr(), d_report=report.data_ptr(), stream=stream,
                                     total_bases=n * L)

        rec["cover_again"] = entry(*timed(cover_again, args.reps, args.warmup))
        assert torch.equal(report, totals) and torch.equal(cover, first), "a second pass over the same reads changed the bitmap"
        log(f"{name}: V2 cover, every bit already set {rec['cover_again']['ms']:.2f} ms")
        del first

        counts = torch.full((d.num_strings() + 1,), -1, dtype=torch.int64, device=dev)

        def string_counts():
            d.cover_string_counts_device(0, cover.data_ptr(), counts.data_ptr(), counts.data_ptr() + 8 * d.num_strings(), stream=stream)

        rec["string_counts"] = entry(*timed(string_counts, args.reps, args.warmup))
        total = int(counts[-1].item())
        assert int(counts[:-1].sum().item()) == total and 0 < total <= rec["report"][1]
        rec["covered_kmers"] = total
        rec["covered_strings"] = int((counts[:-1] > 0).sum().item())
        rec["string_counts"]["bitmap_gb_per_s"] = 8 * words / rec["string_counts"]["ms"] / 1e6
        log(f"{name}: S string counts {rec['string_counts']['ms']:.2f} ms; {total} k-mers covered in {rec['covered_strings']} strings")
        del cover, counts
        if "runs" in rec:
            rec["cover_over_runs"] = rec["cover"]["ms"] / rec["runs"]["ms"]
        rec["cover_over_counters"] = rec["cover"]["ms"] / rec["counters"]["ms"]
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
    ap.add_argument("--only", default="per_read,runs,cover", help="which of per_read, runs, cover to measure beside counters")
    args = ap.parse_args()
    args.only = args.only.split(",")
    sys.path.insert(0, os.path.abspath(args.tree))
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bench_streaming_cover needs a GPU")
    import sshash_amd

    log(f"package: {os.path.dirname(sshash_amd.__file__)}")
    for name in args.configs:
        print(json.dumps(run_config(name, args)), flush=True)


if __name__ == "__main__":
    main()
