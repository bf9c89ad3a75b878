#!/usr/bin/env python
"""The streaming sums (sshash_value_prefix_device + sshash_streaming_sums_device: per read, the sum of a value per k-mer over the read's
positive k-mers, and their number) on one MI355X beside the forms of the run kernel it stands next to. Prints one JSON line per
configuration:

    python tools/bench_streaming_sums.py c3 c4 [--reps 10] [--reads N] [--existing-only] [--cache-dir DIR]

  A  counters   sshash_streaming_query_device: six counters for the batch
  R  per_read   sshash_streaming_query_per_read_device: one report per read (48 bytes a read)
  D  depth      sshash_streaming_depth_device into ZEROED deltas: deltas + totals (no finish)
  U  sums       sshash_streaming_sums_device over the prefix of random values in [0, 1000): 16 bytes a read + totals
  P  prefix     sshash_value_prefix_device alone: num_kmers uint32 -> num_kmers + 1 uint64

The forms ALTERNATE inside one loop of one process (A R D U P, A R D U P, ...), so that a drift of the machine falls on all of them alike;
the zeroing is outside the timed regions. Every figure: median of --reps event-timed calls after --warmup rounds, with all of them listed;
k-mers/s = the reads' k-mers / that. --existing-only leaves U and P out: the same tool then runs against a build that does not have them
yet (the parent commit's, on the same box: the yardstick for "nothing existing moved" and the denominator of the sums form's cost).
Read sets and dictionaries: those of tools/bench_streaming_depth.py."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_streaming_per_read import POSITIVE  # noqa: E402


CHUNK = 1 << 28  # elements of a device array handled at a time outside the timed regions


def log(msg):
    print(f"[bench_streaming_sums] {msg}", file=sys.stderr, flush=True)


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
    n, L, k, n_kmers = args.reads, args.read_len, d.k(), d.num_kmers()
    reads = make_reads_device(d, 0, n, L, positive_fraction=POSITIVE[name], seed=ns.seed)
    offsets = torch.arange(n + 1, dtype=torch.int64, device=dev) * L
    report = torch.zeros(6, dtype=torch.int64, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    kmers = n * (L - k + 1)
    rec = {"config": name, "k": k, "num_kmers_of_the_dictionary": n_kmers, "reads": n, "read_len": L, "positive_fraction_of_reads": POSITIVE[name],
           "kmers_per_call": kmers, "reps": args.reps, "existing_only": bool(args.existing_only), "build": args.label}

    def entry(all_ms, per=kmers):
        ms = statistics.median(all_ms)
        return {"ms": ms, "all_ms": all_ms, "gkmers_per_s": per / ms / 1e6, "spread": (max(all_ms) - min(all_ms)) / ms}

    rows = torch.zeros(6 * n + 1, dtype=torch.int64, device=dev)      # (a guard word behind the last, here and below)
    deltas = torch.zeros(n_kmers + 1, dtype=torch.int32, device=dev)

    def counters():
        d.streaming_query_device(0, reads.data_ptr(), offsets.data_ptr(), n, report.data_ptr(), stream=stream, total_bases=n * L)

    def per_read():
        d.streaming_query_per_read_device(0, reads.data_ptr(), offsets.data_ptr(), n, rows.data_ptr(), d_report=report.data_ptr(), stream=stream, total_bases=n * L)

    def depth_form():
        d.streaming_depth_device(0, reads.data_ptr(), offsets.data_ptr(), n, deltas.data_ptr(), d_report=report.data_ptr(), stream=stream, total_bases=n * L)

    forms = [("counters", counters, lambda: None), ("per_read", per_read, lambda: None), ("depth", depth_form, deltas.zero_)]
    if not args.existing_only:
        values = torch.empty(n_kmers + 1, dtype=torch.int32, device=dev)
        gen = torch.Generator(device=dev).manual_seed(7)
        for a in range(0, n_kmers + 1, CHUNK):
            b = min(n_kmers + 1, a + CHUNK)
            values[a:b] = torch.randint(0, 1000, (b - a,), dtype=torch.int32, device=dev, generator=gen)
        prefix = torch.zeros(n_kmers + 2, dtype=torch.int64, device=dev)
        sums = torch.full((2 * n + 1,), -1, dtype=torch.int64, device=dev)
        sums[-1] = 0
        d.value_prefix_device(0, values.data_ptr(), prefix.data_ptr(), stream=stream)
        torch.cuda.synchronize()
        rec["prefix_bytes"] = 8 * (n_kmers + 1)

        def sums_form():
            d.streaming_sums_device(0, reads.data_ptr(), offsets.data_ptr(), n, prefix.data_ptr(), sums.data_ptr(), d_report=report.data_ptr(), stream=stream,
                                    total_bases=n * L)

        def prefix_alone():
            d.value_prefix_device(0, values.data_ptr(), prefix.data_ptr(), stream=stream)

        forms += [("sums", sums_form, lambda: None), ("prefix", prefix_alone, lambda: None)]
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
            if name_ != "prefix":
                assert torch.equal(report, totals), name_
    for name_ in times:
        rec[name_] = entry(times[name_], n_kmers if name_ == "prefix" else kmers)
    rec["report"] = [int(v) for v in totals.cpu().tolist()]
    rec["per_read_over_counters"] = rec["per_read"]["ms"] / rec["counters"]["ms"]
    # what came out: guards, the column sums
    assert int(rows[-1].item()) == 0 and int(deltas[-1].item()) == 0
    assert int(rows[:-1].view(n, 6)[:, 1].sum().item()) == rec["report"][1]
    line = f"{name}: A {rec['counters']['ms']:.2f}  R {rec['per_read']['ms']:.2f}  D {rec['depth']['ms']:.2f}"
    if not args.existing_only:
        rec["prefix"]["ms_per_1e9_kmers"] = rec["prefix"]["ms"] * 1e9 / n_kmers
        rec["sums_over_per_read"] = rec["sums"]["ms"] / rec["per_read"]["ms"]
        rec["sums_over_counters"] = rec["sums"]["ms"] / rec["counters"]["ms"]
        rec["sums_over_depth"] = rec["sums"]["ms"] / rec["depth"]["ms"]
        pairs = sums[:-1].view(n, 2)
        assert int(sums[-1].item()) == 0 and int(prefix[-1].item()) == 0 and int(prefix[0].item()) == 0
        assert torch.equal(pairs[:, 1], rows[:-1].view(n, 6)[:, 1]), "positive_kmers against column 1 of the per-read rows"
        assert int(prefix[n_kmers].item()) == int(values[:n_kmers].sum(dtype=torch.int64).item()), "the last word of the prefix is the total"
        # (the depth's deltas of the last round, finished, weigh every id by how often the reads hold it: the rows' sums add up to that)
        d.depth_finish_device(0, deltas.data_ptr(), deltas.data_ptr(), stream=stream)
        weighed = 0
        for a in range(0, n_kmers, CHUNK):
            b = min(n_kmers, a + CHUNK)
            weighed += int((deltas[a:b].to(torch.int64) * values[a:b].to(torch.int64)).sum().item())
        assert int(pairs[:, 0].sum().item()) == weighed, "the sums against depth x values"
        rec["reads_with_a_hit"] = int((pairs[:, 1] != 0).sum().item())
        rec["mean_sum_per_positive_kmer"] = float(pairs[:, 0].sum().item()) / max(1, rec["report"][1])
        line += f"  U {rec['sums']['ms']:.2f}  P {rec['prefix']['ms']:.2f}"
    log(line + " ms")
    del reads, rows, deltas
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
    ap.add_argument("--existing-only", action="store_true", help="counters, per-read and depth only: for a build without the sums")
    ap.add_argument("--label", default="this", help="which build of the library this is, for the record (e.g. parent)")
    ap.add_argument("--cache-dir", default=os.environ.get("SSHASH_BENCH_CACHE", "/tmp"))
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bench_streaming_sums needs a GPU")
    for name in args.configs:
        print(json.dumps(run_config(name, args)), flush=True)


if __name__ == "__main__":
    main()
