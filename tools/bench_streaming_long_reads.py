#!/usr/bin/env python
"""Long reads cut into segments for the run kernel (sshash_set_read_segments) on one MI355X: the same total of bases as reads of 150,
10,000 and 2^20 bases, through the device calls with segments off and on, and through the host call with SSHASH_SEGMENTS_OFF against
segments. Prints one JSON line per configuration and read length:

    python tools/bench_streaming_long_reads.py c3 c4 [--segments 256 1024 4096] [--read-lens 150 10000 1048576] [--reps 5]
                                               [--total-bases N] [--host-bases N] [--cache-dir DIR]

  counters   sshash_streaming_query_device: six counters for the batch          -- off, and with every S of --segments
  depth      sshash_streaming_depth_device into ZEROED deltas: deltas + totals  -- off, and with every S
  host       sshash_streaming_query over the first --host-bases bases (pageable host memory in, six counters out)
             -- SSHASH_SEGMENTS_OFF (a piece that holds a read above 2^16 bases takes the position-parallel pipeline), and every S

All device forms ALTERNATE inside one loop of one process (counters off, counters S1, ..., depth off, depth S1, ..., and again), and so do
the host forms in a loop of their own, so that a drift of the machine falls on all of them alike; zeroing is outside the timed regions.
Every figure: median of --reps timed calls (events on the device, the wall clock around the host call) after --warmup rounds, with all of
them listed; k-mers/s = the reads' k-mers / that. The six counters of every form, and the deltas of every depth form, must equal those
of the form without segments: the tool stops otherwise. Read sets and dictionaries: those of tools/bench_streaming_depth.py."""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_streaming_per_read import POSITIVE  # noqa: E402


def log(msg):
    print(f"[bench_streaming_long_reads] {msg}", file=sys.stderr, flush=True)


def entry(all_ms, kmers):
    ms = statistics.median(all_ms)
    return {"ms": ms, "all_ms": all_ms, "gkmers_per_s": kmers / ms / 1e6, "spread": (max(all_ms) - min(all_ms)) / ms}


def run_length(d, name, L, args, seed):
    import numpy as np
    import torch

    import sshash_amd
    from sshash_amd import _binding as B
    from sshash_amd.synthetic import make_reads_device

    dev = torch.device("cuda", 0)
    k, n_kmers = d.k(), d.num_kmers()
    n = max(1, args.total_bases // L)
    reads = make_reads_device(d, 0, n, L, positive_fraction=POSITIVE[name], seed=seed)
    offsets = torch.arange(n + 1, dtype=torch.int64, device=dev) * L
    report = torch.zeros(6, dtype=torch.int64, device=dev)
    deltas = torch.zeros(n_kmers + 1, dtype=torch.int32, device=dev)  # (a guard word behind the last)
    stream = torch.cuda.current_stream().cuda_stream
    kmers = n * (L - k + 1)
    rec = {"config": name, "k": k, "num_kmers_of_the_dictionary": n_kmers, "reads": n, "read_len": L, "positive_fraction_of_reads": POSITIVE[name],
           "kmers_per_call": kmers, "reps": args.reps, "segments": args.segments}

    def counters():
        d.streaming_query_device(0, reads.data_ptr(), offsets.data_ptr(), n, report.data_ptr(), stream=stream, total_bases=n * L)

    def depth():
        d.streaming_depth_device(0, reads.data_ptr(), offsets.data_ptr(), n, deltas.data_ptr(), d_report=report.data_ptr(), stream=stream, total_bases=n * L)

    settings = [("off", sshash_amd.SEGMENTS_OFF)] + [(f"S{S}", S) for S in args.segments]
    forms = [(f"{what}_{label}", fn, S) for what, fn in (("counters", counters), ("depth", depth)) for label, S in settings]
    times = {form: [] for form, _, _ in forms}
    totals = want_deltas = None
    for i in range(args.warmup + args.reps):
        for form, fn, S in forms:
            d.set_read_segments(S, device_calls=True)
            report.zero_()
            deltas.zero_()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if i >= args.warmup:
                times[form].append(e0.elapsed_time(e1))
            if i == 0:  # identical outputs, at the timed size
                totals = report.clone() if totals is None else totals
                assert torch.equal(report, totals), (form, report.tolist(), totals.tolist())
                if fn is depth:
                    want_deltas = deltas.clone() if want_deltas is None else want_deltas
                    assert torch.equal(deltas, want_deltas), form
                    assert int(deltas[-1].item()) == 0
    for form in times:
        rec[form] = entry(times[form], kmers)
    rec["report"] = [int(v) for v in totals.cpu().tolist()]
    rec["segmented_launches"] = d.read_segments()["segmented_launches"]
    log(f"{name} L={L}: " + "  ".join(f"{form} {rec[form]['ms']:.2f}" for form in times) + " ms")
    del deltas, want_deltas

    # ---- the host call, over the first --host-bases bases ----
    h = max(1, min(n, args.host_bases // L))
    host_bases = reads[:h].reshape(-1).cpu().numpy()
    host_offsets = (np.arange(h + 1, dtype=np.uint64) * np.uint64(L))
    del reads
    torch.cuda.empty_cache()
    lib = B._load()
    host_kmers = h * (L - k + 1)
    host_times = {label: [] for label, _ in settings}
    host_totals = None
    for i in range(args.host_warmup + args.host_reps):
        for label, S in settings:
            d.set_read_segments(S)
            r = B._Report()
            t0 = time.perf_counter()
            status = lib.sshash_streaming_query(d._h, host_bases.ctypes.data, host_offsets.ctypes.data, h, C.byref(r))
            t1 = time.perf_counter()
            assert status == 0, status
            got = [r.num_kmers, r.num_positive_kmers, r.num_negative_kmers, r.num_invalid_kmers, r.num_searches, r.num_extensions]
            host_totals = got if host_totals is None else host_totals
            assert got == host_totals, (label, got, host_totals)
            if i >= args.host_warmup:
                host_times[label].append((t1 - t0) * 1e3)
    rec["host"] = {"reads": h, "kmers": host_kmers, "report": host_totals, **{label: entry(host_times[label], host_kmers) for label in host_times}}
    log(f"{name} L={L}: host over {h} reads: " + "  ".join(f"{label} {rec['host'][label]['ms']:.1f}" for label in host_times) + " ms")
    d.set_read_segments(sshash_amd.SEGMENTS_OFF)
    return rec


def run_config(name, args):
    import bench
    from sshash_amd.repeats import load_recipe

    bases, recipe, _, _ = bench.WORKLOADS[name]
    r = load_recipe(recipe)
    ns = argparse.Namespace(bases=args.bases or bases, k=int(r["k"]), m=int(r["m"]), canonical=False, seed=0x5555AAAA,
                            recipe=recipe, repeat_scale=1.0, cache_dir=args.cache_dir, verbose=False)
    d, _ = bench.get_index(ns, 0, 1, lambda: None)
    t0 = time.time()
    d.to_device(0)
    log(f"{name}: uploaded in {time.time() - t0:.1f}s")
    for L in args.read_lens:
        print(json.dumps(run_length(d, name, L, args, ns.seed)), flush=True)
    d.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("configs", nargs="+", choices=["c3", "c4"])
    ap.add_argument("--segments", type=int, nargs="+", default=[256, 1024, 4096], help="segment lengths S in k-mers")
    ap.add_argument("--read-lens", type=int, nargs="+", default=[150, 10_000, 1 << 20])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--host-warmup", type=int, default=1)
    ap.add_argument("--total-bases", type=int, default=3_000_000_000, help="bases of the read set (the other streaming tools: 2 x 10^7 reads of 150)")
    ap.add_argument("--host-bases", type=int, default=1 << 28, help="bases of the host call's batch")
    ap.add_argument("--bases", type=int, default=None, help="bases of the dictionary (default: the workload's, bench.WORKLOADS)")
    ap.add_argument("--cache-dir", default=os.environ.get("SSHASH_BENCH_CACHE", "/tmp"))
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bench_streaming_long_reads needs a GPU")
    for name in args.configs:
        run_config(name, args)


if __name__ == "__main__":
    main()
