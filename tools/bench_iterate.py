#!/usr/bin/env python
"""The k-mer iterator on one MI355X (sshash_iterate_packed_device) over a whole dictionary, beside what bounds it, and the
whole-index check built on it (sshash_check_device). Prints one JSON line per config:

    python tools/bench_iterate.py c3 c4 [--reps 10] [--cache-dir DIR]

  iterate_device        kmers_device(0, num_kmers): median of --reps event-timed calls after --warmup; G k-mers/s and
                        bytes/s of (blocks of bases read + endpoints read + words written)
  access_packed_device  access_packed_device over arange(num_kmers) into the same buffer (the random-access way to the same
                        output: ids read, one binary search per k-mer)
  fill                  a fill of the output buffer (writes only): the store bound of the words the iterator writes
  d2d_copy              a device-to-device copy of the output's size (read + write), counted as read + written bytes
  check                 wall time of Dictionary.check(0), and its counts

The dictionaries are bench.py's C3 / C4 stand-ins (same recipes, seed and cache key: a dictionary bench.py cached under
--cache-dir is loaded, not rebuilt). Kernel times come from a separate `rocprofv3 --kernel-trace --stats` run of this tool.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def log(msg):
    print(f"[bench_iterate] {msg}", file=sys.stderr, flush=True)


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
    import numpy as np
    import torch

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
    n, W, k = d.num_kmers(), d.words_per_kmer(), d.k()
    stream = torch.cuda.current_stream().cuda_stream
    dev = torch.device("cuda", 0)
    out_bytes = n * W * 8
    # atoms of 32 bytes per 32 bases (k <= 31, each also carries the next block) or granules of 16 bytes per 32 bases
    read_bytes = d.num_bases() * (32 if k <= 31 else 16) // 32 + 8 * d.num_strings()
    rec = {"config": name, "k": k, "num_kmers": n, "num_strings": d.num_strings(), "num_bases": d.num_bases(),
           "words_per_kmer": W, "bytes_read": read_bytes, "bytes_written": out_bytes, "reps": args.reps}

    out = torch.empty(n * W, dtype=torch.int64, device=dev)
    ms, all_ms = timed(lambda: d.kmers_device(0, 0, n, out.data_ptr(), stream=stream), args.reps, args.warmup)
    rec["iterate_device"] = {"ms": ms, "all_ms": all_ms, "gkmers_per_s": n / ms / 1e6,
                             "gbytes_per_s": (read_bytes + out_bytes) / ms / 1e6}
    # spot check against the host iterator (first, last and a middle window)
    for b in (0, n // 2, max(0, n - 100_000)):
        e = min(n, b + 100_000)
        assert np.array_equal(out[b * W:e * W].cpu().numpy().view(np.uint64), d.kmers(b, e)), (name, b)
    log(f"{name}: iterate {ms:.2f} ms")

    ids = torch.arange(n, dtype=torch.int64, device=dev)
    ms, all_ms = timed(lambda: d.access_packed_device(0, ids.data_ptr(), n, out.data_ptr(), stream=stream), args.reps, args.warmup)
    rec["access_packed_device"] = {"ms": ms, "all_ms": all_ms, "gkmers_per_s": n / ms / 1e6}
    del ids
    log(f"{name}: access {ms:.2f} ms")

    ms, all_ms = timed(lambda: out.fill_(-1), args.reps, args.warmup)
    rec["fill"] = {"ms": ms, "all_ms": all_ms, "bytes": out_bytes, "gbytes_per_s": out_bytes / ms / 1e6}
    dst = torch.empty_like(out)
    ms, all_ms = timed(lambda: dst.copy_(out), args.reps, args.warmup)
    rec["d2d_copy"] = {"ms": ms, "all_ms": all_ms, "bytes": 2 * out_bytes, "gbytes_per_s": 2 * out_bytes / ms / 1e6}
    del dst, out
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    rec["iterate_over_copy_byte_rate"] = rec["iterate_device"]["gbytes_per_s"] / rec["d2d_copy"]["gbytes_per_s"]
    rec["iterate_writes_over_fill"] = rec["fill"]["ms"] / rec["iterate_device"]["ms"]
    rec["iterate_over_access_rate"] = rec["iterate_device"]["gkmers_per_s"] / rec["access_packed_device"]["gkmers_per_s"]

    if not args.no_check:
        t0 = time.time()
        counts = d.check(0)
        rec["check"] = {"wall_s": time.time() - t0, **counts}
        log(f"{name}: check {rec['check']['wall_s']:.2f} s {counts}")
    d.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("configs", nargs="+", choices=["c2", "c3", "c4"])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--bases", type=int, default=None, help="default: the workload's (bench.WORKLOADS)")
    ap.add_argument("--cache-dir", default=os.environ.get("SSHASH_BENCH_CACHE", "/tmp"))
    ap.add_argument("--no-check", action="store_true")
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bench_iterate needs a GPU")
    for name in args.configs:
        print(json.dumps(run_config(name, args)), flush=True)


if __name__ == "__main__":
    main()
