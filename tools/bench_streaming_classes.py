#!/usr/bin/env python
"""The streaming classes (sshash_streaming_classes_device: per read, its positive k-mers by class of string) on one MI355X beside the
forms of the run kernel it stands next to and beside the route it replaces. Prints one JSON line per configuration:

    python tools/bench_streaming_classes.py c3 c4 [--reps 10] [--reads N] [--classes 4 64 1024] [--existing-only] [--cache-dir DIR]

  A  counters      sshash_streaming_query_device: six counters for the batch
  U  sums          sshash_streaming_sums_device over the prefix of random values in [0, 1000): 16 bytes a read + totals
  and for every C of --classes, labels = string id mod C:
  K  classes       sshash_streaming_classes_device: the rows (n x C words of 32 bits) zeroed inside the call, one launch
  M  memset        the zeroing alone: the call's own hipMemsetAsync over the same n x C x 4 bytes, on the same stream
  X  runs route    what a caller did before: sshash_streaming_runs_device (count, scan, write: 32 bytes a run), then the records into the
                   same zeroed matrix with torch -- the read of every run out of run_offsets (repeat_interleave), labels[string_id],
                   one scatter-add of the lengths

The forms ALTERNATE inside one loop of one process, so that a drift of the machine falls on all of them alike. Every figure: median of
--reps event-timed calls after --warmup rounds, with all of them listed; k-mers/s = the reads' k-mers / that. --existing-only keeps A and
U: the same tool then runs against a build that does not have the classes yet (the parent commit's package, on the same box, through
--package-dir: the yardstick for "nothing existing moved"). In the first round the rows of K and X are compared word for word and
their sum, the sum of class_totals_device and the sum of class_best_device's totals with the report's positive k-mers. Read sets and
dictionaries: those of tools/bench_streaming_sums.py."""
from __future__ import annotations

import argparse
import ctypes
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
    print(f"[bench_streaming_classes] {msg}", file=sys.stderr, flush=True)


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
    n, L, k, n_kmers, n_strings = args.reads, args.read_len, d.k(), d.num_kmers(), d.num_strings()
    reads = make_reads_device(d, 0, n, L, positive_fraction=POSITIVE[name], seed=ns.seed)
    offsets = torch.arange(n + 1, dtype=torch.int64, device=dev) * L
    report = torch.zeros(6, dtype=torch.int64, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    kmers = n * (L - k + 1)
    rec = {"config": name, "k": k, "num_kmers_of_the_dictionary": n_kmers, "num_strings": n_strings, "reads": n, "read_len": L,
           "positive_fraction_of_reads": POSITIVE[name], "kmers_per_call": kmers, "reps": args.reps, "existing_only": bool(args.existing_only),
           "build": args.label}

    def entry(all_ms):
        ms = statistics.median(all_ms)
        return {"ms": ms, "lowest_ms": min(all_ms), "highest_ms": max(all_ms), "all_ms": all_ms, "gkmers_per_s": kmers / ms / 1e6}

    values = torch.empty(n_kmers + 1, dtype=torch.int32, device=dev)
    gen = torch.Generator(device=dev).manual_seed(7)
    for a in range(0, n_kmers + 1, CHUNK):
        b = min(n_kmers + 1, a + CHUNK)
        values[a:b] = torch.randint(0, 1000, (b - a,), dtype=torch.int32, device=dev, generator=gen)
    prefix = torch.zeros(n_kmers + 2, dtype=torch.int64, device=dev)
    sums = torch.zeros(2 * n + 1, dtype=torch.int64, device=dev)
    d.value_prefix_device(0, values.data_ptr(), prefix.data_ptr(), stream=stream)
    torch.cuda.synchronize()
    del values

    def counters():
        d.streaming_query_device(0, reads.data_ptr(), offsets.data_ptr(), n, report.data_ptr(), stream=stream, total_bases=n * L)

    def sums_form():
        d.streaming_sums_device(0, reads.data_ptr(), offsets.data_ptr(), n, prefix.data_ptr(), sums.data_ptr(), d_report=report.data_ptr(), stream=stream,
                                total_bases=n * L)

    nothing = lambda: None
    forms = [("counters", counters, True, nothing, nothing), ("sums", sums_form, True, nothing, nothing)]  # (name, call, fills the report, before, after)
    if not args.existing_only:
        # the runs of the read set: counted once, outside the timed regions, to size the records
        run_offsets = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        d.streaming_runs_device(0, reads.data_ptr(), offsets.data_ptr(), n, run_offsets.data_ptr(), 0, 0, stream=stream, total_bases=n * L)
        torch.cuda.synchronize()
        n_runs = int(run_offsets[n].item())
        rec["runs"] = n_runs
        records = torch.zeros(4 * n_runs + 4, dtype=torch.int64, device=dev)  # (32 bytes a record: kmer_id, string_id, kmer_id_in_string, read_pos | num_kmers << 32)
        read_ids = torch.arange(n, dtype=torch.int64, device=dev)
        # one buffer for the rows of every C and one for the runs route's matrix (n x 1024 words are 82 GB each at 2 x 10^7 reads)
        widest = max(args.classes)
        rows_buf = torch.zeros(n * widest + 1, dtype=torch.int32, device=dev)
        runs_buf = torch.zeros(n * widest, dtype=torch.int32, device=dev)
        checked = set()
        # the runtime's own memset, as the call issues it: looked up through the library, which is linked against the one runtime of the process
        from sshash_amd import _binding

        hip_memset = _binding._load().hipMemsetAsync
        hip_memset.restype, hip_memset.argtypes = ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_void_p]
        for C in args.classes:
            labels = (torch.arange(n_strings, dtype=torch.int64, device=dev) % C).to(torch.int32)
            rows = rows_buf[:n * C + 1]    # (a guard word behind the last)
            by_runs = runs_buf[:n * C]

            def classes_form(labels=labels, rows=rows, C=C):
                d.streaming_classes_device(0, reads.data_ptr(), offsets.data_ptr(), n, labels.data_ptr(), C, rows.data_ptr(), d_report=report.data_ptr(),
                                           stream=stream, total_bases=n * L)

            def memset_alone(rows=rows, C=C):
                assert hip_memset(rows.data_ptr(), 0, 4 * n * C, stream) == 0

            def runs_route(labels=labels, by_runs=by_runs, C=C):
                d.streaming_runs_device(0, reads.data_ptr(), offsets.data_ptr(), n, run_offsets.data_ptr(), records.data_ptr(), n_runs, d_report=report.data_ptr(),
                                        stream=stream, total_bases=n * L)
                by_runs.zero_()
                recs = records[:4 * n_runs].view(n_runs, 4)
                read_of = torch.repeat_interleave(read_ids, run_offsets[1:] - run_offsets[:-1], output_size=n_runs)
                lengths = ((recs[:, 3] >> 32) & 0x7FFFFFFF).to(torch.int32)
                by_runs.scatter_add_(0, read_of * C + labels[recs[:, 1]].to(torch.int64), lengths)

            def guard(rows=rows):  # (garbage under the rows: whatever the wider forms left there; the guard word zero)
                rows[-1:].zero_()

            def check(rows=rows, by_runs=by_runs, C=C):
                """once per C, behind the runs route of the first round: the guard, the two routes word for word, every k-mer in a column
                (every string has a class), the finish kernels"""
                if C in checked:
                    return
                checked.add(C)
                assert int(rows[-1].item()) == 0
                for a in range(0, n * C, CHUNK):
                    assert torch.equal(rows[a:min(n * C, a + CHUNK)], by_runs[a:a + CHUNK]), f"the classes form against the runs route, C = {C}"
                matrix = rows[:-1].view(n, C)
                positive = 0
                for a in range(0, n, CHUNK // C):
                    positive += int(matrix[a:a + CHUNK // C].sum(dtype=torch.int64).item())
                assert positive == int(totals[1].item()), "every positive k-mer in one column"
                totals_c = torch.zeros(C, dtype=torch.int64, device=dev)
                best = torch.zeros(4 * n, dtype=torch.int32, device=dev)
                e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
                e0.record()
                d.class_totals_device(0, rows.data_ptr(), n, C, totals_c.data_ptr(), stream=stream)
                e1.record()
                d.class_best_device(0, rows.data_ptr(), n, C, best.data_ptr(), stream=stream)
                e2.record()
                e2.synchronize()
                assert int(totals_c.sum().item()) == positive
                assert int(best.view(n, 4)[:, 3].to(torch.int64).sum().item()) == positive
                rec[f"class_totals_{C}_ms"], rec[f"class_best_{C}_ms"] = e0.elapsed_time(e1), e1.elapsed_time(e2)

            forms += [(f"memset_{C}", memset_alone, False, nothing, nothing), (f"classes_{C}", classes_form, True, guard, nothing),
                      (f"runs_route_{C}", runs_route, True, nothing, check)]
    times = {name_: [] for name_, *_ in forms}
    totals = None
    for i in range(args.warmup + args.reps):
        for name_, fn, fills_report, before, after in forms:
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
            if fills_report:
                assert torch.equal(report, totals), name_
            after()
    for name_ in times:
        rec[name_] = entry(times[name_])
    rec["report"] = [int(v) for v in totals.cpu().tolist()]
    rec["sums_over_counters"] = rec["sums"]["ms"] / rec["counters"]["ms"]
    assert int(sums[:-1].view(n, 2)[:, 1].sum().item()) == rec["report"][1] and int(sums[-1].item()) == 0
    line = f"{name}: A {rec['counters']['ms']:.2f}  U {rec['sums']['ms']:.2f}"
    for C in ([] if args.existing_only else args.classes):
        rec[f"classes_{C}_over_sums"] = rec[f"classes_{C}"]["ms"] / rec["sums"]["ms"]
        rec[f"classes_{C}_over_counters"] = rec[f"classes_{C}"]["ms"] / rec["counters"]["ms"]
        rec[f"classes_{C}_less_memset_over_sums"] = (rec[f"classes_{C}"]["ms"] - rec[f"memset_{C}"]["ms"]) / rec["sums"]["ms"]
        rec[f"runs_route_{C}_over_classes"] = rec[f"runs_route_{C}"]["ms"] / rec[f"classes_{C}"]["ms"]
        rec[f"rows_bytes_{C}"] = 4 * n * C
        line += f"  | C={C}: K {rec[f'classes_{C}']['ms']:.2f}  M {rec[f'memset_{C}']['ms']:.2f}  X {rec[f'runs_route_{C}']['ms']:.2f}"
    log(line + " ms")
    forms.clear()
    del reads, prefix, sums
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
    ap.add_argument("--classes", type=int, nargs="+", default=[4, 64, 1024])
    ap.add_argument("--bases", type=int, default=None, help="default: the workload's (bench.WORKLOADS)")
    ap.add_argument("--existing-only", action="store_true", help="counters and sums only: for a build without the classes")
    ap.add_argument("--label", default="this", help="which build of the library this is, for the record (e.g. parent)")
    ap.add_argument("--cache-dir", default=os.environ.get("SSHASH_BENCH_CACHE", "/tmp"))
    ap.add_argument("--package-dir", default=None, help="a directory that holds another build's sshash_amd package (its binding and its library): the parent's")
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    if args.package_dir:
        sys.path.insert(0, os.path.abspath(args.package_dir))
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bench_streaming_classes needs a GPU")
    for name in args.configs:
        print(json.dumps(run_config(name, args)), flush=True)


if __name__ == "__main__":
    main()
