#!/usr/bin/env python
"""The streaming anchors (sshash_streaming_best_run_device: per read, its longest run) on one MI355X beside the forms of the run kernel
it stands next to and beside the route it replaces. Prints one JSON line per configuration:

    python tools/bench_streaming_best_run.py c3 c4 [--reps 10] [--reads N] [--parent-package-dir DIR] [--cache-dir DIR]

  A    counters     sshash_streaming_query_device: six counters for the batch
  C    rows         sshash_streaming_query_per_read_device: 48 bytes a read + totals
  R    runs         sshash_streaming_runs_device with records: a counting launch, a prefix sum, a second launch (32 bytes a run)
  R+F  runs route   R, then sshash_runs_best_device over its CSR: what a caller did before to get one place per read
  F    finish       sshash_runs_best_device alone, over the CSR of the read set
  B    best run     sshash_streaming_best_run_device: the records (32 bytes a read) zeroed inside the call, one launch

With --parent-package-dir (a directory that holds the parent commit's sshash_amd package, binding and library) A, C and R are also taken
from that build IN THE SAME PROCESS: its library is loaded beside this one, loads the same dictionary file and uploads a replica of its
own. All forms ALTERNATE inside one loop, so that a drift of the machine falls on all of them alike. Every figure: median of --reps
event-timed calls after --warmup rounds, lowest and highest beside it and all of them listed; k-mers/s = the reads' k-mers / that. In
the first round B's records are compared byte for byte with runs_best_device over R's CSR, a guard record behind them stays as it was,
and the two builds' reports and CSRs are compared. `stores_per_read` is how often B's lane stores a record: the runs of a read that are
longer than every run before them, counted from R's CSR. Read sets and dictionaries: those of tools/bench_streaming_sums.py."""
from __future__ import annotations

import argparse
import importlib.util
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_streaming_per_read import POSITIVE  # noqa: E402


def log(msg):
    print(f"[bench_streaming_best_run] {msg}", file=sys.stderr, flush=True)


def load_parent_package(directory):
    """the parent build's package under a name of its own: its binding loads the library that lies beside it"""
    init = os.path.join(os.path.abspath(directory), "sshash_amd", "__init__.py")
    spec = importlib.util.spec_from_file_location("sshash_amd_parent", init, submodule_search_locations=[os.path.dirname(init)])
    module = importlib.util.module_from_spec(spec)
    sys.modules["sshash_amd_parent"] = module
    spec.loader.exec_module(module)
    return module


def run_config(name, args, parent):
    import torch

    import bench
    import sshash_amd
    from sshash_amd.repeats import load_recipe
    from sshash_amd.synthetic import make_reads_device

    bases, recipe, _, _ = bench.WORKLOADS[name]
    r = load_recipe(recipe)
    ns = argparse.Namespace(bases=args.bases or bases, k=int(r["k"]), m=int(r["m"]), canonical=False, seed=0x5555AAAA,
                            recipe=recipe, repeat_scale=1.0, cache_dir=args.cache_dir, verbose=False)
    d, index_path = bench.get_index(ns, 0, 1, lambda: None)
    t0 = time.time()
    d.to_device(0)
    log(f"{name}: uploaded in {time.time() - t0:.1f}s")
    builds = [("this", d)]
    if parent is not None:
        if not os.path.exists(index_path):
            d.save(index_path)
        t0 = time.time()
        d_parent = parent.Dictionary.load(index_path)
        d_parent.to_device(0)
        assert parent.library_path() != sshash_amd.library_path() and d_parent.num_kmers() == d.num_kmers()
        log(f"{name}: the parent's library ({parent.library_path()}) loaded the dictionary and uploaded it in {time.time() - t0:.1f}s")
        builds.append(("parent", d_parent))
    dev = torch.device("cuda", 0)
    n, L, k = args.reads, args.read_len, d.k()
    reads = make_reads_device(d, 0, n, L, positive_fraction=POSITIVE[name], seed=ns.seed)
    offsets = torch.arange(n + 1, dtype=torch.int64, device=dev) * L
    report = torch.zeros(6, dtype=torch.int64, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    kmers = n * (L - k + 1)
    rec = {"config": name, "k": k, "num_kmers_of_the_dictionary": d.num_kmers(), "reads": n, "read_len": L, "positive_fraction_of_reads": POSITIVE[name],
           "kmers_per_call": kmers, "reps": args.reps, "warmup": args.warmup, "builds": [b for b, _ in builds]}

    def entry(all_ms):
        ms = statistics.median(all_ms)
        return {"ms": ms, "lowest_ms": min(all_ms), "highest_ms": max(all_ms), "all_ms": all_ms, "gkmers_per_s": kmers / ms / 1e6}

    # the runs of the read set: counted once, outside the timed regions, to size the records
    run_offsets = {b: torch.zeros(n + 1, dtype=torch.int64, device=dev) for b, _ in builds}
    d.streaming_runs_device(0, reads.data_ptr(), offsets.data_ptr(), n, run_offsets["this"].data_ptr(), 0, 0, stream=stream, total_bases=n * L)
    torch.cuda.synchronize()
    n_runs = int(run_offsets["this"][n].item())
    rec["num_runs"] = n_runs
    records = {b: torch.zeros(4 * n_runs + 4, dtype=torch.int64, device=dev) for b, _ in builds}  # (32 bytes a record)
    rows = torch.zeros(6 * n, dtype=torch.int64, device=dev)
    best = torch.full((4 * n + 4,), 0x7777777777777777, dtype=torch.int64, device=dev)  # (a guard record behind the last)
    by_runs = torch.zeros(4 * n, dtype=torch.int64, device=dev)

    def counters(dd):
        dd.streaming_query_device(0, reads.data_ptr(), offsets.data_ptr(), n, report.data_ptr(), stream=stream, total_bases=n * L)

    def rows_form(dd):
        dd.streaming_query_per_read_device(0, reads.data_ptr(), offsets.data_ptr(), n, rows.data_ptr(), d_report=report.data_ptr(), stream=stream, total_bases=n * L)

    def runs_form(dd, b):
        dd.streaming_runs_device(0, reads.data_ptr(), offsets.data_ptr(), n, run_offsets[b].data_ptr(), records[b].data_ptr(), n_runs, d_report=report.data_ptr(),
                                 stream=stream, total_bases=n * L)

    def finish():
        d.runs_best_device(0, run_offsets["this"].data_ptr(), records["this"].data_ptr(), n, by_runs.data_ptr(), stream=stream)

    def runs_route():
        runs_form(d, "this")
        finish()

    def best_run():
        d.streaming_best_run_device(0, reads.data_ptr(), offsets.data_ptr(), n, best.data_ptr(), d_report=report.data_ptr(), stream=stream, total_bases=n * L)

    checked = []

    def check():
        """once, behind the runs route of the first round: the guard, the two routes byte for byte, the stores a read costs B"""
        if checked:
            return
        checked.append(True)
        assert bool((best[4 * n:] == 0x7777777777777777).all()), "a byte behind best[0 .. num_reads) was written"
        assert torch.equal(best[:4 * n], by_runs), "the best-run form against runs_best_device over the run records"
        lengths = (records["this"][:4 * n_runs].view(n_runs, 4)[:, 3] >> 32) & 0x7FFFFFFF
        counts = run_offsets["this"][1:] - run_offsets["this"][:-1]
        read_of = torch.repeat_interleave(torch.arange(n, dtype=torch.int64, device=dev), counts, output_size=n_runs)
        key = (read_of << 31) | lengths  # (ascending in the read: a running maximum of it is the running maximum inside every read)
        before = torch.cat([torch.full((1,), -1, dtype=torch.int64, device=dev), torch.cummax(key, 0).values[:-1]])
        first = torch.ones(n_runs, dtype=torch.bool, device=dev)
        first[1:] = read_of[1:] != read_of[:-1]
        stores = int((first | (key > before)).sum().item())
        with_a_run = int((counts > 0).sum().item())
        best_lengths = (best[:4 * n].view(n, 4)[:, 3] >> 32) & 0x7FFFFFFF
        rec["reads_with_a_run"], rec["stores"], rec["stores_per_read"] = with_a_run, stores, stores / n
        rec["stores_per_read_with_a_run"] = stores / max(with_a_run, 1)
        rec["runs_per_read"] = n_runs / n
        rec["mean_best_run"] = float(best_lengths.double().mean().item())
        assert int((best_lengths > 0).sum().item()) == with_a_run
        for b, _ in builds[1:]:
            assert torch.equal(run_offsets[b], run_offsets["this"]) and torch.equal(records[b], records["this"]), "the two builds' run records"

    nothing = lambda: None
    forms = []  # (name, call, fills the report, after)
    for b, dd in builds:
        tag = "" if b == "this" else "_" + b
        forms += [("counters" + tag, lambda dd=dd: counters(dd), True, nothing), ("rows" + tag, lambda dd=dd: rows_form(dd), True, nothing),
                  ("runs" + tag, lambda dd=dd, b=b: runs_form(dd, b), True, nothing)]
    forms += [("best_run", best_run, True, nothing), ("runs_route", runs_route, True, check), ("finish", finish, False, nothing)]
    times = {name_: [] for name_, *_ in forms}
    totals = None
    for i in range(args.warmup + args.reps):
        for name_, fn, fills_report, after in forms:
            report.zero_()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if i >= args.warmup:
                times[name_].append(e0.elapsed_time(e1))
            if totals is None:
                totals = report.clone()
            if fills_report:
                assert torch.equal(report, totals), name_
            after()
    for name_ in times:
        rec[name_] = entry(times[name_])
    rec["report"] = [int(v) for v in totals.cpu().tolist()]
    rec["best_run_over_counters"] = rec["best_run"]["ms"] / rec["counters"]["ms"]
    rec["best_run_over_rows"] = rec["best_run"]["ms"] / rec["rows"]["ms"]
    rec["best_run_over_runs"] = rec["best_run"]["ms"] / rec["runs"]["ms"]
    rec["runs_route_over_best_run"] = rec["runs_route"]["ms"] / rec["best_run"]["ms"]
    span = lambda e: f"{e['ms']:.2f} [{e['lowest_ms']:.2f}-{e['highest_ms']:.2f}]"
    line = f"{name}: A {span(rec['counters'])}  C {span(rec['rows'])}  R {span(rec['runs'])}  R+F {span(rec['runs_route'])}  F {span(rec['finish'])}  B {span(rec['best_run'])}"
    if parent is not None:
        reference = rec["runs_parent"]
        rec["best_run_below_the_parents_runs_by_ms"] = reference["ms"] - rec["best_run"]["ms"]
        rec["the_parents_runs_spread_ms"] = reference["highest_ms"] - reference["lowest_ms"]
        line += f"  | parent: A {span(rec['counters_parent'])}  C {span(rec['rows_parent'])}  R {span(reference)}"
    log(line + f" ms; {rec['stores_per_read']:.3f} stores a read, {rec['runs_per_read']:.3f} runs a read")
    forms.clear()
    del reads, rows, best, by_runs, records, run_offsets
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    for _, dd in builds:
        dd.close()
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
    ap.add_argument("--parent-package-dir", default=None,
                    help="a directory that holds the parent commit's sshash_amd package (its binding and its built library): A, C and R are taken from it as well")
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bench_streaming_best_run needs a GPU")
    parent = load_parent_package(args.parent_package_dir) if args.parent_package_dir else None
    for name in args.configs:
        print(json.dumps(run_config(name, args, parent)), flush=True)


if __name__ == "__main__":
    main()
