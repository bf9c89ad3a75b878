#!/usr/bin/env python
"""Worker of tests/test_gpu_streaming_best_run.py: one process = one dictionary and one setting of the environment switch that decides
whether a replica holds the super-k-mer table (SSHASH_AMD_SKTABLE=0: the run kernel takes the complete seed() path). Everything the
streaming anchors promise -- best[r] = the longest run of read r, among equals the first, 32 zero bytes where there is none -- against
ground truth that shares no code with the kernels: the CPU oracle's point lookup of every k-mer of every read, cut into runs by the
header's rule in numpy (a k-mer continues a run iff the k-mer before is positive, in the same string, and kmer_id == previous +
previous orientation), then the argmax with the tie rule. The second truth is sshash_amd.runs_best over streaming_runs. All comparisons
are byte equality of the 32-byte records. The reads are those of the classes worker and reads made to hold what the kernel has to tell
apart; the oracle's results say, before anything runs on the GPU, that they do. Prints one JSON line; any mismatch is an assertion error.

    python tests/gpu_best_run_worker.py <k31|k63> <canonical 0|1> <scratch directory> [shards]"""
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import numpy as np

from gpu_classes_worker import make_reads as classes_reads
from gpu_depth_worker import upload
from gpu_per_read_worker import random_dna, report_row, revcomp
from gpu_sums_worker import dictionary_input, substitute
from test_streaming_best_run_capi import hand_made_csr

INVALID = np.uint64(0xFFFFFFFFFFFFFFFF)
BACKWARD = np.uint32(0x80000000)
LENGTH = np.uint32(0x7FFFFFFF)
GUARD = 0x5A
GARBAGE = 0x77


def own_dictionary(which, canonical, scratch, **kw):
    """the sums worker's sequences and, at k31, one random string of 40 000 bases behind them, in a FASTA of the worker's own
    -> (dictionary, sequences, k, the string that read (a) is)"""
    import sshash_amd

    fasta, sequences, k, m = dictionary_input(which, canonical, scratch)
    if which == "k31":
        sequences = list(sequences) + [random_dna(np.random.default_rng(43), 40000)]
        fasta = os.path.join(scratch, f"best_run_k31_{int(canonical)}.fa")
        with open(fasta, "w") as f:
            for s in sequences:
                f.write(">\n" + s + "\n")
        whole = sequences[-1]
    else:  # (the golden file has strings of that size: the second longest below 2^16 bases, the longest being a read of the classes worker already)
        whole = sorted((s for s in sequences if (1 << 15) + k <= len(s) < (1 << 16)), key=len)[-2]
    return sshash_amd.Dictionary.build(fasta, k=k, m=m, canonical=canonical, num_threads=4, **kw), sequences, k, whole


def make_reads(sequences, k, whole):
    """the classes worker's reads (-> reads, index of the read above 2^16 bases) and, behind them, (a) a string of more than 2^15 k-mers
    whole and its reverse complement, (b) reads with two runs of 41 k-mers in two strings, (c) reads whose second run is the longer,
    (d) reads of one string with two substitutions more than k apart and neither within k - 1 bases of an end: three runs"""
    reads, long_at = classes_reads(sequences, k)
    rng = np.random.default_rng(31)
    reads += [whole, revcomp(whole)]
    assert (1 << 15) + k <= len(whole) < (1 << 16)
    usable = [s for s in sequences if len(s) >= k + 60]
    for j in range(40):  # (b)
        a, b = (usable[int(i)] for i in rng.choice(len(usable), 2, replace=False))
        r = a[:k + 40] + b[-(k + 40):]
        reads.append(revcomp(r) if j % 2 else r)
    for j in range(24):  # (c)
        a, b = (usable[int(i)] for i in rng.choice(len(usable), 2, replace=False))
        r = a[:k + 10] + b[-(k + 60):]
        reads.append(revcomp(r) if j % 3 == 0 else r)
    lengthy = [s for s in sequences if len(s) >= 4 * k + 30]
    for j in range(12):  # (d)
        s = lengthy[int(rng.integers(0, len(lengthy)))]
        r = substitute(rng, s[:4 * k + 30], [k + 5, 2 * k + 20])
        reads.append(revcomp(r) if j % 2 else r)
    return reads, long_at


def oracle_results(oracle, reads, k):
    """per read the oracle's point lookup of every k-mer (either strand) as a RESULT_DTYPE array; kmer_id INVALID where the k-mer holds
    anything but A, C, G, T in either case or is not in the dictionary"""
    ok = np.zeros(256, dtype=bool)
    ok[list(b"ACGTacgt")] = True
    out, kmers, where = [], [], []
    for i, r in enumerate(reads):
        b = np.frombuffer(r.encode("ascii", "replace"), dtype=np.uint8)
        out.append(max(0, b.size - k + 1))
        if b.size < k:
            continue
        windows = np.lib.stride_tricks.sliding_window_view(b, k)
        valid = ok[windows].all(axis=1)
        kmers.append(windows[valid] & np.uint8(0xDF))  # (upper case)
        where.append((i, np.flatnonzero(valid)))
    got = oracle.lookup_ascii(np.ascontiguousarray(np.concatenate(kmers)).reshape(-1), True)
    results = []
    for n in out:
        res = np.zeros(n, dtype=got.dtype)
        res["kmer_id"] = INVALID
        results.append(res)
    at = 0
    for i, places in where:
        results[i][places] = got[at:at + places.size]
        at += places.size
    return results


def runs_of(res):
    """the header's rule over one read's per-k-mer results -> its run records, in read order"""
    import sshash_amd

    hit = res["kmer_id"] != INVALID
    n = res.size
    if n == 0 or not hit.any():
        return np.zeros(0, dtype=sshash_amd.RUN_DTYPE)
    ids, sid, ori = res["kmer_id"].astype(np.int64), res["string_id"], res["kmer_orientation"].astype(np.int64)
    assert set(np.unique(ori[hit]).tolist()) <= {1, -1}
    follows = np.zeros(n, dtype=bool)
    follows[1:] = hit[1:] & hit[:-1] & (sid[1:] == sid[:-1]) & (ids[1:] == ids[:-1] + ori[:-1])
    starts = np.flatnonzero(hit & ~follows)
    run_of = np.cumsum(hit & ~follows) - 1
    lengths = np.bincount(run_of[hit], minlength=starts.size)
    runs = np.zeros(starts.size, dtype=sshash_amd.RUN_DTYPE)
    runs["kmer_id"] = res["kmer_id"][starts]
    runs["string_id"] = sid[starts]
    runs["kmer_id_in_string"] = res["kmer_id_in_string"][starts]
    runs["read_pos"] = starts
    runs["num_kmers"] = lengths.astype(np.uint32) | np.where(ori[starts] < 0, BACKWARD, np.uint32(0))
    return runs


def best_of(runs):
    """the argmax with the tie rule: the largest num_kmers & 0x7FFFFFFF, among equals the first; zeros where there is no run"""
    import sshash_amd

    best = np.zeros(1, dtype=sshash_amd.RUN_DTYPE)
    if runs.size:
        best[0] = runs[int(np.argmax(runs["num_kmers"] & LENGTH))]  # (argmax: the first of the largest)
    return best


def same(got, want, what):
    import sshash_amd

    assert got.dtype == sshash_amd.RUN_DTYPE and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    if got.tobytes() != want.tobytes():
        bad = [r for r in range(got.size) if got[r:r + 1].tobytes() != want[r:r + 1].tobytes()]
        raise AssertionError((what, "reads", bad[:5], got[bad[:5]].tolist(), want[bad[:5]].tolist()))


def device_best(d, reads, report=None, stream=None, total_bases=None):
    """the device entry point on device 0 over records that held garbage, a guard record on both sides -> (best, report or None)"""
    import torch

    import sshash_amd

    dev = torch.device("cuda", 0)
    n = len(reads)
    d_bases, d_off, n_bases = upload(reads)
    host = np.full((n + 2) * 32, GARBAGE, dtype=np.uint8)
    host[:32] = GUARD
    host[-32:] = GUARD
    t = torch.from_numpy(host.copy()).to(dev)
    assert t.data_ptr() % 16 == 0
    d_report = None if report is None else torch.from_numpy(np.asarray(report, dtype=np.uint64).view(np.int64).copy()).to(dev)
    torch.cuda.synchronize()  # (the copies run on torch's stream, the query may run on another)
    d.streaming_best_run_device(0, d_bases.data_ptr(), d_off.data_ptr(), n, t.data_ptr() + 32, d_report=0 if d_report is None else d_report.data_ptr(),
                                stream=0 if stream is None else stream.cuda_stream, total_bases=n_bases if total_bases is None else total_bases)
    (stream or torch.cuda.current_stream()).synchronize()
    torch.cuda.synchronize()
    got = t.cpu().numpy()
    assert (got[:32] == GUARD).all() and (got[-32:] == GUARD).all(), "a byte outside best[0 .. num_reads) was written"
    return got[32:-32].copy().view(sshash_amd.RUN_DTYPE), None if d_report is None else d_report.cpu().numpy().view(np.uint64)


def host_best(d, reads):
    """the host entry point itself (the binding hands it zeros, which would hide a piece whose records never came back): records that
    held garbage, a guard record on both sides -> (best, the six counters)"""
    import ctypes

    import sshash_amd
    from sshash_amd import _binding as B

    n = len(reads)
    chunks = [r.encode("ascii", "replace") for r in reads]
    offsets = np.zeros(n + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum([len(c) for c in chunks], dtype=np.uint64)
    bases = np.frombuffer(b"".join(chunks) or b"\0", dtype=np.uint8)
    host = np.full((n + 2) * 32, GARBAGE, dtype=np.uint8)
    host[:32] = GUARD
    host[-32:] = GUARD
    rep = B._Report()
    B._check(B._load().sshash_streaming_best_run(d._h, bases.ctypes.data, offsets.ctypes.data, n, ctypes.c_void_p(host.ctypes.data + 32), ctypes.byref(rep)))
    assert (host[:32] == GUARD).all() and (host[-32:] == GUARD).all(), "a byte outside best[0 .. num_reads) was written"
    return host[32:-32].copy().view(sshash_amd.RUN_DTYPE), report_row(d._report(rep))


def device_runs_best(d, run_offsets, runs):
    """runs_best_device over a CSR uploaded as it is, into records that held garbage, a guard record on both sides"""
    import torch

    import sshash_amd

    dev = torch.device("cuda", 0)
    n = run_offsets.size - 1
    d_offsets = torch.from_numpy(np.ascontiguousarray(run_offsets, dtype=np.uint64).view(np.int64).copy()).to(dev)
    d_runs = torch.from_numpy(np.frombuffer(runs.tobytes() or b"\0" * 32, dtype=np.uint8).copy()).to(dev)
    host = np.full((n + 2) * 32, GARBAGE, dtype=np.uint8)
    host[:32] = GUARD
    host[-32:] = GUARD
    t = torch.from_numpy(host.copy()).to(dev)
    torch.cuda.synchronize()
    d.runs_best_device(0, d_offsets.data_ptr(), d_runs.data_ptr(), n, t.data_ptr() + 32)
    torch.cuda.synchronize()
    got = t.cpu().numpy()
    assert (got[:32] == GUARD).all() and (got[-32:] == GUARD).all(), "a byte outside best[0 .. num_reads) was written"
    assert d_runs.cpu().numpy().tobytes()[:runs.nbytes] == runs.tobytes(), "the records were changed"
    return got[32:-32].copy().view(sshash_amd.RUN_DTYPE)


def device_runs(d, reads):
    """streaming_runs_device on device 0 -> (run_offsets, runs) as they lie on the device, read back"""
    import torch

    import sshash_amd

    dev = torch.device("cuda", 0)
    n = len(reads)
    d_bases, d_off, n_bases = upload(reads)
    d_run_offsets = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    d.streaming_runs_device(0, d_bases.data_ptr(), d_off.data_ptr(), n, d_run_offsets.data_ptr(), 0, 0, total_bases=n_bases)
    torch.cuda.synchronize()
    total = int(d_run_offsets[-1].item())
    d_runs = torch.zeros(max(total, 1) * 32, dtype=torch.uint8, device=dev)
    d.streaming_runs_device(0, d_bases.data_ptr(), d_off.data_ptr(), n, d_run_offsets.data_ptr(), d_runs.data_ptr(), total, total_bases=n_bases)
    torch.cuda.synchronize()
    return d_run_offsets.cpu().numpy().view(np.uint64), d_runs.cpu().numpy()[:total * 32].copy().view(sshash_amd.RUN_DTYPE)


def shards_main(which, canonical, scratch):
    """two minimizer shards: the device, host and file calls refuse -- a shard's longest runs are not the whole index's"""
    import sshash_amd

    whole, sequences, k, string = own_dictionary(which, canonical, scratch)
    reads, _ = make_reads(sequences, k, string)
    reads = [r for r in reads if r][:200]
    own = os.path.join(scratch, "best_run_shard_reads.fa")
    with open(own, "w") as f:
        for i, r in enumerate(reads):
            f.write(f">{i}\n{r}\n")
    refused = 0
    for r in range(2):
        shard, _, _, _ = own_dictionary(which, canonical, scratch, num_shards=2, shard_id=r)
        shard.to_device(0)
        for call in (lambda: shard.streaming_best_run_device(0, 8, 8, 1, 16), lambda: shard.streaming_best_run(reads),
                     lambda: shard.streaming_best_run_from_file(own), lambda: shard.streaming_best_run_from_file(own, per_read=lambda first, best: 0)):
            try:
                call()
                raise AssertionError("a call on a minimizer shard did not refuse")
            except sshash_amd.SSHashError as e:
                assert e.status == 1 and "minimizer shard" in str(e) and "sshash_streaming_runs" in str(e), e
                refused += 1
        run_offsets, runs, _ = shard.streaming_runs(reads)  # (what stays open to a shard)
        assert run_offsets.size == len(reads) + 1
    print(json.dumps({"ok": True, "shards": 2, "refused": refused}))


def main():
    import torch

    import sshash_amd
    from oracle import oracle as O

    which, canonical, scratch = sys.argv[1], bool(int(sys.argv[2])), sys.argv[3]
    if len(sys.argv) > 4 and sys.argv[4] == "shards":
        return shards_main(which, canonical, scratch)
    d, sequences, k, string = own_dictionary(which, canonical, scratch)
    reads, long_at = make_reads(sequences, k, string)
    n = len(reads)
    lengths = np.array([len(r) for r in reads])

    # ---- on the CPU, before anything runs on the GPU: the oracle's runs, the truth, and what the reads have to hold ----
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "w.sshash")
        d.save(path)
        results = oracle_results(O.OracleIndex(path), reads, k)
    truth_runs = [runs_of(res) for res in results]
    want = np.concatenate([best_of(runs) for runs in truth_runs])
    best_len = want["num_kmers"] & LENGTH
    def tied(runs):
        length = runs["num_kmers"] & LENGTH
        return runs.size >= 2 and int((length == length.max()).sum()) >= 2
    kinds = {"ties_for_longest": sum(tied(runs) for runs in truth_runs),
             "longest_is_not_the_first": sum(runs.size >= 2 and int(w["read_pos"]) != int(runs["read_pos"][0]) for runs, w in zip(truth_runs, want)),
             "longest_is_backward": int(((want["num_kmers"] & BACKWARD) != 0).sum()),
             "best_of_2_15_or_more": int((best_len >= (1 << 15)).sum()),
             "hitless_reads": int(((best_len == 0) & (lengths >= k)).sum()),
             "reads_shorter_than_k": int((lengths < k).sum()),
             "reads_above_2_16": int((lengths > (1 << 16)).sum()),
             "three_runs_of_one_string": sum(runs.size == 3 and np.unique(runs["string_id"]).size == 1 for runs in truth_runs[-12:])}
    assert kinds["ties_for_longest"] >= 20 and all(v > 0 for v in kinds.values()), kinds
    assert kinds["reads_above_2_16"] == 1 and lengths[long_at] > (1 << 16) and 1800 <= n <= 2400, (kinds, n)
    assert int(lengths[np.flatnonzero(best_len >= (1 << 15))].min()) <= (1 << 16), "a run of 2^15 k-mers in a read that one lane walks in the host call"
    assert (best_len[lengths < k] == 0).all() and not want[best_len == 0].tobytes().strip(b"\0")

    # ---- the GPU: the second truth, then every entry point ----
    d.to_device(0)
    st = d.device_stats(0)
    run_offsets, runs, runs_report = d.streaming_runs(reads)
    truth_offsets = np.zeros(n + 1, dtype=np.uint64)
    truth_offsets[1:] = np.cumsum([r.size for r in truth_runs], dtype=np.uint64)
    assert (run_offsets == truth_offsets).all() and runs.tobytes() == np.concatenate(truth_runs).tobytes(), "streaming_runs against the oracle's runs"
    same(sshash_amd.runs_best(run_offsets, runs), want, "runs_best over streaming_runs against the oracle's truth")
    want_report = report_row(d.streaming_query(reads))

    got, rep = device_best(d, reads, report=[0] * 6)
    same(got, want, "device call")
    assert (rep == want_report).all(), (rep, want_report)
    got, rep = device_best(d, reads, report=[1, 2, 3, 4, 5, 6], stream=torch.cuda.Stream(device=0), total_bases=0)
    same(got, want, "device call on a side stream, total_bases = 0")
    assert (rep == want_report + np.arange(1, 7, dtype=np.uint64)).all(), "the report is accumulated into"
    got, rep = device_best(d, reads)  # a NULL report
    same(got, want, "device call, no report")
    d.streaming_best_run_device(0, 0, 0, 0, 0)  # no reads: no work
    got, rep = device_best(d, ["", "", ""], report=[1] * 6, total_bases=0)
    assert not got.tobytes().strip(b"\0") and (rep == 1).all(), "reads without a base"

    got, rep = host_best(d, reads)  # (the read above 2^16 bases: its piece goes through the per-k-mer records and runs_best_device)
    same(got, want, "host call into records that held garbage")
    assert (rep == want_report).all(), (rep, want_report)
    got, rep = d.streaming_best_run(reads)
    same(got, want, "host call through the binding")
    assert (report_row(rep) == want_report).all()
    got, rep = host_best(d, ["", "", ""])
    assert not got.tobytes().strip(b"\0") and not rep.any(), "host call, reads without a base"
    got, rep = host_best(d, [reads[long_at]])
    same(got, want[long_at:long_at + 1], "host call, the long read alone")
    hitless_long = random_dna(np.random.default_rng(5), (1 << 16) + 100)
    got, rep = host_best(d, [hitless_long, "ACGT"])  # (a long read's piece without a single record)
    assert not got.tobytes().strip(b"\0") and rep[1] == 0 and rep[0] == len(hitless_long) - k + 1
    got, rep = host_best(d, [hitless_long, reads[0]])
    assert int(got["num_kmers"][0]) == 0 and got[1:].tobytes() == want[:1].tobytes()

    # ---- geometry independence: the test hooks of the run kernel and of the host call's pieces ----
    for hook in ("stream_move_out_every=1", "stream_move_out_every=3", "stream_piece_reads=300", "stream_piece_reads=257"):
        os.environ["SSHASH_AMD_TEST_HOOKS"] = hook
        got, rep = host_best(d, reads)  # (pieces of 300 reads: the long read's piece by records, the others by the run kernel)
        same(got, want, "host call, " + hook)
        assert (rep == want_report).all(), hook
        got, rep = device_best(d, reads, report=[0] * 6)
        same(got, want, "device call, " + hook)
        assert (rep == want_report).all(), hook
    del os.environ["SSHASH_AMD_TEST_HOOKS"]

    # ---- segments never apply ----
    launches = d.read_segments()["segmented_launches"]
    d.set_read_segments(kmers=7, device_calls=True)
    got, rep = device_best(d, reads, report=[0] * 6)
    same(got, want, "device call with segments of 7 k-mers set")
    assert (rep == want_report).all()
    got, rep = host_best(d, reads)
    same(got, want, "host call with segments of 7 k-mers set")
    assert (rep == want_report).all()
    assert d.read_segments()["segmented_launches"] == launches, "the best run was cut into segments"
    d.set_read_segments(sshash_amd.SEGMENTS_OFF)

    # ---- a query file: one record a record of the file, in file order, over batch seams ----
    in_file = [i for i, r in enumerate(reads) if r]
    for fastq in (False, True):
        own = os.path.join(scratch, f"best_run_reads_{which}_{int(canonical)}." + ("fq" if fastq else "fa"))
        with open(own, "w") as f:
            for i in in_file:
                f.write(f"@{i}\n{reads[i]}\n+\n{'I' * len(reads[i])}\n" if fastq else f">{i}\n{reads[i]}\n")
        os.environ["SSHASH_AMD_TEST_HOOKS"] = "query_batch_bases=100000"
        seen = []

        def take(first_read, best):
            assert first_read == sum(len(b) for b in seen)
            seen.append(best)

        rep = d.streaming_best_run_from_file(own, per_read=take)
        assert len(seen) > 2, "batch seams inside the file"
        same(np.concatenate(seen), want[in_file], "the file entry point")
        assert len(np.concatenate(seen)) == len(in_file) and (report_row(rep) == want_report).all()
        del os.environ["SSHASH_AMD_TEST_HOOKS"]
    got, _ = d.streaming_best_run_from_file(own)
    same(got, want[in_file], "the file entry point, records kept")
    calls = []
    try:
        d.streaming_best_run_from_file(own, per_read=lambda first, best: calls.append(first) or 3)
        raise AssertionError("a callback's non-zero return did not stop the query")
    except sshash_amd.SSHashError as e:
        assert e.status == 1 and len(calls) == 1, (e, calls)
    os.environ["SSHASH_AMD_TEST_HOOKS"] = "query_batch_bases=100000"
    calls = []

    def broken(first, best):
        calls.append(first)
        if len(calls) == 2:
            raise KeyError("mine")

    try:
        d.streaming_best_run_from_file(own, per_read=broken)
        raise AssertionError("a callback's exception did not stop the query")
    except KeyError as e:
        assert e.args == ("mine",) and len(calls) == 2 and calls[0] == 0 and calls[1] > 0, (e, calls)
    del os.environ["SSHASH_AMD_TEST_HOOKS"]

    # ---- the finish on the device: the device call's own CSR, and the CSR made by hand of the CPU test ----
    dev_offsets, dev_runs = device_runs(d, reads)
    assert (dev_offsets == run_offsets).all() and dev_runs.tobytes() == runs.tobytes()
    same(device_runs_best(d, dev_offsets, dev_runs), sshash_amd.runs_best(dev_offsets, dev_runs), "runs_best_device against runs_best on the device call's CSR")
    same(device_runs_best(d, dev_offsets, dev_runs), want, "runs_best_device against the truth")
    made_offsets, made_runs, _ = hand_made_csr()
    same(device_runs_best(d, made_offsets, made_runs), sshash_amd.runs_best(made_offsets, made_runs), "runs_best_device on the CSR made by hand")
    nothing = np.zeros(4, dtype=np.uint64)
    assert not device_runs_best(d, nothing, np.zeros(0, dtype=sshash_amd.RUN_DTYPE)).tobytes().strip(b"\0"), "a CSR without a record"
    d.runs_best_device(0, 0, 0, 0, 0)  # no reads: no work

    print(json.dumps({"ok": True, "reads": n, "runs": int(run_offsets[-1]), "positive": int(runs_report.num_positive_kmers),
                      "longest": int(best_len.max()), "sk_slots": st["sk_slots"], "kinds": kinds}))


if __name__ == "__main__":
    main()
