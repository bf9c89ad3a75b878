#!/usr/bin/env python
"""Worker of tests/test_gpu_streaming_runs.py: one process = one setting of the environment switches that decide what a replica holds
(read once per process) -- here a replica WITHOUT the super-k-mer table (SSHASH_AMD_SKTABLE=0), whose run kernel takes the complete
seed() path. The runs of the host and of the device entry point against the CPU oracle, record by record. Prints one JSON line; any
mismatch is an assertion error.

    python tests/gpu_runs_worker.py <fasta> <k> <m> <canonical 0|1> <reads>

The generators and the helpers live here so that the test file and this worker make the same reads and the same expectation."""
import gzip
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import numpy as np

from gpu_per_read_worker import random_dna, revcomp, synthetic_reads  # noqa: F401  (the reads of the first set are the per-read test's)

INVALID = 0xFFFFFFFFFFFFFFFF
BACKWARD = 0x80000000
GENOME = os.path.join(ROOT, "tests", "golden", "salmonella_enterica.fasta.gz")
RUN_DTYPE = np.dtype([("kmer_id", "<u8"), ("string_id", "<u8"), ("kmer_id_in_string", "<u8"), ("read_pos", "<u4"), ("num_kmers", "<u4")])


def read_genome():
    """the records of the genome the k = 31 strings were made from, joined, upper case"""
    seq = []
    with gzip.open(GENOME, "rt") as f:
        for line in f:
            if not line.startswith(">"):
                seq.append(line.strip().upper())
    return "".join(seq)


def genome_reads(g, n, L, seed, sub=0.003):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        a = int(rng.integers(0, len(g) - L))
        r = list(g[a:a + L])
        for j in range(L):
            if rng.random() < sub:
                r[j] = "ACGT"[int(rng.integers(0, 4))]
        r = "".join(r)
        out.append(revcomp(r) if rng.random() < 0.5 else r)
    return out


def chimeras(seqs, k, n, seed):
    rng = np.random.default_rng(seed)
    long_seqs = [s for s in seqs if len(s) >= k + 40]
    out = []
    for _ in range(n):
        parts = []
        for _ in range(int(rng.integers(2, 4))):
            s = long_seqs[int(rng.integers(0, len(long_seqs)))]
            L = min(len(s), int(rng.integers(k, k + 60)))
            a = int(rng.integers(0, len(s) - L + 1))
            p = s[a:a + L]
            parts.append(revcomp(p) if rng.random() < 0.5 else p)
        out.append("".join(parts))
    return out


def runs_of_results(res):
    """the runs of one read out of its per-k-mer streaming results (oracle.streaming_read): a positive k-mer continues the run of the
    k-mer before it iff that one is positive, lies in the same string and kmer_id == previous kmer_id + previous orientation"""
    runs = []
    ids, sid, ori, kis = res["kmer_id"], res["string_id"], res["kmer_orientation"], res["kmer_id_in_string"]
    for j in range(len(res)):
        if int(ids[j]) == INVALID:
            continue
        if j and int(ids[j - 1]) != INVALID and sid[j - 1] == sid[j] and int(ids[j]) == int(ids[j - 1]) + int(ori[j - 1]):
            runs[-1][4] += 1
        else:
            runs.append([int(ids[j]), int(sid[j]), int(kis[j]), j, 1, int(ori[j])])
    out = np.zeros(len(runs), dtype=RUN_DTYPE)
    for i, (kid, s, inside, pos, n, o) in enumerate(runs):
        out[i] = (kid, s, inside, pos, n | (BACKWARD if o < 0 else 0))
    return out


def oracle_runs(oracle, reads):
    """-> (run_offsets, records) the calls must give for `reads`"""
    per_read = [runs_of_results(oracle.streaming_read(r)) for r in reads]
    offsets = np.zeros(len(reads) + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum([len(p) for p in per_read])
    return offsets, (np.concatenate(per_read) if per_read else np.zeros(0, dtype=RUN_DTYPE))


def same_records(got, want):
    return got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes()


def device_runs(d, reads, capacity=None, report=None, stream=None, total_bases=None, launches=1, tail=64, sentinel=0x5A):
    """the device entry point on device 0. capacity None: the counting call first, then a call with exactly the room it asked for.
    The record buffer holds capacity + `tail` records, every byte pre-filled with `sentinel` -> (run_offsets, the whole buffer as
    records, report) of the last launch"""
    import torch

    dev = torch.device("cuda", 0)
    blob = "".join(reads).encode()
    offsets = np.zeros(len(reads) + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum([len(r) for r in reads])
    d_bases = torch.frombuffer(bytearray(blob or b"\0"), dtype=torch.uint8).to(dev)
    d_off = torch.from_numpy(offsets.view(np.int64)).to(dev)
    d_report = None if report is None else torch.from_numpy(np.asarray(report, dtype=np.uint64).view(np.int64).copy()).to(dev)
    s = 0 if stream is None else stream.cuda_stream
    tb = len(blob) if total_bases is None else total_bases

    def sync():
        (stream or torch.cuda.current_stream(dev)).synchronize()

    if capacity is None:
        d_ro = torch.full((len(reads) + 1,), -1, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        d.streaming_runs_device(0, d_bases.data_ptr(), d_off.data_ptr(), len(reads), d_ro.data_ptr(), 0, 0, stream=s, total_bases=tb)
        sync()
        capacity = int(d_ro.cpu().numpy().view(np.uint64)[-1])
    out = []
    for _ in range(launches):
        d_ro = torch.full((len(reads) + 1,), -1, dtype=torch.int64, device=dev)
        d_runs = torch.full(((capacity + tail) * 32,), sentinel, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()  # (the fills run on torch's stream, the query may run on another)
        d.streaming_runs_device(0, d_bases.data_ptr(), d_off.data_ptr(), len(reads), d_ro.data_ptr(), d_runs.data_ptr() if capacity else 0, capacity,
                                d_report=0 if d_report is None else d_report.data_ptr(), stream=s, total_bases=tb)
        sync()
        out.append((d_ro.cpu().numpy().view(np.uint64), d_runs.cpu().numpy().view(RUN_DTYPE)))
    torch.cuda.synchronize()
    for ro, recs in out[:-1]:
        assert ro.tobytes() == out[-1][0].tobytes() and recs.tobytes() == out[-1][1].tobytes(), "two launches over the same reads differ"
    return out[-1][0], out[-1][1], None if d_report is None else d_report.cpu().numpy().view(np.uint64)


def check_both(d, reads, want_offsets, want_runs, what=""):
    """the host and the device entry point against the expectation: exact equality of run_offsets and of every field of every record"""
    ro, runs, report = d.streaming_runs(reads)
    assert ro.dtype == np.uint64 and runs.dtype == RUN_DTYPE
    assert (ro == want_offsets).all(), (what, "host run_offsets", np.flatnonzero(ro != want_offsets)[:10])
    assert same_records(runs, want_runs), (what, "host records", [i for i in range(len(runs)) if runs[i] != want_runs[i]][:5])
    dro, druns, _ = device_runs(d, reads)
    total = int(want_offsets[-1])
    assert (dro == want_offsets).all(), (what, "device run_offsets", np.flatnonzero(dro != want_offsets)[:10])
    assert same_records(druns[:total], want_runs), (what, "device records", [i for i in range(total) if druns[i] != want_runs[i]][:5])
    assert (druns[total:].view(np.uint8) == 0x5A).all(), (what, "written past the last record")
    return report


def main():
    import sshash_amd
    from oracle import oracle as O
    from oracle.ground_truth import read_fasta_sequences

    fasta, k, m, canonical, n_reads = sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), bool(int(sys.argv[4])), int(sys.argv[5])
    d = sshash_amd.Dictionary.build(fasta, k=k, m=m, canonical=canonical, num_threads=4).to_device(0)
    st = d.device_stats(0)
    sequences = read_fasta_sequences(fasta, k)
    reads = synthetic_reads(sequences, k, n_reads, seed=17) + chimeras(sequences, k, 1000, 5 if k == 31 else 7)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "w.sshash")
        d.save(path)
        want_offsets, want_runs = oracle_runs(O.OracleIndex(path), reads)
    assert int(want_offsets[-1]) > len(reads) // 2 and (want_runs["num_kmers"] & BACKWARD).any() and not (want_runs["num_kmers"] & BACKWARD).all()
    report = check_both(d, reads, want_offsets, want_runs)
    assert report.num_searches == int(want_offsets[-1]) and report == d.streaming_query(reads)
    print(json.dumps({"ok": True, "reads": len(reads), "runs": int(want_offsets[-1]), "sk_slots": st["sk_slots"],
                      "directory_sectors": st["directory_sectors"]}))


if __name__ == "__main__":
    main()
