#!/usr/bin/env python
"""Worker of tests/test_gpu_streaming_per_read.py: one process = one setting of the environment switches that decide what a replica
holds (they are read once per process) -- here a replica WITHOUT the super-k-mer table (SSHASH_AMD_SKTABLE=0: directory or MPHF), whose
per-read streaming query takes the run kernel's complete seed() path. The rows of the host and of the device entry point against the
CPU oracle, read by read. Prints one JSON line; any mismatch is an assertion error.

    python tests/gpu_per_read_worker.py <fasta> <k> <m> <canonical 0|1> <reads>

The read generator and the helpers live here so that the test file and this worker make the same reads."""
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import numpy as np

COLUMNS = ("num_kmers", "num_positive_kmers", "num_negative_kmers", "num_invalid_kmers", "num_searches", "num_extensions")
_ALPHABET = "ACTG"
_COMP = str.maketrans("ACGT", "TGCA")


def random_dna(rng, n):
    return "".join(_ALPHABET[i] for i in rng.integers(0, 4, n))


def revcomp(s):
    return s.translate(_COMP)[::-1]


def synthetic_reads(sequences, k, n_reads, seed, read_len=120):
    """Half of the reads are sampled from the indexed strings (either strand, 1% substitutions, 'N' at rate 1e-2, some in lower
    case), half are random with random lengths (many shorter than k); an empty read, one of k - 1 bases and one of N's at the end."""
    rng = np.random.default_rng(seed)
    reads = []
    long_seqs = [s for s in sequences if len(s) >= k + 5]
    for i in range(n_reads):
        if i % 2 == 0:
            s = long_seqs[int(rng.integers(0, len(long_seqs)))]
            a = int(rng.integers(0, max(1, len(s) - k)))
            r = list(s[a:a + read_len])
            for j in range(len(r)):
                u = rng.random()
                if u < 0.01:
                    r[j] = "ACGT"[int(rng.integers(0, 4))]
                elif u < 0.02:
                    r[j] = "N"
            r = "".join(r)
            if rng.random() < 0.5:
                r = revcomp(r)
            if rng.random() < 0.3:
                r = r.lower()
        else:
            r = random_dna(rng, int(rng.integers(1, read_len)))
        reads.append(r)
    reads += ["", "A" * (k - 1), "N" * (k + 3)]
    return reads


def oracle_rows(oracle, reads):
    """the oracle's report for every read alone (its state machine is reset at every read): (n, 6) uint64"""
    rows = np.zeros((len(reads), 6), dtype=np.uint64)
    for i, r in enumerate(reads):
        rep = oracle.streaming_query([r])
        rows[i] = [rep[c] for c in COLUMNS]
    return rows


def report_row(rep):
    return np.array([getattr(rep, c) for c in COLUMNS], dtype=np.uint64)


def device_rows(d, reads, prefill=0, report=None, stream=None, total_bases=None, launches=1):
    """the device entry point on device 0: rows pre-filled with `prefill`, `report` (six numbers; None: a NULL report) accumulated
    into -> (rows, report) of the last launch"""
    import torch

    dev = torch.device("cuda", 0)
    blob = "".join(reads).encode()
    offsets = np.zeros(len(reads) + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum([len(r) for r in reads])
    d_bases = torch.frombuffer(bytearray(blob or b"\0"), dtype=torch.uint8).to(dev)
    d_off = torch.from_numpy(offsets.view(np.int64)).to(dev)
    d_report = None if report is None else torch.from_numpy(np.asarray(report, dtype=np.uint64).view(np.int64).copy()).to(dev)
    out = []
    for _ in range(launches):
        d_rows = torch.full((max(1, len(reads)), 6), prefill, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()  # (the fill runs on torch's stream, the query may run on another)
        d.streaming_query_per_read_device(0, d_bases.data_ptr(), d_off.data_ptr(), len(reads), d_rows.data_ptr(),
                                          d_report=0 if d_report is None else d_report.data_ptr(),
                                          stream=0 if stream is None else stream.cuda_stream,
                                          total_bases=len(blob) if total_bases is None else total_bases)
        (stream or torch.cuda.current_stream(dev)).synchronize()
        out.append(d_rows.cpu().numpy().view(np.uint64)[:len(reads)])
    torch.cuda.synchronize()
    for other in out[:-1]:
        assert (other == out[-1]).all(), "two launches over the same reads gave different rows"
    return out[-1], None if d_report is None else d_report.cpu().numpy().view(np.uint64)


def main():
    import sshash_amd
    from oracle import oracle as O
    from oracle.ground_truth import read_fasta_sequences

    fasta, k, m, canonical, n_reads = sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), bool(int(sys.argv[4])), int(sys.argv[5])
    d = sshash_amd.Dictionary.build(fasta, k=k, m=m, canonical=canonical, num_threads=4).to_device(0)
    st = d.device_stats(0)
    sequences = read_fasta_sequences(fasta, k)
    reads = synthetic_reads(sequences, k, n_reads, seed=41)
    s = max(sequences, key=len)
    reads += [s[:3000], revcomp(s[500:2500]), s[-(k + 50):] + random_dna(np.random.default_rng(3), k + 20)]
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "w.sshash")
        d.save(path)
        want = oracle_rows(O.OracleIndex(path), reads)
    assert (want[:, 5] > 0).mean() > 0.2 and (want[:, 2] > 0).mean() > 0.35 and (want[:, 3] > 0).mean() > 0.1
    rows, report = d.streaming_query_per_read(reads)
    assert (rows == want).all(), f"host rows: reads {np.flatnonzero((rows != want).any(1))[:10]} differ"
    assert (report_row(report) == want.sum(0)).all() and (report_row(d.streaming_query(reads)) == want.sum(0)).all()
    got, rep = device_rows(d, reads, prefill=-1, report=[0] * 6, launches=2)
    assert (got == want).all(), f"device rows: reads {np.flatnonzero((got != want).any(1))[:10]} differ"
    assert (rep == 2 * want.sum(0)).all()
    print(json.dumps({"ok": True, "reads": len(reads), "sk_slots": st["sk_slots"], "directory_sectors": st["directory_sectors"],
                      "totals": [int(x) for x in want.sum(0)]}))


if __name__ == "__main__":
    main()
