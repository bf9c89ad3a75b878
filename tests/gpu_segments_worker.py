#!/usr/bin/env python
"""Worker of tests/test_gpu_read_segments.py: one process = one dictionary, one setting of SSHASH_AMD_SKTABLE and one case. Long reads cut
into segments of S k-mers (Dictionary.set_read_segments) must give word for word what the uncut reads give: the six counters, every
per-read row, the cover bitmap and the finished depth array, through the host calls and -- device_calls -- through the device calls.
Expected values come from the CPU oracle's state machine over the whole reads, and independently from the same calls under SEGMENTS_OFF.
Before anything runs on the GPU the worker asserts, from the oracle's per-k-mer results, that the reads hold every kind of read and of
run, and that for every S of {1, 2, 7, 64} seams fall inside forward and backward runs, on a run's first k-mer, behind its last, on a
negative and on an invalid k-mer. That a segmented launch really happened is read from the counter of read_segments(). Prints one JSON
line; any mismatch is an assertion error.

    python tests/gpu_segments_worker.py <fasta> <k> <m> <canonical 0|1> <scratch directory> <case> [S]
    case: segments (needs S) | long | file | shards | device_off"""
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import numpy as np

from gpu_cover_worker import bitmap_of, device_cover
from gpu_depth_worker import depth_of, device_depth, upload
from gpu_per_read_worker import COLUMNS, random_dna, report_row, revcomp, synthetic_reads

INVALID = np.uint64(0xFFFFFFFFFFFFFFFF)
ALL_S = (1, 2, 7, 64)
S_MAX = max(ALL_S)
GUARD = -0x0123456789ABCDEF  # (int64) what the rows around the device array hold


# ---- the reads ----------------------------------------------------------------------------------------------------------------------
def make_reads(sequences, k):
    """a few hundred reads of at most ~600 bases out of the dictionary's strings; what kinds are really there is asserted in kinds_of"""
    rng = np.random.default_rng(77)
    long_seqs = [s for s in sequences if len(s) >= 700]
    assert len(long_seqs) >= 10  # (the k = 63 golden file holds 24 strings, half of them this long; which kinds of reads come out is asserted in kinds_of)

    def piece(n):
        s = long_seqs[int(rng.integers(0, len(long_seqs)))]
        a = int(rng.integers(0, len(s) - n + 1))
        return s[a:a + n]

    reads = synthetic_reads(sequences, k, 120, seed=83)  # substitutions, N, lower case, random reads, "", k - 1 bases, N's
    for n in (555, 431, 600, 300):  # runs far longer than 3 * S_MAX, on either strand
        for _ in range(4):
            r = piece(n)
            reads += [r, revcomp(r)]
    for S in ALL_S:  # exactly S k-mers, S + 1 (a last segment of one k-mer), 2 S + 1
        reads += [piece(k + S - 1), piece(k + S), revcomp(piece(k + S)), piece(k + 2 * S)]
    reads += [piece(k), revcomp(piece(k))]  # one k-mer
    for S in ALL_S:
        for at in (S, 2 * S, 3 * S):  # k-mer `at` is where a seam of S falls
            n = k + at + 150
            fwd, bwd = piece(n), revcomp(piece(n))
            reads += [random_dna(rng, at) + fwd[at:], random_dna(rng, at) + bwd[at:]]       # a run's first k-mer at `at`
            reads += [fwd[:at + k - 1] + random_dna(rng, 90), bwd[:at + k - 1] + random_dna(rng, 90)]  # a run's last k-mer at `at` - 1, a negative at `at`
            for r in (fwd, bwd):
                cut = list(r)
                cut[at + 3] = "N"  # every k-mer over it is invalid, k-mer `at` among them
                reads.append("".join(cut))
                sub = list(r)
                sub[at + k + 7] = "ACGT"[("ACGT".index(sub[at + k + 7]) + 1) % 4]  # a substitution cuts the run
                reads.append("".join(sub))
    for _ in range(6):  # a run of one: a single k-mer of the dictionary between random bases
        reads.append(random_dna(rng, 45) + piece(k) + random_dna(rng, 45))
    for _ in range(4):  # two strings back to back: a run ends where the next begins
        reads.append(piece(250) + revcomp(piece(250)))
    r = piece(400)
    reads += ["N" + r[1:], r[:-1] + "N", r[:200] + "N" + r[201:]]  # N at either edge, N inside a run
    reads += [random_dna(rng, 300), random_dna(rng, 500), "A" * (k - 1), "", "", random_dna(rng, k - 5)]
    order = rng.permutation(len(reads))
    return [reads[int(i)] for i in order]


def per_kmer(oracle, read, k):
    """the oracle's state machine over one read -> per k-mer: 0 invalid, 1 negative, 2 search, 3 extension; orientation; kmer_id"""
    res = oracle.streaming_read(read)
    n = res.size
    b = np.frombuffer(read.encode("ascii", "replace"), dtype=np.uint8)
    ok = np.zeros(256, dtype=bool)
    ok[list(b"ACGTacgt")] = True
    kind = np.zeros(n, dtype=np.int8)
    if n == 0:
        return kind, np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.uint64)
    valid = ok[np.lib.stride_tricks.sliding_window_view(b, k)].all(axis=1)
    ids, sid, ori = res["kmer_id"], res["string_id"], res["kmer_orientation"]
    pos = valid & (ids != INVALID)
    kind[valid & ~pos] = 1
    kind[pos] = 2
    ext = np.zeros(n, dtype=bool)
    ext[1:] = pos[1:] & pos[:-1] & (sid[1:] == sid[:-1]) & (ids[1:] == ids[:-1] + ori[:-1].astype(np.uint64))  # the continuation rule
    kind[ext] = 3
    return kind, ori.astype(np.int64), np.where(pos, ids, INVALID)


def kinds_of(reads, kinds, oris, k):
    """what the read set holds, and where the seams of every S fall: all counts must be positive"""
    got = {"forward_runs_3S": 0, "backward_runs_3S": 0, "runs_of_one": 0, "cut_runs": 0, "N_inside_a_run": 0, "N_at_an_edge": 0,
           "hitless": 0, "shorter_than_k": 0, "empty": 0, "one_kmer": 0}
    for S in ALL_S:
        for name in ("exactly_S", "S_plus_1", "last_segment_of_one", "seam_in_forward_run", "seam_in_backward_run", "seam_on_first_of_run",
                     "seam_behind_last_of_run", "seam_on_negative", "seam_on_invalid"):
            got[f"{name}@{S}"] = 0
    for read, kind, ori in zip(reads, kinds, oris):
        K = kind.size
        got["empty"] += len(read) == 0
        got["shorter_than_k"] += 0 < len(read) < k
        got["one_kmer"] += K == 1
        got["hitless"] += K > 0 and not (kind >= 2).any()
        heads = np.flatnonzero(kind == 2)
        for h in heads:
            n = 1
            while h + n < K and kind[h + n] == 3:
                n += 1
            got["runs_of_one"] += n == 1
            if n > 3 * S_MAX:
                got["forward_runs_3S" if ori[h] > 0 else "backward_runs_3S"] += 1
        got["cut_runs"] += heads.size >= 2 and "N" not in read.upper()
        if "N" in read.upper() and K > 0:
            at = read.upper().index("N")
            got["N_at_an_edge"] += at == 0 or read.upper().rindex("N") == len(read) - 1
            got["N_inside_a_run"] += at >= k and kind[at - k] >= 2 and at + 1 < K and kind[at + 1] >= 2
        for S in ALL_S:
            got[f"exactly_S@{S}"] += K == S
            got[f"S_plus_1@{S}"] += K == S + 1
            got[f"last_segment_of_one@{S}"] += K > S and K % S == 1 % S
            for j in range(S, K, S):  # k-mer j is the first of a segment: a seam lies before it
                got[f"seam_in_forward_run@{S}"] += kind[j] == 3 and ori[j] > 0
                got[f"seam_in_backward_run@{S}"] += kind[j] == 3 and ori[j] < 0
                got[f"seam_on_first_of_run@{S}"] += kind[j] == 2
                got[f"seam_behind_last_of_run@{S}"] += kind[j - 1] >= 2 and kind[j] != 3
                got[f"seam_on_negative@{S}"] += kind[j] == 1
                got[f"seam_on_invalid@{S}"] += kind[j] == 0
    got = {name: int(v) for name, v in got.items()}
    assert all(v > 0 for v in got.values()), {name: v for name, v in got.items() if v == 0}
    return got


# ---- the calls ----------------------------------------------------------------------------------------------------------------------
def device_totals(d, reads, report):
    import torch

    d_bases, d_off, n_bases = upload(reads)
    d_report = torch.from_numpy(np.asarray(report, dtype=np.uint64).view(np.int64).copy()).to(torch.device("cuda", 0))
    torch.cuda.synchronize()
    d.streaming_query_device(0, d_bases.data_ptr(), d_off.data_ptr(), len(reads), d_report.data_ptr(), total_bases=n_bases)
    torch.cuda.synchronize()
    return d_report.cpu().numpy().view(np.uint64)


def device_rows_guarded(d, reads, report=None, total_bases=None):
    """the per-read device call into rows with two guard rows on either side, pre-filled with -1 -> (rows, report or None)"""
    import torch

    dev = torch.device("cuda", 0)
    n = len(reads)
    d_bases, d_off, n_bases = upload(reads)
    host = np.full((n + 4, 6), GUARD, dtype=np.int64)
    host[2:n + 2] = -1
    d_rows = torch.from_numpy(host).to(dev)
    d_report = None if report is None else torch.from_numpy(np.asarray(report, dtype=np.uint64).view(np.int64).copy()).to(dev)
    torch.cuda.synchronize()
    d.streaming_query_per_read_device(0, d_bases.data_ptr(), d_off.data_ptr(), n, d_rows.data_ptr() + 2 * 48,
                                      d_report=0 if d_report is None else d_report.data_ptr(), total_bases=n_bases if total_bases is None else total_bases)
    torch.cuda.synchronize()
    got = d_rows.cpu().numpy()
    assert (got[:2] == GUARD).all() and (got[n + 2:] == GUARD).all(), "a row outside the array was written"
    return got[2:n + 2].view(np.uint64).copy(), None if d_report is None else d_report.cpu().numpy().view(np.uint64)


def everything(d, reads, device):
    """the four forms through the host calls (device False) or the device calls -> a dict of arrays, compared word for word"""
    out = {}
    if device:
        out["totals"] = device_totals(d, reads, [0] * 6)
        out["rows"], out["rows_report"] = device_rows_guarded(d, reads, report=[0] * 6)
        out["rows_no_report"], _ = device_rows_guarded(d, reads)
        out["cover"], out["cover_report"] = device_cover(d, reads, report=[0] * 6)
        out["cover_no_report"], _ = device_cover(d, reads)  # report = NULL: no seam is looked at
        out["depth"], _, out["depth_report"] = device_depth(d, reads, report=[0] * 6)
        out["depth_no_report"], _, _ = device_depth(d, reads)
    else:
        out["totals"] = report_row(d.streaming_query(reads))
        rows, rep = d.streaming_query_per_read(reads)
        out["rows"], out["rows_report"] = rows, report_row(rep)
        cover, rep = d.streaming_cover(reads)
        out["cover"], out["cover_report"] = cover, report_row(rep)
        depth, rep = d.streaming_depth(reads)
        out["depth"], out["depth_report"] = depth, report_row(rep)
    return out


def accumulated(d, reads, device, before_cover, before_depth):
    """the same into a report, a bitmap and deltas (a host depth array) that already hold values"""
    out = {}
    start = np.arange(1, 7, dtype=np.uint64) * np.uint64(1000003)
    if device:
        out["totals"] = device_totals(d, reads, start)
        _, out["rows_report"] = device_rows_guarded(d, reads, report=start)
        out["cover"], out["cover_report"] = device_cover(d, reads, before=before_cover, report=start)
        out["depth"], _, out["depth_report"] = device_depth(d, reads, before=before_depth, report=start)
    else:
        out["cover"], _ = d.streaming_cover(reads, cover=before_cover.copy())
        out["depth"], _ = d.streaming_depth(reads, depth=before_depth.copy())
    return out


def same(got, want, what):
    assert sorted(got) == sorted(want), (what, sorted(got), sorted(want))
    for name in want:
        g, w = np.asarray(got[name]), np.asarray(want[name])
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, w.dtype, g.shape, w.shape)
        bad = np.argwhere(g != w)
        assert bad.size == 0, (what, name, "first differences at", bad[:5].tolist(), g[tuple(bad[0])], w[tuple(bad[0])])


def launches(d):
    return d.read_segments()["segmented_launches"]


def oracle_for(d):
    from oracle import oracle as O

    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "w.sshash")
        d.save(path)
        return O.OracleIndex(path)


# ---- the cases ----------------------------------------------------------------------------------------------------------------------
def case_segments(d, sequences, k, S):
    import sshash_amd

    reads = make_reads(sequences, k)
    assert 200 <= len(reads) <= 600 and max(len(r) for r in reads) <= 640
    oracle = oracle_for(d)
    per = [per_kmer(oracle, r, k) for r in reads]
    kinds, oris, ids = [p[0] for p in per], [p[1] for p in per], [p[2] for p in per]
    found = kinds_of(reads, kinds, oris, k)
    # expected values: the oracle's own state machine for the counters; its per-k-mer results, classified above, agree with it read by read
    want_rows = np.array([[kd.size, (kd >= 2).sum(), (kd == 1).sum(), (kd == 0).sum(), (kd == 2).sum(), (kd == 3).sum()] for kd in kinds], dtype=np.uint64)
    for i in range(0, len(reads), 7):
        rep = oracle.streaming_query([reads[i]])
        assert [rep[c] for c in COLUMNS] == want_rows[i].tolist(), ("the oracle's report against its per-k-mer results", i)
    rep = oracle.streaming_query(reads)
    want_totals = np.array([rep[c] for c in COLUMNS], dtype=np.uint64)
    assert (want_rows.sum(0) == want_totals).all()
    all_ids = np.concatenate(ids)
    want_cover, want_depth = bitmap_of(all_ids, d.cover_words()), depth_of(all_ids, d.num_kmers())
    want_host = {"totals": want_totals, "rows": want_rows, "rows_report": want_totals, "cover": want_cover, "cover_report": want_totals,
                 "depth": want_depth, "depth_report": want_totals}
    want_device = dict(want_host, rows_no_report=want_rows, cover_no_report=want_cover, depth_no_report=want_depth)
    rng = np.random.default_rng(5)
    before_cover = rng.integers(0, 1 << 63, d.cover_words(), dtype=np.uint64) & rng.integers(0, 1 << 63, d.cover_words(), dtype=np.uint64)
    before_cover[-1] &= np.uint64((1 << (d.num_kmers() % 64 or 64)) - 1)
    before_depth = rng.integers(0, 1 << 32, d.num_kmers(), dtype=np.uint64).astype(np.uint32)
    start = np.arange(1, 7, dtype=np.uint64) * np.uint64(1000003)
    want_acc_host = {"cover": want_cover | before_cover, "depth": want_depth + before_depth}
    # (the device call adds to DELTAS: what they held before is scanned with them)
    want_acc_device = dict(cover=want_acc_host["cover"], depth=want_depth + np.cumsum(before_depth, dtype=np.uint32), totals=want_totals + start, rows_report=want_totals + start, cover_report=want_totals + start,
                           depth_report=want_totals + start)

    d.to_device(0)
    st = d.device_stats(0)
    # ---- SEGMENTS_OFF: what the calls gave before there were segments; it is the oracle's too ----
    d.set_read_segments(sshash_amd.SEGMENTS_OFF, device_calls=True)
    off_host, off_device = everything(d, reads, False), everything(d, reads, True)
    same(off_host, want_host, "OFF, host calls, against the oracle")
    same(off_device, want_device, "OFF, device calls, against the oracle")
    assert launches(d) == 0, "SEGMENTS_OFF launched over segments"
    # ---- S: host calls (every read of more than S k-mers makes its piece segmented), device calls ----
    d.set_read_segments(S, device_calls=True)
    assert d.read_segments()["kmers"] == S
    got = everything(d, reads, False)
    n_host = launches(d)
    assert n_host >= 4, "the host calls did not launch over segments"
    same(got, want_host, f"S = {S}, host calls, against the oracle")
    same(got, off_host, f"S = {S}, host calls, against OFF")
    got = everything(d, reads, True)
    assert launches(d) == n_host + 7, "every device call launches over segments once"
    same(got, want_device, f"S = {S}, device calls, against the oracle")
    same(got, off_device, f"S = {S}, device calls, against OFF")
    # ---- accumulation into what is already there ----
    same(accumulated(d, reads, False, before_cover, before_depth), want_acc_host, f"S = {S}, host calls into arrays that hold values")
    same(accumulated(d, reads, True, before_cover, before_depth), want_acc_device, f"S = {S}, device calls into arrays that hold values")
    # ---- geometry: pieces inside the batch (host), partial row flushes that meet segment rows ----
    for hook in ("stream_piece_reads=37", "stream_move_out_every=1", "stream_move_out_every=3,stream_piece_reads=101"):
        os.environ["SSHASH_AMD_TEST_HOOKS"] = hook
        same(everything(d, reads, False), want_host, f"S = {S}, host calls, {hook}")
        same(everything(d, reads, True), want_device, f"S = {S}, device calls, {hook}")
    # five pieces of four reads, the third without a base: nothing is launched for it (totals, rows, cover, depth), its rows are zeros
    picks = [i for i, r in enumerate(reads) if len(r) >= k][:16]
    batch = [reads[i] for i in picks[:8]] + [""] * 4 + [reads[i] for i in picks[8:]]
    batch_rows = np.concatenate([want_rows[picks[:8]], np.zeros((4, 6), dtype=np.uint64), want_rows[picks[8:]]])
    batch_totals, batch_ids = batch_rows.sum(0), np.concatenate([ids[i] for i in picks])
    assert batch_rows[:8, 1].sum() > 0 and batch_rows[12:, 1].sum() > 0
    want_batch = {"totals": batch_totals, "rows": batch_rows, "rows_report": batch_totals, "cover": bitmap_of(batch_ids, d.cover_words()),
                  "cover_report": batch_totals, "depth": depth_of(batch_ids, d.num_kmers()), "depth_report": batch_totals}
    os.environ["SSHASH_AMD_TEST_HOOKS"] = "stream_piece_reads=4"
    same(everything(d, batch, False), want_batch, f"S = {S}, host calls, a piece of reads without a base")
    del os.environ["SSHASH_AMD_TEST_HOOKS"]
    # ---- no reads, reads without a base ----
    d.streaming_depth_device(0, 0, 0, 0, 0)
    rows, rep = device_rows_guarded(d, ["", "", ""], report=[1] * 6, total_bases=0)
    assert not rows.any() and (rep == 1).all()
    return {"ok": True, "S": S, "reads": len(reads), "segmented_launches": launches(d), "sk_slots": st["sk_slots"], "totals": [int(x) for x in want_totals],
            "seams_in_runs": found[f"seam_in_forward_run@{S}"] + found[f"seam_in_backward_run@{S}"]}


def long_read_of(sequences, n):
    parts, size = [], 0
    order = np.random.default_rng(9).permutation(len(sequences))
    while size <= n:  # (as tests/gpu_depth_worker.py: strings come more than once, on either strand)
        for i in order[:12]:
            s = sequences[int(i)][:3000]
            parts.append(revcomp(s) if len(parts) % 3 == 1 else s)
            size += len(parts[-1])
            if size > n:
                break
    return "".join(parts)


def case_long(d, sequences, k):
    """one read of ~70,000 bases at the default S: against the same bases cut into overlapping short reads, and against OFF"""
    import sshash_amd

    long_read = long_read_of(sequences, 70000)
    assert len(long_read) > (1 << 16)
    step = 1000
    pieces = [long_read[a:a + step + k - 1] for a in range(0, len(long_read) - k + 1, step)]  # overlapping by k - 1: the same k-mers
    assert sum(len(p) - k + 1 for p in pieces) == len(long_read) - k + 1
    few = make_reads(sequences, k)[:40]
    batch = few[:20] + [long_read, ""] + few[20:]
    d.to_device(0)
    assert d.read_segments()["kmers"] == sshash_amd.SEGMENTS_OFF, "a new dictionary does not segment"
    d.set_read_segments()
    S = d.read_segments()["kmers"]
    assert 1 < S < len(long_read) // 4, "the default S cuts this read into several segments"
    # the short reads: no read has more than S k-mers at the default S? (reads of ~600 bases: only if S is below that) -- no matter
    d.set_read_segments(sshash_amd.SEGMENTS_OFF)
    want_pieces = everything(d, pieces + few, False)
    off_host = everything(d, batch, False)
    d.set_read_segments(sshash_amd.SEGMENTS_OFF, device_calls=True)
    off_device = everything(d, batch, True)
    assert launches(d) == 0
    # what differs between the pieces and the whole read: a run that spans a cut is a search more and an extension less -- the sums agree
    for name in ("cover", "depth"):
        assert (off_host[name] == want_pieces[name]).all(), name
    assert (off_host["totals"][:4] == want_pieces["totals"][:4]).all() and off_host["totals"][4:].sum() == want_pieces["totals"][4:].sum()
    assert off_host["totals"][4] < want_pieces["totals"][4], "runs of the long read span the cuts"
    d.set_read_segments()  # the default S, host calls only
    got = everything(d, batch, False)
    assert launches(d) >= 4
    same(got, off_host, "the default S, host calls, against OFF")
    before = launches(d)
    d.set_read_segments(device_calls=True)
    got = everything(d, batch, True)
    assert launches(d) == before + 7
    same(got, off_device, "the default S, device calls, against OFF")
    same({name: got[name] for name in off_host}, off_host, "device calls against host calls")
    row = got["rows"][20]
    assert row[0] == len(long_read) - k + 1 and row[5] > row[4] > 0
    return {"ok": True, "S": S, "bases": len(long_read), "row": [int(x) for x in row], "segmented_launches": launches(d)}


def case_file(d, sequences, k, scratch):
    """a multiline FASTA with one record of ~3 kb through the four file calls at S = 64, against OFF and against the parsed reads"""
    import sshash_amd

    s = max(sequences, key=len)[:3000]
    assert len(s) >= 2500
    other = sequences[1][:200]
    path = os.path.join(scratch, f"multiline_k{k}_{int(d.canonical())}.fa")
    with open(path, "w") as f:
        f.write(">long\n" + "".join(s[a:a + 60] + "\n" for a in range(0, len(s), 60)) + "\n>short\n" + other + "\n")
    records = [">long" + s, ">short" + other]  # (multiline: a record is a non-empty segment of the file, header and all)
    d.to_device(0)

    def from_file():
        rows = np.zeros((len(records), 6), dtype=np.uint64)

        def keep(first, block):
            rows[first:first + block.shape[0]] = block

        out = {"totals": report_row(d.streaming_query_from_file(path, multiline=True))}
        out["rows_report"] = report_row(d.streaming_query_from_file(path, multiline=True, per_read=keep))
        out["rows"] = rows
        out["cover"], rep = d.streaming_cover_from_file(path, multiline=True)
        out["cover_report"] = report_row(rep)
        out["depth"], rep = d.streaming_depth_from_file(path, multiline=True)
        out["depth_report"] = report_row(rep)
        return out

    d.set_read_segments(sshash_amd.SEGMENTS_OFF)
    off = from_file()
    same(off, everything(d, records, False), "OFF: the file calls against the parsed records")
    assert launches(d) == 0
    d.set_read_segments(64)
    got = from_file()
    assert launches(d) == 4, "one segmented launch for each of the four file calls"
    same(got, off, "S = 64: the file calls against OFF")
    assert got["rows"][0][0] == len(records[0]) - k + 1 and got["rows"][0][5] > 2000
    return {"ok": True, "row": [int(x) for x in got["rows"][0]], "segmented_launches": launches(d)}


def case_shards(fasta, k, m, canonical, sequences):
    """a minimizer shard never segments: S = 7 gives what OFF gives, and nothing is launched over segments"""
    import sshash_amd

    reads = make_reads(sequences, k)[:150] + [long_read_of(sequences, 70000)]
    out = []
    for r in range(2):
        shard = sshash_amd.Dictionary.build(fasta, k=k, m=m, canonical=canonical, num_threads=4, num_shards=2, shard_id=r).to_device(0)
        shard.set_read_segments(sshash_amd.SEGMENTS_OFF)
        off = everything(shard, reads, False)
        rows_off, _ = device_rows_guarded(shard, reads[:150])  # (the run kernel; the host call above took the per-k-mer pipeline for the long read's piece, and on a shard the two differ)
        shard.set_read_segments(7, device_calls=True)
        got = everything(shard, reads, False)
        same(got, off, f"shard {r}: S = 7 against OFF")
        rows, _ = device_rows_guarded(shard, reads[:150])
        assert (rows == rows_off).all(), "the device call of a shard: S = 7 against OFF"
        assert launches(shard) == 0, "a minimizer shard launched over segments"
        assert off["totals"][1] > 0
        out.append(int(off["totals"][1]))
    return {"ok": True, "shards": 2, "positive": out}


def case_device_off(d, sequences, k):
    """device_calls = 0 with S = 7: the device calls are what they were (no segmented launch), while the host calls segment"""
    import sshash_amd

    reads = make_reads(sequences, k)
    d.to_device(0)
    d.set_read_segments(sshash_amd.SEGMENTS_OFF)
    off = everything(d, reads, True)
    d.set_read_segments(7, device_calls=False)
    got = everything(d, reads, True)
    assert launches(d) == 0, "device_calls = 0 launched over segments"
    same(got, off, "device_calls = 0 against OFF")
    d.streaming_query(reads)
    assert launches(d) > 0
    return {"ok": True, "segmented_launches": launches(d)}


def main():
    import sshash_amd
    from oracle.ground_truth import read_fasta_sequences

    fasta, k, m, canonical, scratch, case = sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), bool(int(sys.argv[4])), sys.argv[5], sys.argv[6]
    sequences = read_fasta_sequences(fasta, k)
    if case == "shards":
        print(json.dumps(case_shards(fasta, k, m, canonical, sequences)))
        return
    d = sshash_amd.Dictionary.build(fasta, k=k, m=m, canonical=canonical, num_threads=4)
    if case == "segments":
        out = case_segments(d, sequences, k, int(sys.argv[7]))
    elif case == "long":
        out = case_long(d, sequences, k)
    elif case == "file":
        out = case_file(d, sequences, k, scratch)
    elif case == "device_off":
        out = case_device_off(d, sequences, k)
    else:
        raise SystemExit("unknown case " + case)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
