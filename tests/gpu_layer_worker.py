#!/usr/bin/env python
"""Worker of tests/test_gpu_layers.py: one process = one replica layer (the layer is chosen from the environment when a replica is
uploaded: SSHASH_AMD_SKTABLE, SSHASH_AMD_DIRECTORY, and the tests' own SSHASH_AMD_TEST_HOOKS). Every dictionary of DICTIONARIES
-- (k, m) from 15 to 63, regular and canonical, plus one of a single k-mer -- goes through every input form against the CPU oracle,
field by field: packed host input, packed device input (ids; every field but `minimizer_found`, the multi-pass kernels; every field),
ASCII device input at unaligned base offsets (the byte-wise staging of the ASCII tile), ASCII host input in page-locked memory at an
odd address (read by the kernels where it lies), neighbours and the streaming query. Prints one JSON line; any mismatch is an
assertion error.

    python tests/gpu_layer_worker.py <layer>

The helpers (packed k-mers as ASCII, a device lookup into fresh buffers) are shared with other tests."""
from __future__ import annotations

import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

INVALID = np.uint64(0xFFFFFFFFFFFFFFFF)
U64_FIELDS = ("kmer_id", "kmer_id_in_string", "kmer_offset", "string_id", "string_begin", "string_end")
ALL_FIELDS = U64_FIELDS + ("kmer_orientation", "minimizer_found")
# the three device forms: ids only; every field but `minimizer_found` (multi-pass); every field (table-less: the MPHF kernel)
DEVICE_FORMS = {"ids": ("kmer_id",), "full_no_flag": U64_FIELDS + ("kmer_orientation",), "full": ALL_FIELDS}

# (k, m, canonical, seed); skewed_sequences plants MIDLOAD and HEAVYLOAD buckets and table keys with lists
DICTIONARIES = [(k, m, canonical, 100 + k + int(canonical)) for k, m in ((15, 7), (31, 11), (33, 13), (47, 15), (63, 17))
                for canonical in (False, True)]
NAMED_REASONS = (None, "disabled", "minimizer shard", "more than 2^39 bases", "too many items for one build pass", "not enough free HBM")
LAYERS = {  # name -> (environment, what device_stats() must show)
    "table": ({}, lambda st: st["sk_slots"] > 0),
    "directory": ({"SSHASH_AMD_SKTABLE": "0", "SSHASH_AMD_DIRECTORY": "1"},
                  lambda st: st["sk_slots"] == 0 and st["sk_absent_reason"] == "disabled" and st["directory_sectors"] > 0),
    "mphf": ({"SSHASH_AMD_SKTABLE": "0", "SSHASH_AMD_DIRECTORY": "0"}, lambda st: st["sk_slots"] == 0 and st["directory_sectors"] == 0),
    # several launch sequences per batch, and a resume queue so short that the bucket-scan pass overflows into the deferred pass
    "directory_pieces": ({"SSHASH_AMD_SKTABLE": "0", "SSHASH_AMD_DIRECTORY": "1", "SSHASH_AMD_TEST_HOOKS": "piece=4096,resume_divisor=64"},
                         lambda st: st["sk_slots"] == 0 and st["sk_absent_reason"] == "disabled" and st["directory_sectors"] > 0),
}


def packed_to_ascii(q: np.ndarray, k: int) -> np.ndarray:
    """Packed k-mers (W words each, character i at bits 2i of the 128-bit value) -> (n, k) uint8 of 'ACTG' (code -> character,
    reference include/kmer.hpp:118)."""
    W = 1 if k <= 31 else 2
    q2 = np.ascontiguousarray(q, dtype=np.uint64).reshape(-1, W)
    codes = np.empty((q2.shape[0], k), dtype=np.uint8)
    for i in range(k):
        codes[:, i] = ((q2[:, i // 32] >> np.uint64(2 * (i % 32))) & np.uint64(3)).astype(np.uint8)
    return np.frombuffer(b"ACTG", dtype=np.uint8)[codes]


def mixed_case(text: np.ndarray, seed: int) -> np.ndarray:
    """About half of the characters in lower case (the packer maps both cases alike: (c >> 1) & 3)."""
    rng = np.random.default_rng(seed)
    out = text.copy()
    out[rng.random(out.shape) < 0.5] += 32
    return out


def device_lookup(d, ptr: int, n: int, fields, ascii_input=False, check_rc=True) -> dict:
    """lookup_device into fresh device buffers pre-filled with a value no field takes (an unwritten place shows); -> numpy arrays."""
    import torch

    bufs = {}
    for f in fields:
        dtype = torch.int8 if f in ("kmer_orientation", "minimizer_found") else torch.int64
        bufs[f] = torch.full((max(n, 1),), 5 if dtype == torch.int8 else -5, dtype=dtype, device="cuda:0")
    extra = {f: t.data_ptr() for f, t in bufs.items() if f != "kmer_id"}
    d.lookup_device(0, ptr, n, bufs["kmer_id"].data_ptr(), check_reverse_complement=check_rc, ascii_input=ascii_input,
                    stream=torch.cuda.current_stream().cuda_stream, **extra)
    torch.cuda.synchronize()
    out = {}
    for f, t in bufs.items():
        a = t[:n].cpu().numpy()
        out[f] = a.view(np.uint64) if a.dtype == np.int64 else (a.view(np.uint8) if f == "minimizer_found" else a)
    return out


def assert_fields(got, want, fields, what):
    """`got`: LookupResult or dict of arrays; `want`: oracle result array (RESULT_DTYPE) or another `got`."""
    def get(x, f):
        v = x[f] if isinstance(x, (dict, np.ndarray)) else getattr(x, f)
        return np.asarray(v).astype(np.int64) if f in ("kmer_orientation", "minimizer_found") else np.asarray(v)

    for f in fields:
        g, w = get(got, f), get(want, f)
        assert g.shape == w.shape, f"{what}: {f} has {g.shape} entries, expected {w.shape}"
        bad = np.flatnonzero(g != w)
        assert bad.size == 0, f"{what}: {f} differs at {bad.size} of {g.size} places (first {bad[:5].tolist()}: {g[bad[:5]].tolist()} != {w[bad[:5]].tolist()})"


def every_kmer_queries(case):
    """Every k-mer of the input in file order, every other one (even ids) reverse-complemented; -> packed words."""
    n = case.gt.num_kmers
    every = case.gt.kmers(np.arange(n)).reshape(n, case.W)
    rc = case.gt._revcomp(every.reshape(-1)).reshape(n, case.W)
    every[::2] = rc[::2]
    return np.ascontiguousarray(every).reshape(-1)


def check_dictionary(case, layer, seed, single=False):
    import torch

    from test_gpu_parity import _expand_neighbours
    from test_gpu_streaming import _as_dict, _synthetic_reads

    k, W = case.k, case.W
    d = case.dict.to_device(0)
    st = d.device_stats()
    if single:
        assert st["sk_absent_reason"] in NAMED_REASONS, st
    else:
        assert LAYERS[layer][1](st), f"{case.name}: the replica is not the {layer} layer: {st}"
    n = case.gt.num_kmers
    Q = np.concatenate([every_kmer_queries(case), case.queries(n, n, seed=seed)])
    N = Q.size // W
    what = f"{layer} {case.name}"

    # -- packed host input: ids, every field, is_member; both settings of check_reverse_complement
    want = {rc: case.oracle.lookup_packed(Q, rc) for rc in (True, False)}
    for rc in (True, False):
        w = want[rc]
        assert_fields(d.lookup(Q, check_reverse_complement=rc, full=True), w, ALL_FIELDS, f"{what} host full rc={rc}")
        assert_fields(d.lookup(Q, check_reverse_complement=rc), w, ("kmer_id",), f"{what} host ids rc={rc}")
        assert (d.is_member(Q, check_reverse_complement=rc) == (w["kmer_id"] != INVALID)).all(), f"{what} host is_member rc={rc}"
    assert (want[True]["kmer_id"][:n] == np.arange(n, dtype=np.uint64)).all(), f"{what}: ids are not the file order"
    w = want[True]

    # -- packed device input: three forms, is_member
    dq = torch.from_numpy(Q.view(np.int64)).to("cuda:0")
    for form, fields in DEVICE_FORMS.items():
        assert_fields(device_lookup(d, dq.data_ptr(), N, fields), w, fields, f"{what} device packed {form}")
    assert_fields(device_lookup(d, dq.data_ptr(), N, ("kmer_id",), check_rc=False), want[False], ("kmer_id",), f"{what} device packed ids rc=False")
    member = torch.full((N,), 7, dtype=torch.uint8, device="cuda:0")
    d.is_member_device(0, dq.data_ptr(), N, member.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert (member.cpu().numpy() == (w["kmer_id"] != INVALID)).all(), f"{what} device is_member"

    # -- ASCII device input: mixed case, at base offsets 0, 1, 3, 8 and 15 of one larger buffer (a workgroup's run of characters starts
    #    256 * k bytes after the previous one's, so all of a batch's workgroups share the base's alignment); ragged batch sizes --
    #    517 leaves a last workgroup of 5 queries, whose 5 * k characters are no multiple of 16
    text = mixed_case(packed_to_ascii(Q, k), seed)
    want_ascii = case.oracle.lookup_ascii(text)
    assert_fields(want_ascii, w, ALL_FIELDS, f"{what} oracle ascii vs packed")
    #    Every launch takes the queries in an order of its own: a tile that misses a character keeps what the previous workgroup on
    #    that compute unit left in LDS, and a launch over the same queries as the one before would find the right character there.
    filler = np.frombuffer(b"GATTACA" * ((N * k + 64) // 7 + 1), dtype=np.uint8)[: N * k + 64]
    big = torch.from_numpy(filler.copy()).to("cuda:0")
    sizes = sorted({s for s in (N, 1, 255, 257, 517) if s <= N})
    order = np.random.default_rng(seed)
    for off in (0, 1, 3, 8, 15):
        for size in sizes:
            for form, fields in DEVICE_FORMS.items():
                pick = order.permutation(N)[:size]
                big[off:off + size * k] = torch.from_numpy(text[pick].reshape(-1)).to("cuda:0")
                got = device_lookup(d, big.data_ptr() + off, size, fields, ascii_input=True)
                assert_fields(got, want_ascii[pick], fields, f"{what} device ascii {form} offset {off} size {size}")
                big[off:off + size * k] = torch.from_numpy(filler[off:off + size * k].copy()).to("cuda:0")

    # -- ASCII host input, page-locked, one byte into its allocation: with a page-locked output the kernels read it where it lies
    #    (in an order of its own, as above)
    pageable = d.lookup(text).kmer_id
    assert (pageable == w["kmer_id"]).all(), f"{what}: pageable ascii"
    pick = order.permutation(N)
    pin = torch.empty(N * k + 1, dtype=torch.uint8).pin_memory()
    pin[1:] = torch.from_numpy(text[pick].reshape(-1))
    out_pin = torch.full((N,), -5, dtype=torch.int64).pin_memory()
    d.lookup(pin.numpy()[1:], out=out_pin.numpy().view(np.uint64))
    assert (out_pin.numpy().view(np.uint64) == pageable[pick]).all(), f"{what}: page-locked ascii at an odd address"

    # -- neighbours: eight oracle lookups each
    sub = Q[: min(N, 600) * W]
    expanded = _expand_neighbours(sub, k, W)
    assert_fields(d.neighbours(sub, full=True), case.oracle.lookup_packed(expanded), ALL_FIELDS, f"{what} neighbours")
    assert (d.neighbours(sub).kmer_id == case.oracle.lookup_packed(expanded)["kmer_id"]).all(), f"{what} neighbour ids"

    # -- streaming: counters, every k-mer of every read, the device entry point
    rng = np.random.default_rng(seed)
    if single:
        s = case.sequences[0]
        comp = str.maketrans("ACGT", "TGCA")
        reads = [s, s.translate(comp)[::-1], "A" + s + "C", s[:10] + "N" + s[11:], s.lower(), s[1:], ""]
    else:
        reads = _synthetic_reads(case, 300, seed=seed, read_len=3 * k)
    reads += ["".join(rng.choice(list("AC"), size=150)) for _ in range(6)] + ["A" * 200, "ACGT" * 40, ("A" * 30 + "C" * 30) * 3]
    want_report = case.oracle.streaming_query(reads)
    assert _as_dict(d.streaming_query(reads)) == want_report, f"{what} streaming_query"
    per_read, report = d.streaming_lookup(reads, full=True)
    assert _as_dict(report) == want_report, f"{what} streaming_lookup report"
    for r, (read, got) in enumerate(zip(reads, per_read)):
        wr = case.oracle.streaming_read(read)
        assert got.kmer_id.size == wr.size == max(0, len(read) - k + 1)
        found = wr["kmer_id"] != INVALID
        assert_fields(got, wr, ("kmer_id", "kmer_id_in_string", "string_id", "string_begin", "string_end"), f"{what} streaming read {r}")
        assert (got.kmer_orientation[found] == wr["kmer_orientation"][found]).all(), f"{what} streaming read {r} orientation"
    blob = "".join(reads).encode()
    offsets = np.zeros(len(reads) + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum([len(x) for x in reads])
    d_bases = torch.frombuffer(bytearray(blob), dtype=torch.uint8).to("cuda:0")
    d_off = torch.from_numpy(offsets.view(np.int64)).to("cuda:0")
    ids = torch.full((len(blob),), -1, dtype=torch.int64, device="cuda:0")
    rep = torch.zeros(6, dtype=torch.int64, device="cuda:0")
    d.streaming_lookup_device(0, d_bases.data_ptr(), d_off.data_ptr(), len(reads), len(blob), ids.data_ptr(), d_report=rep.data_ptr(),
                              stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    host_ids = np.full(len(blob), INVALID, dtype=np.uint64)
    for i, got in enumerate(per_read):
        host_ids[int(offsets[i]):int(offsets[i]) + got.kmer_id.size] = got.kmer_id
    assert (ids.cpu().numpy().view(np.uint64) == host_ids).all(), f"{what} streaming_lookup_device ids"
    assert dict(zip(want_report, rep.cpu().numpy().tolist())) == want_report, f"{what} streaming_lookup_device report"
    d.close()
    return {"kmers": n, "queries": N, "sk_slots": st["sk_slots"], "directory_sectors": st["directory_sectors"],
            "sk_absent_reason": st["sk_absent_reason"]}


def main(layer):
    import tempfile

    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from conftest import Case, random_dna, skewed_sequences

    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for k, m, canonical, seed in DICTIONARIES:
            # (k = 15: fewer planted copies, or two of the short k-mers would coincide)
            seqs = skewed_sequences(k, m, seed=seed, n_heavy=80 if k <= 15 else 150, n_plain=40, canonical=canonical)
            case = Case(f"k{k}_m{m}_{'canonical' if canonical else 'regular'}", seqs, k, m, canonical, tmp)
            buckets = case.dict.bucket_stats()
            assert buckets["num_buckets_in_skew_index"] > 0 and buckets["num_buckets_larger_than_1_not_in_skew_index"] > 0, buckets
            out[case.name] = check_dictionary(case, layer, seed)
        single = Case("single_kmer", [random_dna(np.random.default_rng(9), 31)], 31, 11, False, tmp)
        out[single.name] = check_dictionary(single, layer, 9, single=True)
    print(json.dumps({"ok": True, "layer": layer, "dictionaries": out}))


if __name__ == "__main__":
    main(sys.argv[1])
