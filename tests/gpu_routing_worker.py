#!/usr/bin/env python
"""Worker of tests/test_gpu_routing.py: one process = one dictionary (conftest.skewed_sequences) and everything the routing layer of the
multi-GPU lookup promises, on ONE GPU, against references that share no code with the kernels.

A. Owners. The minimizer owners (compute_minimizer, shard_of_minimizer, the canonical rule and the check_reverse_complement == 0 rule of
   route_bucket_kernel) restated in numpy over the k-mers' base codes -- first held against route_device on the same queries, then used
   as the expected owners of every query. The table-key owners from tests/cpp/route_owners.cpp, the host's build of sk_key / sk_owner.
B. The public two-call protocol (sshash_route_bucket_device, sshash_route_bucket_by_key_device: the scattering launch elects the owners
   again, the branch the sharded lookup never takes) at the sizes around a tile (256) and a workgroup (4096 queries) and at 1 .. 1024
   shards: counts into cursors that are not zero, regions of `slots` as sets, `send` against the queries, guard words, the cursors after
   the scattering launch; sshash_route_combine_device against the same loop in numpy; argument errors; n = 0; a caller's stream.
C. sshash_sharded_lookup_device at R = 1, 3, 8 ranks -- R threads of this process, each with its own handle and stream on device 0 and
   an exchange written here -- over minimizer shards and table shards, every id against the oracle of the whole dictionary.

Which kinds of input the batches hold is asserted from the references, never from the kernels. A shard count of 1000 or 1024 leaves
shards without a message whenever 4097 queries have one owner each (4 messages per shard on average), so "no shard is empty" is asked
of the uniform-random batch for every entry point at 64 shards, and at 1000 and 1024 shards of a regular dictionary's two-owner routing
(8 messages per shard; the batch's seed is searched for with the reference). Prints one JSON line; any mismatch is an assertion error.

    python tests/gpu_routing_worker.py <k> <m> <canonical 0|1> <seed> <route_owners binary> <scratch directory>"""
import json
import os
import subprocess
import sys
import threading

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import numpy as np

INVALID = np.uint64(0xFFFFFFFFFFFFFFFF)
GUARD, GUARD32, GUARD_WORDS = 0x5A5A5A5A5A5A5A5A, 0x5A5A5A5A, 256
PATTERN = np.uint64(0xC0DE000000000000)  # | index: what `out` holds before a call that must not rely on its contents
ERR_ARGUMENT = 1
SHARDS = (1, 2, 3, 7, 64, 1000, 1024)
SIZES = (1, 255, 256, 257, 4095, 4096, 4097, 8193)  # a tile is 256 queries, a workgroup routes 16 tiles
RANKS = (1, 3, 8)
ENTRIES = (("minimizer", True), ("minimizer", False), ("key", True))  # (entry point, check_reverse_complement)


# ---- A. the references -------------------------------------------------------------------------------------------------------------
def codes_of(kmers, k, W):
    """packed k-mers (W words each, first base in the low bits) -> (n, k) base codes"""
    q = np.ascontiguousarray(kmers, dtype=np.uint64).reshape(-1, W)
    out = np.empty((q.shape[0], k), dtype=np.uint64)
    for j in range(k):
        out[:, j] = (q[:, j // 32] >> np.uint64(2 * (j % 32))) & np.uint64(3)
    return out


def pack(codes, W):
    out = np.zeros((codes.shape[0], W), dtype=np.uint64)
    for j in range(codes.shape[1]):
        out[:, j // 32] |= codes[:, j] << np.uint64(2 * (j % 32))
    return out.reshape(-1)


def revcomp(kmers, k, W):
    return pack(codes_of(kmers, k, W)[:, ::-1] ^ np.uint64(2), W)  # A0 C1 T2 G3: the complement is code ^ 2


def minimizers(codes, m, magic):
    """compute_minimizer: the leftmost m-mer with the strictly smallest (mmer * 0x517CC1B727220A95) ^ magic over the k - m + 1 positions"""
    n, k = codes.shape
    places = k - m + 1
    mmers = np.zeros((n, places), dtype=np.uint64)
    for j in range(m):
        mmers |= codes[:, j:j + places] << np.uint64(2 * j)
    h = (mmers * np.uint64(0x517CC1B727220A95)) ^ np.uint64(magic)  # (uint64 arrays wrap)
    return mmers[np.arange(n), np.argmin(h, axis=1)]  # argmin: the first place of the minimum


def shard_of_minimizer(minimizer, S):
    h = minimizer * np.uint64(0xA24BAED4963EE407)
    x = ((h >> np.uint64(32)) ^ (h >> np.uint64(11))) & np.uint64(0xFFFFFFFF)
    return ((x * np.uint64(S)) >> np.uint64(32)).astype(np.int64)


class Reference:
    """expected (owner_f, owner_r) of a fixed set of k-mers, for any number of shards"""

    def __init__(self, kmers, k, m, W, canonical, magic, key_owners):
        codes = codes_of(kmers, k, W)
        self.n = codes.shape[0]
        self.f = minimizers(codes, m, magic)
        self.r = minimizers(codes[:, ::-1] ^ np.uint64(2), m, magic)
        self.canonical = canonical
        self.key_owners = key_owners  # {S: owners} from route_owners.cpp

    def owners(self, S, entry, check_rc, index=None):
        if entry == "key":
            o = self.key_owners[S].astype(np.int64)
            f, r = o, o
        else:
            f, r = self.f, self.r
            if self.canonical:
                f = r = np.minimum(f, r)
            if not check_rc:
                r = f
            f, r = shard_of_minimizer(f, S), shard_of_minimizer(r, S)
        return (f, r) if index is None else (f[index], r[index])


def host_key_owners(exe, kmers, k, key_length, shards):
    p = subprocess.run([exe, str(k), str(key_length)] + [str(s) for s in shards], input=np.ascontiguousarray(kmers, dtype=np.uint64).tobytes(),
                       capture_output=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    out = np.frombuffer(p.stdout, dtype=np.uint32).reshape(-1, len(shards))
    return {s: out[:, i].copy() for i, s in enumerate(shards)}


def messages(f, r, S):
    """-> (messages per shard, owner of every message, query of every message), the messages ordered by (owner, query)"""
    two = f != r
    owner = np.concatenate([f, r[two]])
    query = np.concatenate([np.arange(f.size), np.flatnonzero(two)])
    order = np.lexsort((query, owner))
    return np.bincount(owner, minlength=S).astype(np.uint64), owner[order], query[order]


# ---- device plumbing ---------------------------------------------------------------------------------------------------------------
def to_device(a):
    import torch

    a = np.ascontiguousarray(a)
    signed = {np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32}[a.dtype]
    return torch.from_numpy(a.view(signed).copy()).to("cuda:0")


def to_host(t, dtype):
    return t.cpu().numpy().view(dtype)


def bucket_call(d, entry, check_rc, d_kmers, n, S, d_cursors, d_send=0, d_slots=0, stream=0):
    if entry == "key":
        d.route_bucket_by_key_device(0, d_kmers, n, S, d_cursors, d_send, d_slots, stream=stream)
    else:
        d.route_bucket_device(0, d_kmers, n, S, d_cursors, d_send, d_slots, check_reverse_complement=check_rc, stream=stream)


def two_calls(d, entry, check_rc, kmers, W, S, f, r, what, stream=None):
    """The public protocol on n = f.size queries against the expected owners (f, r): every check of part B. -> messages per shard"""
    import torch

    n = f.size
    want_counts, want_owner, want_query = messages(f, r, S)
    total = int(want_counts.sum())
    assert n <= total <= 2 * n
    if entry == "key" or not check_rc:
        assert total == n, what
    hip_stream = 0 if stream is None else stream.cuda_stream

    def sync():
        if stream is not None:
            stream.synchronize()
        torch.cuda.synchronize()

    d_kmers = to_device(kmers[:n * W])
    prefill = np.arange(S, dtype=np.uint64) * np.uint64(7) + np.uint64(5)  # cursors that are not zero: the launch adds
    d_cursors = to_device(prefill)
    sync()
    bucket_call(d, entry, check_rc, d_kmers.data_ptr(), n, S, d_cursors.data_ptr(), stream=hip_stream)
    sync()
    counts = to_host(d_cursors, np.uint64) - prefill
    bad = np.flatnonzero(counts != want_counts)
    assert bad.size == 0, (what, "messages per shard: first differing shard", int(bad[0]), int(counts[bad[0]]), int(want_counts[bad[0]]))
    # (the counts are the expected ones: the buffers below hold every message the scattering launch may write)
    first = np.concatenate([[np.uint64(0)], np.cumsum(want_counts, dtype=np.uint64)[:-1]])
    d_cursors = to_device(first)
    d_send = to_device(np.full(total * W + GUARD_WORDS, GUARD, dtype=np.uint64))
    d_slots = to_device(np.full(total + GUARD_WORDS, GUARD32, dtype=np.uint32))
    sync()
    bucket_call(d, entry, check_rc, d_kmers.data_ptr(), n, S, d_cursors.data_ptr(), d_send.data_ptr(), d_slots.data_ptr(), stream=hip_stream)
    sync()
    send, slots, after = to_host(d_send, np.uint64), to_host(d_slots, np.uint32), to_host(d_cursors, np.uint64)
    assert (send[total * W:] == GUARD).all() and (slots[total:] == GUARD32).all(), (what, "words behind the last message were written")
    slots = slots[:total].astype(np.int64)
    assert (slots < n).all(), (what, "a slot names no query", int(np.flatnonzero(slots >= n)[0]))
    order = np.lexsort((slots, want_owner))  # (want_owner: the region every place belongs to)
    bad = np.flatnonzero(slots[order] != want_query)
    assert bad.size == 0, (what, "queries of a region: first differing place", int(bad[0]), "shard", int(want_owner[bad[0]]),
                           int(slots[order][bad[0]]), int(want_query[bad[0]]))
    bad = np.flatnonzero((send[:total * W].reshape(total, W) != kmers[:n * W].reshape(n, W)[slots]).any(axis=1))
    assert bad.size == 0, (what, "send: first message that is not its query's k-mer", int(bad[0]), "query", int(slots[bad[0]]))
    assert (after == first + want_counts).all(), (what, "cursors after the scattering launch")
    return want_counts


def combine_case(d, m, rng, stream=None):
    """sshash_route_combine_device on m replies against the same loop in numpy"""
    import torch

    queries = max(m, 4)
    slots, replies = np.zeros(m, dtype=np.uint32), np.zeros(m, dtype=np.uint64)
    doubles = {"invalid_then_id": 0, "id_then_invalid": 0, "same_id_twice": 0, "invalid_twice": 0}
    t, order = 0, rng.permutation(queries)
    for q in order:
        if t >= m:
            break
        an_id = np.uint64(rng.integers(0, 1 << 40))
        kind = int(rng.integers(0, 8))
        if kind < 4 and t + 2 <= m:  # two replies for one query
            pair = ((INVALID, an_id), (an_id, INVALID), (an_id, an_id), (INVALID, INVALID))[kind]
            doubles[list(doubles)[kind]] += 1
            slots[t:t + 2], replies[t:t + 2] = q, pair
            t += 2
        else:
            slots[t], replies[t] = q, INVALID if kind == 7 else an_id
            t += 1
    assert t == m
    mix = rng.permutation(m)  # the two replies of a query lie anywhere, in both orders
    slots, replies = slots[mix], replies[mix]
    before = np.concatenate([PATTERN | np.arange(queries, dtype=np.uint64), [np.uint64(GUARD)]])
    want = before.copy()
    for t in range(m):
        if replies[t] != INVALID:
            want[slots[t]] = replies[t]
    d_out, d_replies, d_slots = to_device(before), to_device(np.append(replies, INVALID)), to_device(np.append(slots, np.uint32(queries)))
    torch.cuda.synchronize()
    d.route_combine_device(0, d_replies.data_ptr(), d_slots.data_ptr(), m, d_out.data_ptr(), stream=0 if stream is None else stream.cuda_stream)
    if stream is not None:
        stream.synchronize()
    torch.cuda.synchronize()
    got = to_host(d_out, np.uint64)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, ("route_combine", m, "first differing query", int(bad[0]), hex(int(got[bad[0]])), hex(int(want[bad[0]])))
    return doubles, int((replies == INVALID).sum()), int((replies != INVALID).sum())


def argument_error(call):
    import sshash_amd

    try:
        call()
    except sshash_amd.SSHashError as e:
        return e.status == ERR_ARGUMENT
    return False


# ---- C. R ranks as threads ---------------------------------------------------------------------------------------------------------
class _DevicePointer:
    """a raw device pointer as something torch.as_tensor accepts (sshash_amd/sharded.py)"""

    def __init__(self, ptr, nbytes):
        self.__cuda_array_interface__ = {"shape": (nbytes,), "typestr": "|u1", "data": (ptr, False), "version": 2}


class Hub:
    """where the R ranks meet: a rank that fails breaks the barrier, so every rank's exchange fails instead of waiting"""

    def __init__(self, R, timeout=120.0):
        self.R = R
        self.barrier = threading.Barrier(R, timeout=timeout)
        self.counts, self.send = [None] * R, [None] * R

    def exchange(self, rank, stream):
        import torch

        def counts_fn(send):
            self.counts[rank] = list(send)
            self.barrier.wait()
            got = [self.counts[p][rank] for p in range(self.R)]
            self.barrier.wait()
            return got

        def data_fn(send_ptr, send_counts, recv_ptr, recv_counts, elem_bytes, hip_stream):
            assert hip_stream == stream.cuda_stream
            stream.synchronize()  # my send buffer is complete
            self.send[rank] = (send_ptr, list(send_counts), elem_bytes)
            self.barrier.wait()
            at = 0
            with torch.cuda.stream(stream):
                for p in range(self.R):  # the block of rank p: what it holds for me, behind its blocks for the ranks before me
                    ptr, theirs, their_bytes = self.send[p]
                    assert their_bytes == elem_bytes and theirs[rank] == recv_counts[p], "the counts exchange and the data exchange disagree"
                    nbytes = recv_counts[p] * elem_bytes
                    if nbytes:
                        src = torch.as_tensor(_DevicePointer(ptr + sum(theirs[:rank]) * elem_bytes, nbytes), device="cuda:0")
                        torch.as_tensor(_DevicePointer(recv_ptr + at * elem_bytes, nbytes), device="cuda:0").copy_(src)
                    at += recv_counts[p]
            stream.synchronize()
            self.barrier.wait()  # nobody releases a buffer before every copy out of it is complete

        return counts_fn, data_fn


def sharded_rounds(handles, by_table, rounds, W):
    """rounds: [(check_rc, [batch of rank 0, batch of rank 1, ...])] -> got[round][rank], through R threads"""
    import torch

    R = len(handles)
    hub = Hub(R)
    got = [[None] * R for _ in rounds]
    errors = [None] * R

    def rank_main(r):
        try:
            stream = torch.cuda.Stream(device=0)
            counts_fn, data_fn = hub.exchange(r, stream)
            for j, (check_rc, batches) in enumerate(rounds):
                q = batches[r]
                n = q.size // W
                before = np.concatenate([PATTERN | np.arange(n, dtype=np.uint64), [np.uint64(GUARD)]])  # (not filled when every query has one owner)
                with torch.cuda.stream(stream):
                    d_q, d_out = to_device(q if n else np.zeros(W, dtype=np.uint64)), to_device(before)
                    stream.synchronize()
                    handles[r].sharded_lookup_device(0, R, by_table, d_q.data_ptr() if n else 0, n, d_out.data_ptr(), counts_fn, data_fn,
                                                     check_reverse_complement=check_rc, stream=stream.cuda_stream)
                    stream.synchronize()
                    got[j][r] = to_host(d_out, np.uint64)
        except BaseException as e:  # noqa: BLE001 -- reported by the main thread
            errors[r] = e
            hub.barrier.abort()

    threads = [threading.Thread(target=rank_main, args=(r,)) for r in range(R)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    first = [e for e in errors if e is not None and not isinstance(e, threading.BrokenBarrierError)] + [e for e in errors if e is not None]
    if first:
        raise first[0]
    return got


# ---- the batches -------------------------------------------------------------------------------------------------------------------
def random_kmers(rng, n, k, W):
    q = rng.integers(0, 1 << 63, (n, W), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, (n, W), dtype=np.uint64)
    q[:, W - 1] &= np.uint64((1 << (2 * k - 64 * (W - 1))) - 1)
    return q.reshape(-1)


def dictionary_kmers(case, rng, n):
    """n k-mers of the dictionary, every other one reverse-complemented"""
    pos = case.gt.kmers(rng.integers(0, case.gt.num_kmers, n)).reshape(n, case.W)
    pos[::2] = revcomp(pos[::2].reshape(-1), case.k, case.W).reshape(-1, case.W)
    return pos.reshape(-1)


def main():
    import torch

    import sshash_amd
    from conftest import Case, skewed_sequences
    from oracle import oracle as O

    k, m, canonical, seed, owners_exe, scratch = int(sys.argv[1]), int(sys.argv[2]), bool(int(sys.argv[3])), int(sys.argv[4]), sys.argv[5], sys.argv[6]
    case = Case(f"routing_k{k}_{int(canonical)}", skewed_sequences(k, m, seed=seed, canonical=canonical), k, m, canonical, scratch)
    W, num_kmers = case.W, case.gt.num_kmers
    magic = O.xxh64_u64(1, 0)  # as conftest.mmer_hash derives it (the build's seed is 1)
    d = case.dict.to_device(0)
    stats = d.device_stats(0)
    key_length = stats["sk_key_length"]
    assert stats["sk_slots"] > 0 and 0 < key_length <= k
    rng = np.random.default_rng(seed)
    kinds, forms = {}, set()

    def reference(kmers, shards=SHARDS):
        return Reference(kmers, k, m, W, canonical, magic, host_key_owners(owners_exe, kmers, k, key_length, shards))

    # ---- the batches of part B: a mixed pool whose prefixes are the batches of every size; uniform random k-mers; one k-mer; two k-mers
    n_pool = max(SIZES)
    pool = np.concatenate([dictionary_kmers(case, rng, n_pool // 2), random_kmers(rng, n_pool - n_pool // 2, k, W)]).reshape(n_pool, W)
    from_dictionary = np.concatenate([np.ones(n_pool // 2, dtype=bool), np.zeros(n_pool - n_pool // 2, dtype=bool)])
    perm = rng.permutation(n_pool)
    pool, from_dictionary = np.ascontiguousarray(pool[perm]).reshape(-1), from_dictionary[perm]
    assert (case.oracle.lookup_ids(pool)[from_dictionary] != INVALID).all()
    ref_pool = reference(pool)
    half = from_dictionary[:4097].sum()
    assert 1900 < half < 2200, half
    kinds["dictionary_kmers_in_the_mixed_batch"], kinds["random_kmers_in_the_mixed_batch"] = int(half), int(4097 - half)
    for attempt in range(64):  # a seed whose two-owner routing leaves no shard empty (regular dictionary: 8 messages per shard at 1024)
        uniform = random_kmers(np.random.default_rng(1000 * seed + attempt), 4097, k, W)
        ref_uniform = reference(uniform)
        smallest = {S: int(messages(*ref_uniform.owners(S, "minimizer", True), S)[0].min()) for S in (64, 1000, 1024)}
        if canonical or min(smallest.values()) > 0:
            break
    assert canonical or min(smallest.values()) > 0, smallest
    kinds["uniform_batch_seed_attempt"] = attempt

    # ---- A. the restated minimizer owners against route_device; properties of the table-key owners ----
    for kmers, ref in ((pool, ref_pool), (uniform, ref_uniform)):
        d_q = to_device(kmers)
        for S in SHARDS:
            owners = [torch.full((ref.n,), -1, dtype=torch.int32, device="cuda:0") for _ in range(2)]
            d.route_device(0, d_q.data_ptr(), ref.n, S, owners[0].data_ptr(), owners[1].data_ptr())
            torch.cuda.synchronize()
            f, r = ref.owners(S, "minimizer", True)
            for got, want, which in ((owners[0], f, "forward"), (owners[1], r, "reverse")):
                bad = np.flatnonzero(got.cpu().numpy() != want)
                assert bad.size == 0, ("route_device against the restated owners", S, which, "first differing query", int(bad[0]))
    back = host_key_owners(owners_exe, revcomp(pool, k, W), k, key_length, SHARDS)
    for S in SHARDS:
        assert (back[S] == ref_pool.key_owners[S]).all(), ("a k-mer and its reverse complement have different table-key owners", S)
        assert (ref_pool.key_owners[S] < S).all()
    whole_keys = stats["sk_keys"]
    shard_keys = []
    for r in range(3):
        part = sshash_amd.Dictionary.load(case.index_path).to_device(0, table_shards=3, table_shard_id=r)
        shard_keys.append(part.device_stats(0)["sk_keys"])
        part.close()
    assert sum(shard_keys) == whole_keys and all(0 < x < whole_keys for x in shard_keys), (shard_keys, whole_keys)
    kinds["table_keys"], kinds["table_keys_of_three_shards"] = whole_keys, shard_keys

    # ---- B. the two-call protocol ----
    side = torch.cuda.Stream(device=0)
    two_owner_fraction, per_shard = {}, {}
    plan = sorted({(S, 4097) for S in SHARDS} | {(S, n) for S in (3, 64) for n in SIZES} | {(1000, 257)})
    one_and_two = 0
    for S, n in plan:
        for entry, check_rc in ENTRIES:
            f, r = ref_pool.owners(S, entry, check_rc, slice(0, n))
            what = f"mixed batch, {entry} owners, check_rc={int(check_rc)}, S={S}, n={n}"
            counts = two_calls(d, entry, check_rc, pool, W, S, f, r, what)
            forms |= {f"W={W} SCATTER={s} BY_KEY={int(entry == 'key')}" for s in (0, 1)}
            if entry == "minimizer" and check_rc and not canonical and S >= 2 and n >= 255:
                assert 0 < int((f != r).sum()) < n, (what, "queries with two owners and queries with one")
                one_and_two += 1
            if (S, n) == (1000, 257):
                assert int((counts == 0).sum()) > 0, what
                kinds["empty_shards_at_S1000_n257_" + entry + str(int(check_rc))] = int((counts == 0).sum())
            if n == 4097:  # the uniform-random batch
                f, r = ref_uniform.owners(S, entry, check_rc)
                what = "uniform" + what[5:]
                counts = two_calls(d, entry, check_rc, uniform, W, S, f, r, what)
                if S == 64 or (S > 64 and entry == "minimizer" and check_rc and not canonical):
                    assert int(counts.min()) > 0, (what, "no shard is empty")
                    per_shard[f"S{S}_{entry}{int(check_rc)}"] = [int(counts.min()), int(counts.max())]
                if entry == "minimizer" and check_rc and not canonical:
                    two_owner_fraction[S] = round(float((f != r).mean()), 3)
    if not canonical:  # 1 - 1/S of uniform random k-mers have two owners (n = 4097: +- 0.05 is six standard deviations)
        assert abs(two_owner_fraction[2] - 0.50) < 0.05 and abs(two_owner_fraction[7] - 6 / 7) < 0.05, two_owner_fraction
    kinds["combinations_with_one_owner_and_two_owner_queries"] = one_and_two if not canonical else None
    kinds["two_owner_fraction_of_uniform_kmers"], kinds["messages_per_shard_min_max"] = two_owner_fraction, per_shard
    # the device gives a k-mer's reverse complement the table-key owner of the k-mer itself
    back_pool = revcomp(pool, k, W)
    for S in (3, 64, 1024):
        o = ref_pool.key_owners[S].astype(np.int64)
        two_calls(d, "key", True, back_pool, W, S, o, o, f"reverse complements of the mixed batch against the owners of the batch itself, key owners, S={S}")
    kinds["reverse_complement_batches"] = 3
    # one k-mer 4097 times (one owner, or one pair of owners); two k-mers with different owners in turn
    repeated_runs = alternating_runs = 0
    for S in (3, 64, 1024):
        for entry, check_rc in ENTRIES:
            f, r = ref_pool.owners(S, entry, check_rc)
            pick = [int(np.flatnonzero(f != r)[0])] if (f != r).any() else []
            pick.append(int(np.flatnonzero(f == r)[0]))
            for i in pick:
                index = np.full(4097, i)
                counts = two_calls(d, entry, check_rc, np.ascontiguousarray(pool.reshape(-1, W)[index]).reshape(-1), W, S, f[index], r[index],
                                   f"one k-mer 4097 times, {entry} owners, check_rc={int(check_rc)}, S={S}, owners {int(f[i])} {int(r[i])}")
                assert int((counts > 0).sum()) == (1 if f[i] == r[i] else 2) and int(counts.sum()) == 4097 * (1 if f[i] == r[i] else 2)
                repeated_runs += 1
            a = int(np.flatnonzero(f == r)[0])
            b = int(np.flatnonzero((f != f[a]) & (r != f[a]))[0])
            index = np.where(np.arange(4097) % 2 == 0, a, b)
            two_calls(d, entry, check_rc, np.ascontiguousarray(pool.reshape(-1, W)[index]).reshape(-1), W, S, f[index], r[index],
                      f"two k-mers in turn, {entry} owners, check_rc={int(check_rc)}, S={S}")
            alternating_runs += 1
    kinds["repeated_kmer_batches"], kinds["alternating_batches"] = repeated_runs, alternating_runs
    # a caller's stream: the same regions (every check above is on the regions as sets)
    for entry, check_rc in ENTRIES:
        f, r = ref_pool.owners(7, entry, check_rc, slice(0, 4097))
        two_calls(d, entry, check_rc, pool, W, 7, f, r, f"side stream, {entry} owners, check_rc={int(check_rc)}", stream=side)
    kinds["side_stream_runs"] = len(ENTRIES)
    # n = 0 writes nothing; bad arguments are refused before any launch
    tiny = to_device(np.full(16, GUARD, dtype=np.uint64))
    tiny32 = to_device(np.full(16, GUARD32, dtype=np.uint32))
    d_q = to_device(pool[:16 * W])
    torch.cuda.synchronize()
    for entry, check_rc in ENTRIES:
        bucket_call(d, entry, check_rc, d_q.data_ptr(), 0, 3, tiny.data_ptr())
        bucket_call(d, entry, check_rc, d_q.data_ptr(), 0, 3, tiny.data_ptr(), tiny.data_ptr() + 32, tiny32.data_ptr())
        bucket_call(d, entry, check_rc, 0, 0, 3, tiny.data_ptr())
        for S, n, send, slots in ((0, 4, 0, 0), (1025, 4, 0, 0), (3, 4, tiny.data_ptr() + 32, 0), (3, 4, 0, tiny32.data_ptr()), (3, 1 << 32, 0, 0),
                                  (3, 1 << 32, tiny.data_ptr() + 32, tiny32.data_ptr())):
            assert argument_error(lambda: bucket_call(d, entry, check_rc, d_q.data_ptr(), n, S, tiny.data_ptr(), send, slots)), (entry, S, n, send, slots)
    d.route_combine_device(0, tiny.data_ptr(), tiny32.data_ptr(), 0, tiny.data_ptr() + 64)
    torch.cuda.synchronize()
    assert (to_host(tiny, np.uint64) == GUARD).all() and (to_host(tiny32, np.uint32) == GUARD32).all(), "a call that had nothing to do, or was refused, wrote"
    # route_combine
    combine_kinds = {}
    for m_replies in (0, 1, 255, 257, 4097):
        for stream in (None, side):
            doubles, invalid, valid = combine_case(d, m_replies, np.random.default_rng(seed + m_replies), stream)
        if m_replies >= 255:
            assert all(v > 0 for v in doubles.values()) and invalid > 0 and valid > 0, (m_replies, doubles, invalid, valid)
            combine_kinds[m_replies] = dict(doubles, invalid_replies=invalid, ids=valid)
    kinds["combine"] = combine_kinds

    # ---- C. the whole sharded lookup ----
    every = case.gt.kmers(np.arange(num_kmers))
    one = dictionary_kmers(case, rng, 1)
    batches = [np.zeros(0, dtype=np.uint64), one, case.queries(128, 129, seed=seed + 1), case.queries(2048, 2049, seed=seed + 2),
               case.queries(4500, 4501, seed=seed + 3), np.tile(dictionary_kmers(case, rng, 2)[W:], 4097), random_kmers(rng, 257, k, W), None]
    names = ["empty", "one", "mixed_257", "mixed_4097", "mixed_9001", "one_kmer_4097_times", "negatives_only", "positives_of_a_single_owner"]
    assert (case.oracle.lookup_ids(batches[6]) == INVALID).all() and (case.oracle.lookup_ids(batches[5]) != INVALID).all()
    refs = [None if b is None or b.size == 0 else reference(b, RANKS) for b in batches]
    ref_every = reference(every, RANKS)
    sharded = {"runs_with_two_owner_queries": 0, "runs_where_every_query_has_one_owner": 0, "ranks_whose_batch_has_a_single_owner": 0,
               "owners_that_get_nothing_from_a_rank": 0, "queries": 0, "found": 0, "batches": {name: 0 for name in names}, "check_rc_0_rounds": 0}
    for R in RANKS:
        for by_table in (False, True):
            entry = "key" if by_table else "minimizer"
            if by_table:
                handles = [sshash_amd.Dictionary.load(case.index_path).to_device(0, table_shards=R, table_shard_id=r) for r in range(R)]
            else:
                handles = [sshash_amd.Dictionary.build(case.fasta, k=k, m=m, canonical=canonical, num_threads=4, num_shards=R, shard_id=r).to_device(0)
                           for r in range(R)]
            schedule = [(True, [(j * R + r) % len(batches) for r in range(R)]) for j in range(-(-len(batches) // R))]
            schedule.append((False, [(3 + r) % len(batches) for r in range(R)]))
            rounds, expected = [], []
            for check_rc, which in schedule:
                mine, owners = [], []
                for r, b in enumerate(which):
                    if batches[b] is None:  # the dictionary's k-mers whose owners are all one rank, the next one
                        f, o = ref_every.owners(R, entry, check_rc)
                        index = np.flatnonzero((f == (r + 1) % R) & (o == (r + 1) % R))[:1000]
                        assert index.size >= 16, (R, entry, index.size)
                        mine.append(np.ascontiguousarray(every.reshape(-1, W)[index]).reshape(-1))
                        owners.append((f[index], o[index]))
                    else:
                        mine.append(batches[b])
                        owners.append((np.zeros(0, dtype=np.int64),) * 2 if refs[b] is None else refs[b].owners(R, entry, check_rc))
                    sharded["batches"][names[b]] += 1
                    f, o = owners[-1]
                    if f.size:  # (what the library sees as total == n, from the reference)
                        sharded["runs_with_two_owner_queries" if (f != o).any() else "runs_where_every_query_has_one_owner"] += 1
                        got_some = np.bincount(np.concatenate([f, o]), minlength=R) > 0
                        sharded["ranks_whose_batch_has_a_single_owner"] += int(got_some.sum() == 1)
                        sharded["owners_that_get_nothing_from_a_rank"] += int((~got_some).sum())
                rounds.append((check_rc, mine))
                expected.append([case.oracle.lookup_ids(q, check_rc=check_rc) if q.size else np.zeros(0, dtype=np.uint64) for q in mine])
                sharded["check_rc_0_rounds"] += int(not check_rc)
            got = sharded_rounds(handles, by_table, rounds, W)
            for j, (check_rc, mine) in enumerate(rounds):
                for r in range(R):
                    want, ids = expected[j][r], got[j][r]
                    assert ids.size == want.size + 1 and int(ids[-1]) == GUARD, (R, entry, j, r, "the word behind the ids was written")
                    bad = np.flatnonzero(ids[:-1] != want)
                    assert bad.size == 0, ("sharded lookup", R, entry, "round", j, "rank", r, "check_rc", check_rc, "first differing query", int(bad[0]),
                                           hex(int(ids[bad[0]])), hex(int(want[bad[0]])), "of", want.size)
                    sharded["queries"] += want.size
                    sharded["found"] += int((want != INVALID).sum())
            forms |= {f"W={W} SCATTER={s} BY_KEY={int(by_table)} known owners" for s in (0, 1)}
            for h in handles:
                h.close()
    assert sharded["runs_where_every_query_has_one_owner"] > 0 and (canonical or sharded["runs_with_two_owner_queries"] > 0), sharded
    assert all(v > 0 for v in sharded["batches"].values()) and sharded["ranks_whose_batch_has_a_single_owner"] > 0, sharded
    assert sharded["owners_that_get_nothing_from_a_rank"] > 0 and 0 < sharded["found"] < sharded["queries"], sharded
    print(json.dumps({"ok": True, "k": k, "canonical": canonical, "num_kmers": num_kmers, "sk_key_length": key_length, "kinds": kinds, "sharded": sharded,
                      "forms": sorted(forms)}))


if __name__ == "__main__":
    main()
