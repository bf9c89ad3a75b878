"""The k-mer iterator on the GPU (sshash_iterate_packed_device: Dictionary.kmers_device) and the whole-index check built on
it (sshash_check_device: Dictionary.check). Expected k-mers come from the input strings (GroundTruth, input order), expected
check failures from the CPU oracle."""
from __future__ import annotations

import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import sshash_amd
from conftest import ALL_SMALL_CASES, ROOT, random_dna
from test_iterate import sub_ranges

pytestmark = pytest.mark.gpu

INVALID = 0xFFFFFFFFFFFFFFFF
TILE = 2048  # ids per tile of iterate_kernel (csrc/engine.hip)
SENTINEL = 0x5A5A5A5A5A5A5A5A
CASES = ALL_SMALL_CASES + ["case_se_regular", "case_se_canonical", "case_k63_regular"]
FIELDS = ("kmers", "forward_not_found", "forward_other_id", "reverse_complement_wrong", "not_member", "first_failure")


def iterate_on_device(d, b, e, W):
    """kmers_device(b, e) into a torch buffer with TILE k-mers of sentinels on either side, on a non-default stream;
    returns (the k-mers, whether both margins kept their sentinels)"""
    import torch

    pad = TILE * W
    buf = torch.full(((e - b) * W + 2 * pad,), SENTINEL, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    s = torch.cuda.Stream(device="cuda:0")
    d.kmers_device(0, b, e, buf.data_ptr() + pad * 8, stream=s.cuda_stream)
    s.synchronize()
    host = buf.cpu().numpy().view(np.uint64)
    margins = (host[:pad] == SENTINEL).all() and (host[host.size - pad:] == SENTINEL).all()
    return host[pad:host.size - pad], margins


@pytest.mark.parametrize("case_name", CASES)
def test_kmers_device(case_name, request):
    case = request.getfixturevalue(case_name)
    d = case.dict
    d.to_device(0)
    n = d.num_kmers()
    got, margins = iterate_on_device(d, 0, n, case.W)
    assert margins
    assert np.array_equal(got, case.gt.kmers(np.arange(n)))
    assert np.array_equal(got, d.kmers())
    for b, e in sub_ranges(case, seed=1):
        got, margins = iterate_on_device(d, b, e, case.W)
        assert margins, (b, e)
        assert np.array_equal(got, case.gt.kmers(np.arange(b, e))), (b, e)
        assert np.array_equal(got, d.kmers(b, e)), (b, e)


def test_kmers_device_argument_errors(case_skew_regular):
    d = case_skew_regular.dict
    d.to_device(0)
    n = d.num_kmers()
    for b, e in ((5, 4), (0, n + 1)):
        with pytest.raises(sshash_amd.SSHashError) as err:
            d.kmers_device(0, b, e, 0)
        assert err.value.status == 1, (b, e)
    d.kmers_device(0, 7, 7, 0)  # empty: writes nothing, needs no buffer
    with pytest.raises(sshash_amd.SSHashError) as err:
        d.kmers_device(0, 0, 4, 0)  # NULL output with a range
    assert err.value.status == 1
    import torch

    fresh = sshash_amd.Dictionary.load(case_skew_regular.index_path)
    buf = torch.zeros(4, dtype=torch.int64, device="cuda:0")
    with pytest.raises(sshash_amd.SSHashError) as err:
        fresh.kmers_device(0, 0, 4, buf.data_ptr())  # no replica on device 0
    assert err.value.status == 5
    assert (buf.cpu() == 0).all()
    with pytest.raises(sshash_amd.SSHashError) as err:
        fresh.check(0)
    assert err.value.status == 5


@pytest.mark.parametrize("case_name", CASES)
def test_check(case_name, request):
    case = request.getfixturevalue(case_name)
    d = case.dict
    d.to_device(0)
    r = d.check(0)
    assert r == dict(zip(FIELDS, (d.num_kmers(), 0, 0, 0, 0, INVALID))), r


@pytest.mark.parametrize("case_name", ["case_skew_regular", "case_k63_canonical"])
def test_check_table_shard(case_name, request):
    case = request.getfixturevalue(case_name)
    d = sshash_amd.Dictionary.load(case.index_path)
    d.to_device(0, table_shards=2, table_shard_id=1)
    assert d.check(0) == dict(zip(FIELDS, (d.num_kmers(), 0, 0, 0, 0, INVALID)))
    n = d.num_kmers()
    got, margins = iterate_on_device(d, 0, n, case.W)
    assert margins and np.array_equal(got, case.gt.kmers(np.arange(n)))


def test_check_refuses_a_minimizer_shard(case_skew_regular):
    d = sshash_amd.Dictionary.build(case_skew_regular.fasta, k=31, m=11, num_threads=2, num_shards=2, shard_id=0)
    d.to_device(0)
    with pytest.raises(sshash_amd.SSHashError) as err:
        d.check(0)
    assert err.value.status == 1
    n = d.num_kmers()  # the strings are complete in a shard: the iterator still works
    got, margins = iterate_on_device(d, 0, n, 1)
    assert margins and np.array_equal(got, case_skew_regular.gt.kmers(np.arange(n)))


@pytest.mark.parametrize("canonical", [False, True], ids=["regular", "canonical"])
def test_check_counts_failures_as_the_oracle_predicts(tmp_path, canonical):
    """One short string occurs twice among random ones: each of its k-mers has two ids, a lookup answers one of them, and the
    other fails. The counts of each kind of failure are what the oracle predicts for every id. WHICH of the two ids a lookup
    answers is not fixed for such an input (it breaks the one-occurrence rule of a spectrum-preserving string set): the oracle
    returns the first position of the bucket, the device's super-k-mer table may return the other. So, from the oracle: the
    failing ids lie in the two copies, and of the two ids of one k-mer exactly one fails, forward and reverse-complemented. The
    smallest failing id is then the one the library's own lookups of the same k-mers give, and is checked against both."""
    from conftest import Case

    rng = np.random.default_rng(17 + canonical)
    k = 31
    dup = random_dna(rng, k + 6)
    seqs = [random_dna(rng, int(rng.integers(k, 4 * k))) for _ in range(60)]
    seqs.insert(13, dup)
    seqs.insert(41, dup)
    case = Case("dup_%d" % canonical, seqs, k, 13, canonical, str(tmp_path))
    d = case.dict
    d.to_device(0)
    n = d.num_kmers()
    ids = np.arange(n, dtype=np.uint64)
    fwd_q = case.gt.kmers(ids)
    rc_q = case.gt._revcomp(fwd_q)
    first = np.concatenate([[0], np.cumsum([len(x) - k + 1 for x in seqs])])
    size = len(dup) - k + 1
    copy_a, copy_b = np.arange(first[13], first[13] + size), np.arange(first[41], first[41] + size)
    in_copies = np.zeros(n, dtype=bool)
    in_copies[copy_a] = in_copies[copy_b] = True

    def failures(fwd, rc):
        not_found = fwd == np.uint64(INVALID)
        other = ~not_found & (fwd != ids)
        rc_wrong = rc != ids
        return not_found, other, rc_wrong

    o_nf, o_other, o_rc = failures(case.oracle.lookup_packed(fwd_q, True)["kmer_id"], case.oracle.lookup_packed(rc_q, True)["kmer_id"])
    l_nf, l_other, l_rc = failures(d.lookup(fwd_q).kmer_id, d.lookup(rc_q).kmer_id)
    # the oracle's picture: no k-mer missing, failures only inside the copies, one of the two ids of every k-mer
    assert not o_nf.any() and not (o_other | o_rc)[~in_copies].any()
    assert (o_other[copy_a] ^ o_other[copy_b]).all() and (o_rc[copy_a] ^ o_rc[copy_b]).all()
    # the library's lookups draw the same picture, whichever copy they answer
    assert not l_nf.any() and not (l_other | l_rc)[~in_copies].any()
    assert (l_other[copy_a] ^ l_other[copy_b]).all() and (l_rc[copy_a] ^ l_rc[copy_b]).all()

    got = d.check(0)
    want_counts = (n, 0, int(o_other.sum()), int(o_rc.sum()), 0)
    assert size > 0 and want_counts[2] == want_counts[3] == size
    assert tuple(got[f] for f in FIELDS[:5]) == want_counts, got
    assert got["first_failure"] in set(copy_a.tolist()) | set(copy_b.tolist()), got
    assert got["first_failure"] == int(ids[l_other | l_rc].min()), got
    assert (d.is_member(fwd_q) != 0).all()


def test_check_leaves_no_scratch_behind(case_se_regular):
    """check() makes a stream of its own and hands back the lookup scratch the replica kept for it: repeated calls -- more
    than the replica keeps streams for -- do not take device memory with them."""
    import torch

    d = case_se_regular.dict
    d.to_device(0)
    want = dict(zip(FIELDS, (d.num_kmers(), 0, 0, 0, 0, INVALID)))
    assert d.check(0) == want
    torch.cuda.synchronize()
    free_before, _ = torch.cuda.mem_get_info(0)
    for _ in range(20):
        assert d.check(0) == want
    torch.cuda.synchronize()
    free_after, _ = torch.cuda.mem_get_info(0)
    assert free_before - free_after < (64 << 20), (free_before, free_after)


def test_table_less_replica(tmp_path):
    """SSHASH_AMD_SKTABLE=0 (set as test_gpu_parity.py::test_accelerators_disabled sets it, in a child process): a replica
    without the super-k-mer table iterates and checks the same."""
    script = tmp_path / "tableless.py"
    script.write_text(textwrap.dedent(
        """
        import os, sys, tempfile
        import numpy as np
        sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
        import conftest as c
        import torch
        from test_gpu_iterate import FIELDS, INVALID, iterate_on_device
        from test_iterate import sub_ranges
        with tempfile.TemporaryDirectory() as tmp:
            for name, k, m, canonical, seed in (("r31", 31, 11, False, 3), ("c31", 31, 11, True, 5), ("c63", 63, 17, True, 11),
                                                ("r15", 15, 7, False, 13)):
                case = c.Case(name, c.skewed_sequences(k, m, seed=seed, n_heavy=60, n_plain=30), k, m, canonical, tmp)
                d = case.dict.to_device(0)
                assert d.device_stats()["sk_slots"] == 0
                for b, e in sub_ranges(case, seed=2, n_random=40):
                    got, margins = iterate_on_device(d, b, e, case.W)
                    assert margins and np.array_equal(got, case.gt.kmers(np.arange(b, e))), (name, b, e)
                r = d.check(0)
                assert r == dict(zip(FIELDS, (d.num_kmers(), 0, 0, 0, 0, INVALID))), (name, r)
        print("TABLELESS OK")
        """))
    env = dict(os.environ)
    env.pop("SSHASH_AMD_DIRECTORY", None)
    env.pop("SSHASH_AMD_TEST_HOOKS", None)
    env["SSHASH_AMD_SKTABLE"] = "0"
    p = subprocess.run([sys.executable, str(script), ROOT], env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "TABLELESS OK" in p.stdout, p.stdout + p.stderr
