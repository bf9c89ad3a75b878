// table_hashes.cpp -- the HOST's view of where the super-k-mer table puts a key (csrc/device_layout.hpp: sk_hash, sk_filter_index,
// sk_owner, sk_kmer_key), for tests/table_reference.py: the functions the builder and the readers share, compiled by g++ for the
// CPU (tests/cpp/check_table_key.cpp tests them). Nothing of sktable.hip is in here. Plain g++, no GPU.
//
//     table_hashes hash <num_buckets> <num_shards>  < keys (uint64 each)              > records of 8 uint32:
//                                                     the five bucket choices, the 24-bit fingerprint, its filter index, the owner
//     table_hashes kmer_key <k>                     < packed k-mers (W uint64 each)   > sk_kmer_key of each (uint64)
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../sshash_amd/csrc/device_layout.hpp"

using namespace sshash_amd;

static int hashes(uint32_t num_buckets, uint32_t num_shards) {
    uint64_t key;
    while (fread(&key, sizeof(key), 1, stdin) == 1) {
        const sk_hash_t h = sk_hash(key, num_buckets);
        uint32_t out[8];
        for (uint32_t c = 0; c < SK_CHOICES; ++c) out[c] = h.bucket[c];
        out[5] = h.fingerprint;
        out[6] = sk_filter_index(h.fingerprint);
        out[7] = sk_owner(key, num_shards);
        if (fwrite(out, sizeof(out), 1, stdout) != 1) return 2;
    }
    return 0;
}

template <int W>
static int kmer_keys(uint32_t k) {
    uint64_t words[W];
    while (fread(words, sizeof(uint64_t), W, stdin) == size_t(W)) {
        kmer_w<W> x;
        for (int j = 0; j < W; ++j) x.w[j] = words[j];
        const uint64_t key = sk_kmer_key<W>(x, kmer_revcomp<W>(x, k));
        if (fwrite(&key, sizeof(key), 1, stdout) != 1) return 2;
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 4 && strcmp(argv[1], "hash") == 0) {
        const long buckets = atol(argv[2]), shards = atol(argv[3]);
        if (buckets < 1 || buckets >= (1l << 32) || shards < 1) return fprintf(stderr, "bad number of buckets or shards\n"), 1;
        return hashes(uint32_t(buckets), uint32_t(shards));
    }
    if (argc == 3 && strcmp(argv[1], "kmer_key") == 0) {
        const uint32_t k = uint32_t(atoi(argv[2]));
        if (k < 1 || k > 63) return fprintf(stderr, "bad k\n"), 1;
        return k <= 31 ? kmer_keys<1>(k) : kmer_keys<2>(k);
    }
    return fprintf(stderr, "usage: table_hashes hash <num_buckets> <num_shards> < keys | table_hashes kmer_key <k> < k-mers\n"), 1;
}
