// route_owners.cpp -- the HOST's election of the owner of a k-mer's table key (csrc/device_layout.hpp: sk_key, sk_owner), for
// tests/gpu_routing_worker.py to hold the device's route_bucket_kernel<*, *, BY_KEY> against: the same functions, compiled by
// g++ for the CPU, so what it catches is device code that disagrees with the host. Plain g++, no GPU.
//
//     route_owners <k> <table key length> <num_shards> [<num_shards> ...]  < packed k-mers (W uint64 each)  > owners
//
// For every k-mer on stdin, one uint32 per given num_shards on stdout (k-mer major): the owner of its table key, or -- a k-mer whose
// strands tie has no key -- of the first word of its smaller strand.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../sshash_amd/csrc/device_layout.hpp"

using namespace sshash_amd;

template <int W>
static int run(uint32_t k, uint32_t m, std::vector<uint32_t> const& shards) {
    uint64_t words[W];
    std::vector<uint32_t> out(shards.size());
    while (fread(words, sizeof(uint64_t), W, stdin) == size_t(W)) {
        kmer_w<W> x;
        for (int j = 0; j < W; ++j) x.w[j] = words[j];
        const kmer_w<W> x_rc = kmer_revcomp<W>(x, k);
        const sk_key_t kk = sk_key<W>(x, x_rc, k, m);
        const uint64_t key = kk.tie ? (kmer_less<W>(x_rc, x) ? x_rc.w[0] : x.w[0]) : kk.key;
        for (size_t s = 0; s < shards.size(); ++s) out[s] = sk_owner(key, shards[s]);
        if (fwrite(out.data(), sizeof(uint32_t), out.size(), stdout) != out.size()) return 2;
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 4) return fprintf(stderr, "usage: route_owners <k> <table key length> <num_shards>... < k-mers > owners\n"), 1;
    const uint32_t k = uint32_t(atoi(argv[1])), m = uint32_t(atoi(argv[2]));
    if (k < 1 || k > 63 || m < 1 || m > k || m > 31) return fprintf(stderr, "bad k or key length\n"), 1;
    std::vector<uint32_t> shards;
    for (int i = 3; i < argc; ++i) {
        const int s = atoi(argv[i]);
        if (s < 1) return fprintf(stderr, "bad num_shards\n"), 1;
        shards.push_back(uint32_t(s));
    }
    return k <= 31 ? run<1>(k, m, shards) : run<2>(k, m, shards);
}
