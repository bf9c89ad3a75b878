// table_keys.cpp -- the HOST's view of the super-k-mer table's key election (csrc/device_layout.hpp: sk_key), for
// tests/gpu_even_m_worker.py to find out which k-mers have no table key (the two strands elect equal hashes: a tie) before a
// batch is sent to a device -- so that a batch of ties is chosen, not hoped for. The same function the kernels run, compiled by
// g++ for the CPU. Plain g++, no GPU.
//
//     table_keys <k> <table key length>  < packed k-mers (W uint64 each)  > records
//
// For every k-mer on stdin one 16-byte record on stdout, the fields of sk_key_t as sk_key gives them:
//     uint8 tie, uint8 rc, uint16 pos, uint32 zero, uint64 key
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "../../sshash_amd/csrc/device_layout.hpp"

using namespace sshash_amd;

struct record {
    uint8_t tie, rc;
    uint16_t pos;
    uint32_t zero;
    uint64_t key;
};
static_assert(sizeof(record) == 16, "one record is 16 bytes");

template <int W>
static int run(uint32_t k, uint32_t m) {
    uint64_t words[W];
    while (fread(words, sizeof(uint64_t), W, stdin) == size_t(W)) {
        kmer_w<W> x;
        for (int j = 0; j < W; ++j) x.w[j] = words[j];
        const sk_key_t kk = sk_key<W>(x, kmer_revcomp<W>(x, k), k, m);
        const record out = {uint8_t(kk.tie), uint8_t(kk.rc), uint16_t(kk.pos), 0u, kk.key};
        if (fwrite(&out, sizeof(out), 1, stdout) != 1) return 2;
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc != 3) return fprintf(stderr, "usage: table_keys <k> <table key length> < k-mers > records\n"), 1;
    const uint32_t k = uint32_t(atoi(argv[1])), m = uint32_t(atoi(argv[2]));
    if (k < 1 || k > 63 || m < 1 || m > k || m > 31) return fprintf(stderr, "bad k or key length\n"), 1;
    return k <= 31 ? run<1>(k, m) : run<2>(k, m);
}
