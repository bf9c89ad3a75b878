// check_iterators.cpp -- the reference's iterator checkers, re-expressed over the C++ facade (include/sshash_amd.hpp):
//   [A] check_correctness_kmer_iterator: per thread, at_kmer_id(start) walked to the end of the thread's range; every
//       (kmer_id, kmer) equals (start, access(start))                              (reference test/check.hpp:177-227)
//   [B] check_correctness_string_iterator: at_string_id(s) for every string; ids run from string_offsets(s).begin - s*(k-1)
//       and every k-mer equals access(id)                                          (reference test/check.hpp:229-289)
//   [C] begin(): the whole dictionary, has_next() false exactly after num_kmers() k-mers
// Host only: the iterator decodes the host index (sshash_iterate_packed), access() too.
// Usage: check_iterators <input.fa[.gz]> <k> <m> [--canonical]
#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "sshash_amd.hpp"

using namespace sshash_amd;

/* util::uint_kmer_to_string (reference include/util.hpp): 2 bits per base, first base lowest, alphabet "ACTG" */
static void uint_kmer_to_string(uint_kmer_t const& x, char* out, uint64_t k) {
    static const char alphabet[] = "ACTG";
    for (uint64_t i = 0; i < k; ++i) out[i] = alphabet[(x.bits[i >> 5] >> (2 * (i & 31))) & 3];
}

static uint64_t threads_for(uint64_t n) {
    const uint64_t hc = std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
    return std::max<uint64_t>(1, std::min(hc, n));
}

template <typename Worker>
static void run_threads(uint64_t n, Worker const& worker) {
    const uint64_t nt = threads_for(n), chunk = (n + nt - 1) / nt;
    std::vector<std::thread> threads;
    for (uint64_t t = 0; t < nt; ++t) {
        const uint64_t start = t * chunk, end = std::min(n, start + chunk);
        if (start >= end) break;
        threads.emplace_back(worker, start, end);
    }
    for (auto& th : threads) th.join();
}

static bool check_correctness_kmer_iterator(dictionary const& dict) {
    const uint64_t k = dict.k();
    std::cout << "checking correctness of kmer iterator..." << std::endl;
    std::atomic<bool> ok{true};
    std::mutex print_mutex;
    run_threads(dict.num_kmers(), [&](uint64_t start, uint64_t end) {
        std::string read_kmer(k, 0), expected_kmer(k, 0);
        for (auto it = dict.at_kmer_id(start); start != end; ++start) {
            auto [kmer_id, kmer] = it.next();
            uint_kmer_to_string(kmer, read_kmer.data(), k);
            dict.access(kmer_id, expected_kmer.data());
            if (read_kmer != expected_kmer || kmer_id != start) {
                std::lock_guard<std::mutex> lock(print_mutex);
                std::cerr << "got (" << kmer_id << ",'" << read_kmer << "') but expected (" << start << ",'" << expected_kmer
                          << "')" << std::endl;
                ok = false;
                return;
            }
        }
    });
    if (!ok) return false;
    std::cout << "EVERYTHING OK!" << std::endl;
    return true;
}

static bool check_correctness_string_iterator(dictionary const& dict) {
    const uint64_t k = dict.k();
    std::cout << "checking correctness of string iterator..." << std::endl;
    std::atomic<bool> ok{true};
    std::mutex print_mutex;
    run_threads(dict.num_strings(), [&](uint64_t start, uint64_t end) {
        std::string read_kmer(k, 0), expected_kmer(k, 0);
        for (uint64_t string_id = start; string_id < end; ++string_id) {
            auto [begin, string_end] = dict.string_offsets(string_id);
            uint64_t from_kmer_id = begin - string_id * (k - 1);
            const uint64_t expected_end = string_end - (string_id + 1) * (k - 1);
            auto it = dict.at_string_id(string_id);
            while (it.has_next()) {
                auto [kmer_id, kmer] = it.next();
                uint_kmer_to_string(kmer, read_kmer.data(), k);
                dict.access(kmer_id, expected_kmer.data());
                if (read_kmer != expected_kmer || kmer_id != from_kmer_id) {
                    std::lock_guard<std::mutex> lock(print_mutex);
                    std::cerr << "ERROR at string_id " << string_id << ": got (" << kmer_id << ", '" << read_kmer
                              << "') but expected (" << from_kmer_id << ", '" << expected_kmer << "')" << std::endl;
                    ok = false;
                    return;
                }
                ++from_kmer_id;
            }
            if (from_kmer_id != expected_end) {
                std::lock_guard<std::mutex> lock(print_mutex);
                std::cerr << "ERROR at string_id " << string_id << ": iterator stopped at id " << from_kmer_id << ", string ends at "
                          << expected_end << std::endl;
                ok = false;
                return;
            }
        }
    });
    if (!ok) return false;
    std::cout << "checked " << dict.num_strings() << " strings" << std::endl;
    std::cout << "EVERYTHING OK!" << std::endl;
    return true;
}

static bool check_begin(dictionary const& dict) {
    std::cout << "checking begin() over the whole dictionary..." << std::endl;
    const uint64_t k = dict.k();
    std::string read_kmer(k, 0), expected_kmer(k, 0);
    uint64_t count = 0;
    for (auto it = dict.begin(); it.has_next(); ++count) {
        auto [kmer_id, kmer] = it.next();
        if (kmer_id != count) {
            std::cerr << "begin(): id " << kmer_id << " at position " << count << std::endl;
            return false;
        }
        if (count % 997 == 0) {  // the k-mers themselves are [A]'s business: a sample here
            uint_kmer_to_string(kmer, read_kmer.data(), k);
            dict.access(kmer_id, expected_kmer.data());
            if (read_kmer != expected_kmer) {
                std::cerr << "begin(): k-mer " << kmer_id << " is '" << read_kmer << "', expected '" << expected_kmer << "'" << std::endl;
                return false;
            }
        }
    }
    if (count != dict.num_kmers()) {
        std::cerr << "begin(): " << count << " k-mers, expected " << dict.num_kmers() << std::endl;
        return false;
    }
    std::cout << "EVERYTHING OK!" << std::endl;
    return true;
}

int main(int argc, char** argv) {
    if (argc < 4) {
        std::cerr << "usage: " << argv[0] << " <input.fa[.gz]> <k> <m> [--canonical]" << std::endl;
        return 2;
    }
    build_configuration cfg;
    cfg.k = std::strtoull(argv[2], nullptr, 10);
    cfg.m = std::strtoull(argv[3], nullptr, 10);
    cfg.canonical = argc > 4 && std::strcmp(argv[4], "--canonical") == 0;
    cfg.num_threads = 4;
    try {
        dictionary dict;
        dict.build(argv[1], cfg);
        std::cout << "k = " << dict.k() << ", " << dict.num_kmers() << " k-mers, " << dict.num_strings() << " strings"
                  << (dict.canonical() ? ", canonical" : "") << std::endl;
        const bool ok = check_correctness_kmer_iterator(dict) && check_correctness_string_iterator(dict) && check_begin(dict);
        return ok ? 0 : 1;
    } catch (std::exception const& e) {
        std::cerr << "error: " << e.what() << std::endl;
        return 1;
    }
}
