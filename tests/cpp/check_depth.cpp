// check_depth.cpp -- the streaming depth over the C++ facade (include/sshash_amd.hpp):
//   [A] depth[i] of streaming_depth is the number of places where streaming_lookup over the same reads returns kmer_id == i, word for word;
//       its sum is num_positive_kmers; its report is the batch's report of streaming_query_per_read;
//   [B] the array is added into: a second batch into the array of the first gives the sum, values set by the caller survive (modulo 2^32);
//   [C] the same array out of the runs of streaming_runs, as a difference array: +1 at a run's first id, -1 behind its last, a prefix sum;
//       (depth != 0) is the bitmap of streaming_cover;
//   [D] depth_string_sums: per string the 64-bit sum over its ids, their sum the array's;
//   [E] streaming_depth_from_file over the second batch written as FASTA, into the array of the first: the sum of [B], the same report.
// Reads: those of check_cover.cpp (windows of the dictionary's own strings, either strand, with substitutions and N's; two windows glued
// together; random reads; reads shorter than k), a whole string, its reverse complement, and one window many times.
// Usage: check_depth <input.fa[.gz]> <k> <m> [--canonical]
#include <algorithm>
#include <cctype>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <filesystem>
#include <fstream>
#include <iostream>
#include <random>
#include <string>
#include <vector>

#include "sshash_amd.hpp"

using namespace sshash_amd;

static std::string string_of(dictionary const& dict, uint64_t string_id, uint64_t at_most) {
    const uint64_t k = dict.k();
    const auto [begin, end] = dict.string_offsets(string_id);
    const uint64_t first_id = begin - string_id * (k - 1), n = std::min(end - begin - k + 1, at_most);
    std::string s(k, 0), kmer(k, 0);
    dict.access(first_id, s.data());
    for (uint64_t i = 1; i < n; ++i) {
        dict.access(first_id + i, kmer.data());
        s.push_back(kmer[k - 1]);
    }
    return s;
}

static std::string reverse_complement(std::string const& s) {
    std::string r(s.rbegin(), s.rend());
    for (char& c : r) c = c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : c == 'T' ? 'A' : c;
    return r;
}

struct batch {
    std::string bases;
    std::vector<uint64_t> offsets{0};
    void add(std::string const& r) {
        bases += r;
        offsets.push_back(bases.size());
    }
    uint64_t size() const { return offsets.size() - 1; }
};

/* the depth out of the per-k-mer ids of streaming_lookup */
static std::vector<uint32_t> depth_of_lookup(dictionary const& dict, batch const& b) {
    lookup_results per_kmer;
    dict.streaming_lookup(b.bases.data(), b.offsets.data(), b.size(), per_kmer);
    std::vector<uint32_t> depth(dict.num_kmers(), 0);
    const uint64_t k = dict.k();
    for (uint64_t r = 0; r < b.size(); ++r) {
        const uint64_t lo = b.offsets[r], len = b.offsets[r + 1] - lo;
        for (uint64_t j = 0; j + k <= len; ++j) {
            const uint64_t id = per_kmer.kmer_id[lo + j];
            if (id != constants::invalid_uint64) ++depth[id];
        }
    }
    return depth;
}

template <typename T>
static bool same(std::vector<T> const& got, std::vector<T> const& want, char const* what) {
    if (got.size() != want.size()) {
        std::cerr << what << ": " << got.size() << " words, expected " << want.size() << std::endl;
        return false;
    }
    for (uint64_t i = 0; i < got.size(); ++i)
        if (got[i] != want[i]) {
            std::cerr << what << ": word " << i << " is " << got[i] << ", expected " << want[i] << std::endl;
            return false;
        }
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
        dict.to_device(0);
        const uint64_t k = dict.k();
        std::mt19937_64 rng(7);
        auto below = [&](uint64_t n) { return uint64_t(rng() % n); };
        auto window = [&]() {
            const std::string s = string_of(dict, below(dict.num_strings()), 400);
            std::string r = s.substr(below(s.size() - k + 1), 60 + below(200));
            return below(2) ? reverse_complement(r) : r;
        };
        batch one, two;
        for (uint64_t i = 0; i < 300; ++i) {
            batch& b = i % 2 ? two : one;
            std::string r = window();
            for (char& c : r) {
                const uint64_t u = below(1000);
                if (u < 10) c = "ACGT"[below(4)];
                else if (u < 15) c = 'N';
            }
            if (i % 5 == 0)
                for (char& c : r) c = char(std::tolower(c));
            b.add(r);
            b.add(window() + window());
            std::string junk(1 + below(150), 'A');
            for (char& c : junk) c = "ACGT"[below(4)];
            b.add(junk);
            if (i % 7 == 0) b.add(std::string(below(k), 'C'));
        }
        one.add("");
        one.add(string_of(dict, 0, 400));
        two.add(reverse_complement(string_of(dict, dict.num_strings() - 1, 400)));
        const std::string often = window();
        for (uint64_t i = 0; i < 500; ++i) one.add(often);
        std::cout << "checking the streaming depth on " << one.size() + two.size() << " reads, " << one.bases.size() + two.bases.size() << " bases..." << std::endl;
        bool ok = true;
        const uint64_t n = dict.num_kmers();

        /* [A] */
        const std::vector<uint32_t> want_one = depth_of_lookup(dict, one), want_two = depth_of_lookup(dict, two);
        std::vector<uint32_t> depth;
        const streaming_query_report rep = dict.streaming_depth(one.bases.data(), one.offsets.data(), one.size(), depth);
        ok = ok && same(depth, want_one, "[A] the first batch");
        std::vector<streaming_query_report> rows;
        const streaming_query_report plain = dict.streaming_query_per_read(one.bases.data(), one.offsets.data(), one.size(), rows);
        if (rep.num_kmers != plain.num_kmers || rep.num_positive_kmers != plain.num_positive_kmers || rep.num_negative_kmers != plain.num_negative_kmers ||
            rep.num_invalid_kmers != plain.num_invalid_kmers || rep.num_searches != plain.num_searches || rep.num_extensions != plain.num_extensions) {
            std::cerr << "[A] the report differs from streaming_query_per_read's: " << rep.num_positive_kmers << " positive against " << plain.num_positive_kmers << std::endl;
            ok = false;
        }
        uint64_t sum = 0, held = 0, deepest = 0;
        for (uint32_t c : depth) sum += c, held += c != 0, deepest = std::max<uint64_t>(deepest, c);
        if (sum != rep.num_positive_kmers || held == 0 || held >= n || deepest < 500) {
            std::cerr << "[A] the depths sum to " << sum << " for " << rep.num_positive_kmers << " positive k-mers; " << held << " of " << n << " held, at most "
                      << deepest << " times" << std::endl;
            ok = false;
        }

        /* [B] */
        std::vector<uint32_t> both = depth, want_both(n);
        for (uint64_t i = 0; i < n; ++i) want_both[i] = want_one[i] + want_two[i];
        const streaming_query_report rep_two = dict.streaming_depth(two.bases.data(), two.offsets.data(), two.size(), both);
        ok = ok && same(both, want_both, "[B] the second batch into the array of the first");
        std::vector<uint32_t> kept(n, 0), want_kept = want_two;
        for (uint64_t i = 0; i < n; i += 3) {
            const uint32_t mine = i % 5 ? uint32_t(i * 2654435761u) : 0xFFFFFFFFu;  // (values that wrap when something is added)
            kept[i] = mine;
            want_kept[i] += mine;
        }
        dict.streaming_depth(two.bases.data(), two.offsets.data(), two.size(), kept);
        ok = ok && same(kept, want_kept, "[B] values set before the call");

        /* [C] */
        std::vector<uint64_t> run_offsets;
        std::vector<sshash_streaming_run> runs;
        dict.streaming_runs(one.bases.data(), one.offsets.data(), one.size(), run_offsets, runs);
        std::vector<uint32_t> from_runs(n + 1, 0);
        uint64_t forward_runs = 0, backward_runs = 0;
        for (sshash_streaming_run const& run : runs) {
            const uint64_t count = run.num_kmers & ~SSHASH_RUN_BACKWARD;
            const bool backward = (run.num_kmers & SSHASH_RUN_BACKWARD) != 0;
            (backward ? backward_runs : forward_runs) += 1;
            const uint64_t lo = backward ? run.kmer_id + 1 - count : run.kmer_id;
            from_runs[lo] += 1;
            from_runs[lo + count] -= 1;
        }
        for (uint64_t i = 1; i < n; ++i) from_runs[i] += from_runs[i - 1];
        from_runs.resize(n);
        ok = ok && same(depth, from_runs, "[C] the difference array of the runs");
        if (forward_runs < 50 || backward_runs < 50) {
            std::cerr << "the reads exercise too little: " << forward_runs << " forward runs, " << backward_runs << " backward" << std::endl;
            ok = false;
        }
        std::vector<uint64_t> cover;
        dict.streaming_cover(one.bases.data(), one.offsets.data(), one.size(), cover);
        for (uint64_t i = 0; i < n && ok; ++i)
            if (((cover[i >> 6] >> (i & 63)) & 1) != uint64_t(depth[i] != 0)) {
                std::cerr << "[C] k-mer " << i << ": depth " << depth[i] << " against the bit of streaming_cover" << std::endl;
                ok = false;
            }

        /* [D] */
        std::vector<uint64_t> sums, want_sums(dict.num_strings(), 0);
        const uint64_t total = dict.depth_string_sums(kept, sums);
        uint64_t want_total = 0;
        for (uint64_t s = 0; s < dict.num_strings(); ++s) {
            const auto [begin, end] = dict.string_offsets(s);
            for (uint64_t id = begin - s * (k - 1); id < end - (s + 1) * (k - 1); ++id) want_sums[s] += kept[id];
            want_total += want_sums[s];
        }
        ok = ok && same(sums, want_sums, "[D] sums per string (CPU)");
        if (total != want_total || (want_total >> 32) == 0) {
            std::cerr << "[D] total " << total << ", expected " << want_total << " (and more than 32 bits of it)" << std::endl;
            ok = false;
        }
        /* [E] */
        const std::string path = (std::filesystem::temp_directory_path() / ("check_depth_" + std::to_string(k) + (cfg.canonical ? "c" : "r") + ".fa")).string();
        {
            std::ofstream f(path);
            for (uint64_t r = 0; r < two.size(); ++r)
                if (two.offsets[r + 1] > two.offsets[r]) f << ">" << r << "\n" << two.bases.substr(two.offsets[r], two.offsets[r + 1] - two.offsets[r]) << "\n";
        }
        std::vector<uint32_t> from_file = depth;
        const streaming_query_report file_rep = dict.streaming_depth_from_file(path, false, from_file);
        std::remove(path.c_str());
        ok = ok && same(from_file, want_both, "[E] the file of the second batch into the array of the first");
        if (file_rep.num_kmers != rep_two.num_kmers || file_rep.num_positive_kmers != rep_two.num_positive_kmers || file_rep.num_searches != rep_two.num_searches ||
            file_rep.num_extensions != rep_two.num_extensions || file_rep.num_positive_kmers == 0) {
            std::cerr << "[E] the file's report differs from the in-memory call's: " << file_rep.num_positive_kmers << " positive against " << rep_two.num_positive_kmers << std::endl;
            ok = false;
        }
        if (ok) std::cout << "EVERYTHING OK! " << held << " of " << n << " k-mers held by the first batch, " << sum << " times in all, one of them " << deepest << " times" << std::endl;
        return ok ? 0 : 1;
    } catch (std::exception const& e) {
        std::cerr << "error: " << e.what() << std::endl;
        return 1;
    }
}
