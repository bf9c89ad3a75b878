// check_sums.cpp -- the streaming sums over the C++ facade (include/sshash_amd.hpp):
//   [A] row r of streaming_sums is (the sum of values[id], the number) of the places of read r where streaming_lookup over the same reads
//       returns a k-mer id; positive_kmers is num_positive_kmers of the read's row of streaming_query_per_read, the report is that call's;
//   [B] at_least: the sum counts the read's k-mers with values[id] >= at_least; values that are all 0xFFFFFFFF: sums of more than 32 bits;
//   [C] the same rows out of the runs of streaming_runs over a prefix sum of the checker's own: a run of ids [lo, hi) is worth P[hi] - P[lo];
//   [D] streaming_sums_from_file over the reads written as FASTA: the same rows in file order; a callback's non-zero return stops the query.
// Reads: those of check_depth.cpp (windows of the dictionary's own strings, either strand, with substitutions and N's; two windows glued
// together; random reads; reads shorter than k; an empty read), a whole string and a reverse complement.
// Usage: check_sums <input.fa[.gz]> <k> <m> [--canonical]
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
    std::string read(uint64_t r) const { return bases.substr(offsets[r], offsets[r + 1] - offsets[r]); }
};

static bool same(std::vector<sshash_read_sum> const& got, std::vector<sshash_read_sum> const& want, char const* what) {
    if (got.size() != want.size()) {
        std::cerr << what << ": " << got.size() << " rows, expected " << want.size() << std::endl;
        return false;
    }
    for (uint64_t i = 0; i < got.size(); ++i)
        if (got[i].sum != want[i].sum || got[i].positive_kmers != want[i].positive_kmers) {
            std::cerr << what << ": read " << i << " is (" << got[i].sum << ", " << got[i].positive_kmers << "), expected (" << want[i].sum << ", "
                      << want[i].positive_kmers << ")" << std::endl;
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
        const uint64_t k = dict.k(), n = dict.num_kmers();
        std::mt19937_64 rng(7);
        auto below = [&](uint64_t m) { return uint64_t(rng() % m); };
        auto window = [&]() {
            const std::string s = string_of(dict, below(dict.num_strings()), 400);
            std::string r = s.substr(below(s.size() - k + 1), 60 + below(200));
            return below(2) ? reverse_complement(r) : r;
        };
        batch b;
        for (uint64_t i = 0; i < 300; ++i) {
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
            if (i % 7 == 0) b.add(std::string(1 + below(k - 1), 'C'));
        }
        b.add(string_of(dict, 0, 400));
        b.add(reverse_complement(string_of(dict, dict.num_strings() - 1, 400)));
        const uint64_t in_file = b.size();  // (the file form has a row per record: the empty read comes behind the reads that go into the file)
        b.add("");
        std::cout << "checking the streaming sums on " << b.size() << " reads, " << b.bases.size() << " bases..." << std::endl;
        bool ok = true;

        std::vector<uint32_t> values(n);
        for (uint64_t i = 0; i < n; ++i) values[i] = uint32_t(rng() % 1000);
        lookup_results per_kmer;
        dict.streaming_lookup(b.bases.data(), b.offsets.data(), b.size(), per_kmer);
        auto truth = [&](std::vector<uint32_t> const& v, uint32_t at_least) {
            std::vector<sshash_read_sum> want(b.size(), sshash_read_sum{0, 0});
            for (uint64_t r = 0; r < b.size(); ++r) {
                const uint64_t lo = b.offsets[r], len = b.offsets[r + 1] - lo;
                for (uint64_t j = 0; j + k <= len; ++j) {
                    const uint64_t id = per_kmer.kmer_id[lo + j];
                    if (id == constants::invalid_uint64) continue;
                    want[r].sum += at_least ? uint64_t(v[id] >= at_least) : uint64_t(v[id]);
                    want[r].positive_kmers += 1;
                }
            }
            return want;
        };

        /* [A] */
        const std::vector<sshash_read_sum> want = truth(values, 0);
        std::vector<sshash_read_sum> sums;
        const streaming_query_report rep = dict.streaming_sums(b.bases.data(), b.offsets.data(), b.size(), values, 0, sums);
        ok = ok && same(sums, want, "[A] the rows");
        std::vector<streaming_query_report> rows;
        const streaming_query_report plain = dict.streaming_query_per_read(b.bases.data(), b.offsets.data(), b.size(), rows);
        if (rep.num_kmers != plain.num_kmers || rep.num_positive_kmers != plain.num_positive_kmers || rep.num_negative_kmers != plain.num_negative_kmers ||
            rep.num_invalid_kmers != plain.num_invalid_kmers || rep.num_searches != plain.num_searches || rep.num_extensions != plain.num_extensions) {
            std::cerr << "[A] the report differs from streaming_query_per_read's: " << rep.num_positive_kmers << " positive against " << plain.num_positive_kmers << std::endl;
            ok = false;
        }
        uint64_t positive = 0, hitless = 0;
        for (uint64_t r = 0; r < b.size() && ok; ++r) {
            positive += sums[r].positive_kmers;
            hitless += sums[r].positive_kmers == 0;
            if (sums[r].positive_kmers != rows[r].num_positive_kmers) {
                std::cerr << "[A] read " << r << ": " << sums[r].positive_kmers << " positive k-mers against " << rows[r].num_positive_kmers << " of its row" << std::endl;
                ok = false;
            }
        }
        if (ok && (positive != rep.num_positive_kmers || positive == 0 || hitless == 0)) {
            std::cerr << "[A] " << positive << " positive k-mers in the rows, " << rep.num_positive_kmers << " in the report; " << hitless << " reads without a hit" << std::endl;
            ok = false;
        }

        /* [B] */
        std::vector<sshash_read_sum> solid;
        dict.streaming_sums(b.bases.data(), b.offsets.data(), b.size(), values, 500, solid);
        ok = ok && same(solid, truth(values, 500), "[B] at_least = 500");
        const std::vector<uint32_t> all_ones(n, 0xFFFFFFFFu);
        std::vector<sshash_read_sum> wide;
        dict.streaming_sums(b.bases.data(), b.offsets.data(), b.size(), all_ones, 0, wide);
        ok = ok && same(wide, truth(all_ones, 0), "[B] values of 0xFFFFFFFF");
        uint64_t widest = 0;
        for (sshash_read_sum const& row : wide) widest = std::max(widest, row.sum);
        if ((widest >> 32) == 0) {
            std::cerr << "[B] no sum of more than 32 bits" << std::endl;
            ok = false;
        }

        /* [C] */
        std::vector<uint64_t> prefix(n + 1, 0);
        for (uint64_t i = 0; i < n; ++i) prefix[i + 1] = prefix[i] + values[i];
        std::vector<uint64_t> run_offsets;
        std::vector<sshash_streaming_run> runs;
        dict.streaming_runs(b.bases.data(), b.offsets.data(), b.size(), run_offsets, runs);
        std::vector<sshash_read_sum> from_runs(b.size(), sshash_read_sum{0, 0});
        uint64_t forward_runs = 0, backward_runs = 0;
        for (uint64_t r = 0; r < b.size(); ++r)
            for (uint64_t i = run_offsets[r]; i < run_offsets[r + 1]; ++i) {
                const uint64_t count = runs[i].num_kmers & ~SSHASH_RUN_BACKWARD;
                const bool backward = (runs[i].num_kmers & SSHASH_RUN_BACKWARD) != 0;
                (backward ? backward_runs : forward_runs) += 1;
                const uint64_t lo = backward ? runs[i].kmer_id + 1 - count : runs[i].kmer_id;
                from_runs[r].sum += prefix[lo + count] - prefix[lo];
                from_runs[r].positive_kmers += count;
            }
        ok = ok && same(sums, from_runs, "[C] the runs over a prefix sum");
        if (forward_runs < 50 || backward_runs < 50) {
            std::cerr << "the reads exercise too little: " << forward_runs << " forward runs, " << backward_runs << " backward" << std::endl;
            ok = false;
        }

        /* [D] */
        const std::string path = (std::filesystem::temp_directory_path() / ("check_sums_" + std::to_string(k) + (cfg.canonical ? "c" : "r") + ".fa")).string();
        {
            std::ofstream f(path);
            for (uint64_t r = 0; r < in_file; ++r) f << ">" << r << "\n" << b.read(r) << "\n";
        }
        std::vector<sshash_read_sum> from_file;
        bool in_order = true;
        const streaming_query_report file_rep = dict.streaming_sums_from_file(path, false, values, 0, [&](uint64_t first_read, sshash_read_sum const* part, uint64_t count) {
            in_order = in_order && first_read == from_file.size();
            from_file.insert(from_file.end(), part, part + count);
            return 0;
        });
        ok = ok && same(from_file, std::vector<sshash_read_sum>(want.begin(), want.begin() + in_file), "[D] the rows of the file");
        if (!in_order || file_rep.num_positive_kmers != rep.num_positive_kmers || file_rep.num_kmers != rep.num_kmers) {
            std::cerr << "[D] the file's batches came out of order, or its report differs" << std::endl;
            ok = false;
        }
        uint64_t calls = 0;
        bool stopped = false;
        try {
            dict.streaming_sums_from_file(path, false, values, 0, [&](uint64_t, sshash_read_sum const*, uint64_t) { return ++calls, 7; });
        } catch (std::runtime_error const&) {  // (the facade's error type, and no other)
            stopped = true;
        }
        std::remove(path.c_str());
        if (!stopped || calls != 1) {
            std::cerr << "[D] a callback's non-zero return did not stop the query: " << calls << " calls" << std::endl;
            ok = false;
        }
        if (ok) std::cout << "EVERYTHING OK! " << positive << " positive k-mers in " << b.size() - hitless << " of " << b.size() << " reads, the widest sum " << widest << std::endl;
        return ok ? 0 : 1;
    } catch (std::exception const& e) {
        std::cerr << "error: " << e.what() << std::endl;
        return 1;
    }
}
