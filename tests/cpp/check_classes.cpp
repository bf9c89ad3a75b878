// check_classes.cpp -- the streaming classes over the C++ facade (include/sshash_amd.hpp):
//   [A] word c of row r of streaming_classes is the number of places of read r where streaming_lookup over the same reads returns a k-mer
//       of a string s with labels[s] == c; the report is streaming_query_per_read's; with every string in a class a row sums to
//       num_positive_kmers of the read's row there;
//   [B] labels at or above num_classes are no class: the masked truth, rows that sum to less; num_classes of 1, 64, 65;
//   [C] the same rows out of the runs of streaming_runs: a run of n k-mers in string s is worth n in column labels[s];
//   [D] class_best and class_totals (host) against a restatement here: the tie goes to the smaller class, a row of zeros has no class;
//   [E] streaming_classes_from_file over the reads written as FASTA: the same rows in file order; a callback's non-zero return stops the query.
// Reads: those of check_sums.cpp (windows of the dictionary's own strings, either strand, with substitutions and N's; two windows glued
// together -- hits in two strings --; random reads; reads shorter than k; an empty read), a whole string and a reverse complement.
// Usage: check_classes <input.fa[.gz]> <k> <m> [--canonical]
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

static bool same(std::vector<uint32_t> const& got, std::vector<uint32_t> const& want, uint32_t C, char const* what) {
    if (got.size() != want.size()) {
        std::cerr << what << ": " << got.size() << " words, expected " << want.size() << std::endl;
        return false;
    }
    for (uint64_t i = 0; i < got.size(); ++i)
        if (got[i] != want[i]) {
            std::cerr << what << ": read " << i / C << ", class " << i % C << " is " << got[i] << ", expected " << want[i] << std::endl;
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
        const uint64_t k = dict.k(), strings = dict.num_strings();
        std::mt19937_64 rng(7);
        auto below = [&](uint64_t m) { return uint64_t(rng() % m); };
        auto window = [&]() {
            const std::string s = string_of(dict, below(strings), 400);
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
        b.add(reverse_complement(string_of(dict, strings - 1, 400)));
        const uint64_t in_file = b.size();  // (the file form has a row per record: the empty read comes behind the reads that go into the file)
        b.add("");
        std::cout << "checking the streaming classes on " << b.size() << " reads, " << b.bases.size() << " bases, " << strings << " strings..." << std::endl;
        bool ok = true;

        lookup_results per_kmer;
        dict.streaming_lookup(b.bases.data(), b.offsets.data(), b.size(), per_kmer);
        auto truth = [&](std::vector<uint32_t> const& labels, uint32_t C) {
            std::vector<uint32_t> want(b.size() * C, 0u);
            for (uint64_t r = 0; r < b.size(); ++r) {
                const uint64_t lo = b.offsets[r], len = b.offsets[r + 1] - lo;
                for (uint64_t j = 0; j + k <= len; ++j) {
                    if (per_kmer.kmer_id[lo + j] == constants::invalid_uint64) continue;
                    const uint32_t label = labels[per_kmer.string_id[lo + j]];
                    if (label < C) want[r * C + label] += 1;
                }
            }
            return want;
        };

        /* [A] */
        const uint32_t C = 5;
        std::vector<uint32_t> labels(strings);
        for (uint64_t s = 0; s < strings; ++s) labels[s] = uint32_t(s % C);
        const std::vector<uint32_t> want = truth(labels, C);
        std::vector<uint32_t> rows;
        const streaming_query_report rep = dict.streaming_classes(b.bases.data(), b.offsets.data(), b.size(), labels, C, rows);
        ok = ok && same(rows, want, C, "[A] the rows");
        std::vector<streaming_query_report> per_read;
        const streaming_query_report plain = dict.streaming_query_per_read(b.bases.data(), b.offsets.data(), b.size(), per_read);
        if (rep.num_kmers != plain.num_kmers || rep.num_positive_kmers != plain.num_positive_kmers || rep.num_negative_kmers != plain.num_negative_kmers ||
            rep.num_invalid_kmers != plain.num_invalid_kmers || rep.num_searches != plain.num_searches || rep.num_extensions != plain.num_extensions) {
            std::cerr << "[A] the report differs from streaming_query_per_read's: " << rep.num_positive_kmers << " positive against " << plain.num_positive_kmers << std::endl;
            ok = false;
        }
        uint64_t positive = 0, hitless = 0, in_two_classes = 0;
        for (uint64_t r = 0; r < b.size() && ok; ++r) {
            uint64_t sum = 0, columns = 0;
            for (uint32_t c = 0; c < C; ++c) {
                sum += rows[r * C + c];
                columns += rows[r * C + c] != 0;
            }
            positive += sum;
            hitless += sum == 0;
            in_two_classes += columns >= 2;
            if (sum != per_read[r].num_positive_kmers) {
                std::cerr << "[A] read " << r << ": its row sums to " << sum << " against " << per_read[r].num_positive_kmers << " positive k-mers of its row" << std::endl;
                ok = false;
            }
        }
        if (ok && (positive != rep.num_positive_kmers || positive == 0 || hitless == 0 || in_two_classes == 0)) {
            std::cerr << "[A] " << positive << " k-mers in the rows, " << rep.num_positive_kmers << " in the report; " << hitless << " reads without a hit, "
                      << in_two_classes << " with hits in two classes" << std::endl;
            ok = false;
        }

        /* [B] */
        for (uint32_t classes : {1u, 64u, 65u}) {
            std::vector<uint32_t> masked(strings);
            for (uint64_t s = 0; s < strings; ++s) masked[s] = below(3) ? uint32_t(below(classes)) : classes + uint32_t(below(2)) * 0x7FFFFFF0u;
            std::vector<uint32_t> got;
            dict.streaming_classes(b.bases.data(), b.offsets.data(), b.size(), masked, classes, got);
            ok = ok && same(got, truth(masked, classes), classes, "[B] labels that are no class");
            uint64_t counted = 0;
            for (uint32_t v : got) counted += v;
            if (counted == 0 || counted >= positive) {
                std::cerr << "[B] " << classes << " classes: " << counted << " k-mers counted of " << positive << std::endl;
                ok = false;
            }
        }

        /* [C] */
        std::vector<uint64_t> run_offsets;
        std::vector<sshash_streaming_run> runs;
        dict.streaming_runs(b.bases.data(), b.offsets.data(), b.size(), run_offsets, runs);
        std::vector<uint32_t> from_runs(b.size() * C, 0u);
        for (uint64_t r = 0; r < b.size(); ++r)
            for (uint64_t i = run_offsets[r]; i < run_offsets[r + 1]; ++i)
                from_runs[r * C + labels[runs[i].string_id]] += uint32_t(runs[i].num_kmers & ~SSHASH_RUN_BACKWARD);
        ok = ok && same(rows, from_runs, C, "[C] the runs, each worth its length in its string's class");

        /* [D] */
        std::vector<uint32_t> made = rows;
        made.insert(made.end(), {7, 7, 0, 7, 1, /* a tie */ 0, 0, 0, 0, 0, /* zeros */ 0, 0, 0, 4, 0, /* one column */ 0xFFFFFFFFu, 1, 0xFFFFFFFFu, 0, 0});
        const std::vector<sshash_read_class> best = dictionary::class_best(made, C);
        const std::vector<uint64_t> totals = dictionary::class_totals(made, C);
        std::vector<uint64_t> want_totals(C, 0);
        for (uint64_t r = 0; r < best.size() && ok; ++r) {
            sshash_read_class w{SSHASH_NO_CLASS, 0, 0, 0};
            for (uint32_t c = 0; c < C; ++c) {
                const uint32_t v = made[r * C + c];
                want_totals[c] += v;
                w.total += v;
                if (v > w.best) w.best = v, w.best_class = c;
            }
            for (uint32_t c = 0; c < C; ++c)
                if (c != w.best_class) w.second = std::max(w.second, made[r * C + c]);
            if (best[r].best_class != w.best_class || best[r].best != w.best || best[r].second != w.second || best[r].total != w.total) {
                std::cerr << "[D] row " << r << ": {" << best[r].best_class << ", " << best[r].best << ", " << best[r].second << ", " << best[r].total << "}, expected {"
                          << w.best_class << ", " << w.best << ", " << w.second << ", " << w.total << "}" << std::endl;
                ok = false;
            }
        }
        const uint64_t m0 = b.size();
        if (ok && (best[m0].best_class != 0 || best[m0].second != 7 || best[m0 + 1].best_class != SSHASH_NO_CLASS || best[m0 + 2].second != 0 ||
                   best[m0 + 3].best_class != 0 || best[m0 + 3].second != 0xFFFFFFFFu || best[m0 + 3].total != 0xFFFFFFFFu || totals != want_totals)) {
            std::cerr << "[D] the rows made by hand, or the totals" << std::endl;
            ok = false;
        }

        /* [E] */
        const std::string path = (std::filesystem::temp_directory_path() / ("check_classes_" + std::to_string(k) + (cfg.canonical ? "c" : "r") + ".fa")).string();
        {
            std::ofstream f(path);
            for (uint64_t r = 0; r < in_file; ++r) f << ">" << r << "\n" << b.read(r) << "\n";
        }
        std::vector<uint32_t> from_file;
        bool in_order = true;
        const streaming_query_report file_rep = dict.streaming_classes_from_file(path, false, labels, C, [&](uint64_t first_read, uint32_t const* part, uint64_t count) {
            in_order = in_order && first_read * C == from_file.size();
            from_file.insert(from_file.end(), part, part + count * C);
            return 0;
        });
        ok = ok && same(from_file, std::vector<uint32_t>(want.begin(), want.begin() + in_file * C), C, "[E] the rows of the file");
        if (!in_order || file_rep.num_positive_kmers != rep.num_positive_kmers || file_rep.num_kmers != rep.num_kmers) {
            std::cerr << "[E] the file's batches came out of order, or its report differs" << std::endl;
            ok = false;
        }
        uint64_t calls = 0;
        bool stopped = false;
        try {
            dict.streaming_classes_from_file(path, false, labels, C, [&](uint64_t, uint32_t const*, uint64_t) { return ++calls, 7; });
        } catch (std::runtime_error const&) {  // (the facade's error type, and no other)
            stopped = true;
        }
        std::remove(path.c_str());
        if (!stopped || calls != 1) {
            std::cerr << "[E] a callback's non-zero return did not stop the query: " << calls << " calls" << std::endl;
            ok = false;
        }
        if (ok) std::cout << "EVERYTHING OK! " << positive << " positive k-mers in " << b.size() - hitless << " of " << b.size() << " reads, " << in_two_classes
                          << " reads with hits in two classes" << std::endl;
        return ok ? 0 : 1;
    } catch (std::exception const& e) {
        std::cerr << "error: " << e.what() << std::endl;
        return 1;
    }
}
