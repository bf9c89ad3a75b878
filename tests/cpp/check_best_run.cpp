// check_best_run.cpp -- the streaming anchors (per read, its longest run) over the C++ facade (include/sshash_amd.hpp):
//   [A] record r of streaming_best_run is, byte for byte, the argmax over the records of read r of streaming_runs on the same reads -- the
//       largest num_kmers & 0x7FFFFFFF, among equals the first --, restated here; a read without a run has 32 zero bytes; the report is
//       streaming_query_per_read's, and a read's best run is no longer than its positive k-mers;
//   [B] runs_best (host) over that CSR gives the same records, and over a CSR made by hand: a tie, a tie between the strands, empty ranges;
//   [C] streaming_best_run_from_file over the reads written as FASTA: the same records in file order; a callback's non-zero return stops
//       the query.
// Reads: those of check_classes.cpp (windows of the dictionary's own strings, either strand, with substitutions and N's; two windows glued
// together -- runs in two strings --; random reads; reads shorter than k; an empty read), a whole string and a reverse complement.
// Usage: check_best_run <input.fa[.gz]> <k> <m> [--canonical]
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

static uint32_t length_of(sshash_streaming_run const& run) { return run.num_kmers & ~SSHASH_RUN_BACKWARD; }

/* the rule of include/sshash_amd.h, restated: the longest, among equals the first; zero bytes for an empty range */
static std::vector<sshash_streaming_run> argmax(std::vector<uint64_t> const& run_offsets, std::vector<sshash_streaming_run> const& runs) {
    std::vector<sshash_streaming_run> best(run_offsets.size() - 1);
    for (uint64_t r = 0; r + 1 < run_offsets.size(); ++r) {
        std::memset(&best[r], 0, sizeof(best[r]));
        for (uint64_t i = run_offsets[r]; i < run_offsets[r + 1]; ++i)
            if (length_of(runs[i]) > length_of(best[r])) best[r] = runs[i];
    }
    return best;
}

static bool same(std::vector<sshash_streaming_run> const& got, std::vector<sshash_streaming_run> const& want, char const* what) {
    if (got.size() != want.size()) {
        std::cerr << what << ": " << got.size() << " records, expected " << want.size() << std::endl;
        return false;
    }
    for (uint64_t r = 0; r < got.size(); ++r)
        if (std::memcmp(&got[r], &want[r], sizeof(sshash_streaming_run)) != 0) {
            std::cerr << what << ": read " << r << " is {" << got[r].kmer_id << ", " << got[r].string_id << ", " << got[r].kmer_id_in_string << ", " << got[r].read_pos
                      << ", " << got[r].num_kmers << "}, expected {" << want[r].kmer_id << ", " << want[r].string_id << ", " << want[r].kmer_id_in_string << ", "
                      << want[r].read_pos << ", " << want[r].num_kmers << "}" << std::endl;
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
        std::mt19937_64 rng(11);
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
        const uint64_t in_file = b.size();  // (the file form has a record per record of the file: the empty read comes behind the reads that go into it)
        b.add("");
        std::cout << "checking the streaming anchors on " << b.size() << " reads, " << b.bases.size() << " bases, " << strings << " strings..." << std::endl;
        bool ok = true;

        /* [A] */
        std::vector<uint64_t> run_offsets;
        std::vector<sshash_streaming_run> runs;
        dict.streaming_runs(b.bases.data(), b.offsets.data(), b.size(), run_offsets, runs);
        const std::vector<sshash_streaming_run> want = argmax(run_offsets, runs);
        std::vector<sshash_streaming_run> best(3);  // (the wrong size, and not zeros: the call sizes and overwrites it)
        std::memset(best.data(), 0x77, best.size() * sizeof(sshash_streaming_run));
        const streaming_query_report rep = dict.streaming_best_run(b.bases.data(), b.offsets.data(), b.size(), best);
        ok = ok && same(best, want, "[A] the best runs");
        std::vector<streaming_query_report> per_read;
        const streaming_query_report plain = dict.streaming_query_per_read(b.bases.data(), b.offsets.data(), b.size(), per_read);
        if (rep.num_kmers != plain.num_kmers || rep.num_positive_kmers != plain.num_positive_kmers || rep.num_negative_kmers != plain.num_negative_kmers ||
            rep.num_invalid_kmers != plain.num_invalid_kmers || rep.num_searches != plain.num_searches || rep.num_extensions != plain.num_extensions) {
            std::cerr << "[A] the report differs from streaming_query_per_read's: " << rep.num_positive_kmers << " positive against " << plain.num_positive_kmers << std::endl;
            ok = false;
        }
        uint64_t hitless = 0, backward = 0, not_first = 0, several = 0;
        for (uint64_t r = 0; r < b.size() && ok; ++r) {
            const uint64_t n_runs = run_offsets[r + 1] - run_offsets[r];
            hitless += n_runs == 0;
            several += n_runs >= 2;
            backward += (best[r].num_kmers & SSHASH_RUN_BACKWARD) != 0;
            not_first += n_runs && std::memcmp(&best[r], &runs[run_offsets[r]], sizeof(sshash_streaming_run)) != 0;
            if ((n_runs == 0) != (best[r].num_kmers == 0) || length_of(best[r]) > per_read[r].num_positive_kmers) {
                std::cerr << "[A] read " << r << ": " << n_runs << " runs, " << per_read[r].num_positive_kmers << " positive k-mers, a best run of " << length_of(best[r]) << std::endl;
                ok = false;
            }
        }
        if (ok && (hitless == 0 || backward == 0 || not_first == 0 || several == 0)) {
            std::cerr << "[A] the reads do not hold what is to be told apart: " << hitless << " without a run, " << backward << " backward, " << not_first
                      << " whose longest run is not their first, " << several << " with several runs" << std::endl;
            ok = false;
        }

        /* [B] */
        ok = ok && same(dictionary::runs_best(run_offsets, runs), want, "[B] runs_best over the runs of the reads");
        auto run = [](uint64_t id, uint32_t pos, uint32_t n) { return sshash_streaming_run{id, 1, id, pos, n}; };
        const std::vector<sshash_streaming_run> made{run(10, 0, 4), run(20, 9, 4), run(30, 20, 3),                   // a tie: the first
                                                     run(40, 0, 2), run(50, 5, 6 | SSHASH_RUN_BACKWARD), run(60, 30, 6),  // a tie between the strands: the first
                                                     run(70, 3, 1)};
        const std::vector<uint64_t> made_offsets{0, 0, 3, 3, 6, 7, 7};
        const std::vector<sshash_streaming_run> made_best = dictionary::runs_best(made_offsets, made);
        ok = ok && same(made_best, argmax(made_offsets, made), "[B] runs_best over records made by hand");
        if (ok && (made_best[0].num_kmers != 0 || made_best[1].kmer_id != 10 || made_best[2].num_kmers != 0 || made_best[3].kmer_id != 50 || made_best[4].kmer_id != 70 ||
                   made_best[5].num_kmers != 0)) {
            std::cerr << "[B] the records made by hand" << std::endl;
            ok = false;
        }

        /* [C] */
        const std::string path = (std::filesystem::temp_directory_path() / ("check_best_run_" + std::to_string(k) + (cfg.canonical ? "c" : "r") + ".fa")).string();
        {
            std::ofstream f(path);
            for (uint64_t r = 0; r < in_file; ++r) f << ">" << r << "\n" << b.read(r) << "\n";
        }
        std::vector<sshash_streaming_run> from_file;
        bool in_order = true;
        const streaming_query_report file_rep = dict.streaming_best_run_from_file(path, false, [&](uint64_t first_read, sshash_streaming_run const* part, uint64_t count) {
            in_order = in_order && first_read == from_file.size();
            from_file.insert(from_file.end(), part, part + count);
            return 0;
        });
        ok = ok && same(from_file, std::vector<sshash_streaming_run>(want.begin(), want.begin() + in_file), "[C] the records of the file");
        if (!in_order || file_rep.num_positive_kmers != rep.num_positive_kmers || file_rep.num_kmers != rep.num_kmers) {
            std::cerr << "[C] the file's batches came out of order, or its report differs" << std::endl;
            ok = false;
        }
        uint64_t calls = 0;
        bool stopped = false;
        try {
            dict.streaming_best_run_from_file(path, false, [&](uint64_t, sshash_streaming_run const*, uint64_t) { return ++calls, 7; });
        } catch (std::runtime_error const&) {  // (the facade's error type, and no other)
            stopped = true;
        }
        std::remove(path.c_str());
        if (!stopped || calls != 1) {
            std::cerr << "[C] a callback's non-zero return did not stop the query: " << calls << " calls" << std::endl;
            ok = false;
        }
        if (ok) std::cout << "EVERYTHING OK! " << b.size() - hitless << " of " << b.size() << " reads have a best run, " << backward << " of them backward, " << not_first
                          << " not the read's first run" << std::endl;
        return ok ? 0 : 1;
    } catch (std::exception const& e) {
        std::cerr << "error: " << e.what() << std::endl;
        return 1;
    }
}
