// check_runs.cpp -- the streaming runs over the C++ facade (include/sshash_amd.hpp):
//   [A] per read, the number of runs is num_searches and the k-mers in its runs are num_positive_kmers of its row of
//       streaming_query_per_read; the report of the call is that call's report;
//   [B] the runs of a read lie in increasing read_pos, do not overlap and stay inside the read;
//   [C] expanded -- k-mer j of a run starts at base read_pos + j and has kmer_id +/- j, kmer_id_in_string +/- j, the run's string and
//       orientation --, the runs give exactly the per-k-mer results of streaming_lookup (the orientation: of the positive k-mers): every
//       positive k-mer lies in one run, no other
//       k-mer in any; and a run starts exactly where streaming_lookup's results do not continue the k-mer before (the rule of the header).
// Reads: windows of the dictionary's own strings (rebuilt through access()), either strand, with substitutions and N's; two windows of
// different strings glued together; random reads; reads shorter than k.
// Usage: check_runs <input.fa[.gz]> <k> <m> [--canonical]
#include <algorithm>
#include <cctype>
#include <cstdio>
#include <cstdlib>
#include <cstring>
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
        std::vector<std::string> reads;
        for (uint64_t i = 0; i < 300; ++i) {
            std::string r = window();
            for (char& c : r) {
                const uint64_t u = below(1000);
                if (u < 10) c = "ACGT"[below(4)];
                else if (u < 15) c = 'N';
            }
            if (i % 5 == 0)
                for (char& c : r) c = char(std::tolower(c));
            reads.push_back(r);
            reads.push_back(window() + window());
            std::string junk(1 + below(150), 'A');
            for (char& c : junk) c = "ACGT"[below(4)];
            reads.push_back(junk);
            if (i % 7 == 0) reads.push_back(std::string(below(k), 'C'));
        }
        reads.push_back("");
        reads.push_back(string_of(dict, 0, 400));
        std::string bases;
        std::vector<uint64_t> offsets{0};
        for (auto const& r : reads) {
            bases += r;
            offsets.push_back(bases.size());
        }
        const uint64_t n = reads.size();
        std::cout << "checking the streaming runs on " << n << " reads, " << bases.size() << " bases..." << std::endl;

        std::vector<uint64_t> run_offsets;
        std::vector<sshash_streaming_run> runs;
        const streaming_query_report total = dict.streaming_runs(bases.data(), offsets.data(), n, run_offsets, runs);
        std::vector<streaming_query_report> rows;
        const streaming_query_report by_rows = dict.streaming_query_per_read(bases.data(), offsets.data(), n, rows);
        lookup_results per_kmer;
        dict.streaming_lookup(bases.data(), offsets.data(), n, per_kmer);
        bool ok = run_offsets.size() == n + 1 && run_offsets[0] == 0 && run_offsets[n] == runs.size();
        if (!ok) std::cerr << "run_offsets: " << run_offsets.size() << " entries, the last " << (run_offsets.empty() ? 0 : run_offsets.back()) << ", " << runs.size() << " records" << std::endl;
        if (total.num_searches != by_rows.num_searches || total.num_positive_kmers != by_rows.num_positive_kmers || total.num_kmers != by_rows.num_kmers ||
            total.num_searches != runs.size()) {
            std::cerr << "the reports differ: " << total.num_searches << " searches, " << runs.size() << " runs, per read " << by_rows.num_searches << std::endl;
            ok = false;
        }
        uint64_t backward_runs = 0, forward_runs = 0, reads_with_two = 0;
        for (uint64_t r = 0; r < n && ok; ++r) {
            const uint64_t lo = offsets[r], len = offsets[r + 1] - lo, kmers = len >= k ? len - k + 1 : 0;
            /* [A] */
            uint64_t in_runs = 0;
            for (uint64_t i = run_offsets[r]; i < run_offsets[r + 1]; ++i) in_runs += runs[i].num_kmers & ~SSHASH_RUN_BACKWARD;
            if (run_offsets[r + 1] - run_offsets[r] != rows[r].num_searches || in_runs != rows[r].num_positive_kmers) {
                std::cerr << "read " << r << ": " << run_offsets[r + 1] - run_offsets[r] << " runs of " << in_runs << " k-mers, its row says "
                          << rows[r].num_searches << " searches, " << rows[r].num_positive_kmers << " positive" << std::endl;
                ok = false;
                break;
            }
            reads_with_two += run_offsets[r + 1] - run_offsets[r] >= 2;
            /* [B], [C] */
            std::vector<uint64_t> id(kmers, constants::invalid_uint64), sid(kmers, constants::invalid_uint64), inside(kmers, constants::invalid_uint64);
            std::vector<int8_t> ori(kmers, 1);
            std::vector<uint8_t> head(kmers, 0);
            uint64_t next_free = 0;
            for (uint64_t i = run_offsets[r]; i < run_offsets[r + 1] && ok; ++i) {
                sshash_streaming_run const& run = runs[i];
                const uint64_t count = run.num_kmers & ~SSHASH_RUN_BACKWARD;
                const bool backward = (run.num_kmers & SSHASH_RUN_BACKWARD) != 0;
                (backward ? backward_runs : forward_runs) += 1;
                if (count == 0 || run.read_pos < next_free || run.read_pos + count > kmers) {
                    std::cerr << "read " << r << ": run " << i << " of " << count << " k-mers at base " << run.read_pos << " (the read has " << kmers << ", the run before ends at " << next_free << ")" << std::endl;
                    ok = false;
                    break;
                }
                next_free = run.read_pos + count;
                head[run.read_pos] = 1;
                for (uint64_t j = 0; j < count; ++j) {
                    id[run.read_pos + j] = backward ? run.kmer_id - j : run.kmer_id + j;
                    inside[run.read_pos + j] = backward ? run.kmer_id_in_string - j : run.kmer_id_in_string + j;
                    sid[run.read_pos + j] = run.string_id;
                    ori[run.read_pos + j] = backward ? -1 : 1;
                }
            }
            for (uint64_t j = 0; j < kmers && ok; ++j) {
                const uint64_t p = lo + j;
                /* (a negative k-mer's orientation is the strand of the lookup's last probe -- no run carries it) */
                const bool positive = per_kmer.kmer_id[p] != constants::invalid_uint64;
                if (id[j] != per_kmer.kmer_id[p] || sid[j] != per_kmer.string_id[p] || inside[j] != per_kmer.kmer_id_in_string[p] ||
                    (positive && ori[j] != per_kmer.kmer_orientation[p])) {
                    std::cerr << "read " << r << " '" << reads[r] << "', k-mer " << j << ": the runs say id " << id[j] << " string " << sid[j] << " at " << inside[j] << " orientation " << int(ori[j])
                              << ", streaming_lookup " << per_kmer.kmer_id[p] << " " << per_kmer.string_id[p] << " " << per_kmer.kmer_id_in_string[p] << " " << int(per_kmer.kmer_orientation[p]) << std::endl;
                    ok = false;
                    break;
                }
                if (per_kmer.kmer_id[p] == constants::invalid_uint64) continue;
                const bool continues = j > 0 && per_kmer.kmer_id[p - 1] != constants::invalid_uint64 && per_kmer.string_id[p - 1] == per_kmer.string_id[p] &&
                                       per_kmer.kmer_id[p] == per_kmer.kmer_id[p - 1] + uint64_t(int64_t(per_kmer.kmer_orientation[p - 1]));
                if (continues == (head[j] != 0)) {
                    std::cerr << "read " << r << ", k-mer " << j << ": " << (continues ? "continues the run before it but starts a record" : "starts a run but has no record") << std::endl;
                    ok = false;
                }
            }
        }
        if (ok && (forward_runs < 50 || backward_runs < 50 || reads_with_two < 100)) {
            std::cerr << "the reads exercise too little: " << forward_runs << " forward runs, " << backward_runs << " backward, " << reads_with_two << " reads with two runs and more" << std::endl;
            ok = false;
        }
        if (ok) std::cout << "EVERYTHING OK! " << runs.size() << " runs (" << forward_runs << " forward, " << backward_runs << " backward) in " << n << " reads" << std::endl;
        return ok ? 0 : 1;
    } catch (std::exception const& e) {
        std::cerr << "error: " << e.what() << std::endl;
        return 1;
    }
}
