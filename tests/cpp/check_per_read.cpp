// check_per_read.cpp -- the per-read streaming query over the C++ facade (include/sshash_amd.hpp):
//   [A] the rows of streaming_query_per_read add up, column by column, to the report the same call returns, and that report is the
//       one streaming_lookup gives for the same reads;
//   [B] every row equals what streaming_lookup's per-k-mer results say about its read: a k-mer is invalid iff one of its characters is,
//       positive iff it has an id, an extension iff the k-mer before it was positive in the same string and the id moved by that
//       k-mer's orientation, else a search (reference include/streaming_query.hpp:59-65, 86-100);
//   [C] the same reads as a FASTQ file: the callback gets every record exactly once, in order, with the rows of [A] -- the records
//       shorter than k included --, and a callback that returns non-zero stops the query with an exception.
// Reads: windows of the dictionary's own strings (rebuilt through access()), either strand, with substitutions and N's; random reads;
// reads shorter than k.
// Usage: check_per_read <input.fa[.gz]> <k> <m> [--canonical]     (the FASTQ of [C] is written under $TMPDIR, /tmp without one)
#include <algorithm>
#include <cctype>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <random>
#include <string>
#include <vector>

#include "sshash_amd.hpp"

using namespace sshash_amd;

static bool same(streaming_query_report const& a, streaming_query_report const& b) {
    return a.num_kmers == b.num_kmers && a.num_positive_kmers == b.num_positive_kmers && a.num_negative_kmers == b.num_negative_kmers &&
           a.num_invalid_kmers == b.num_invalid_kmers && a.num_searches == b.num_searches && a.num_extensions == b.num_extensions;
}

static std::ostream& operator<<(std::ostream& o, streaming_query_report const& r) {
    return o << "{" << r.num_kmers << " k-mers, " << r.num_positive_kmers << " positive, " << r.num_negative_kmers << " negative, "
             << r.num_invalid_kmers << " invalid, " << r.num_searches << " searches, " << r.num_extensions << " extensions}";
}

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
        std::mt19937_64 rng(99);
        auto below = [&](uint64_t n) { return uint64_t(rng() % n); };
        std::vector<std::string> reads;
        const uint64_t strings = std::min<uint64_t>(dict.num_strings(), 300);
        for (uint64_t i = 0; i < strings; ++i) {
            const std::string s = string_of(dict, below(dict.num_strings()), 400);
            std::string r = s.substr(below(s.size() - k + 1), 60 + below(200));
            for (char& c : r) {
                const uint64_t u = below(1000);
                if (u < 10) c = "ACGT"[below(4)];
                else if (u < 18) c = 'N';
            }
            if (i % 2) r = reverse_complement(r);
            if (i % 5 == 0)
                for (char& c : r) c = char(std::tolower(c));
            reads.push_back(r);
            std::string junk(1 + below(150), 'A');
            for (char& c : junk) c = "ACGT"[below(4)];
            reads.push_back(junk);
            if (i % 7 == 0) reads.push_back(std::string(below(k), 'C'));
        }
        reads.push_back(string_of(dict, 0, 400));
        std::string bases;
        std::vector<uint64_t> offsets{0};
        for (auto const& r : reads) {
            bases += r;
            offsets.push_back(bases.size());
        }
        const uint64_t n = reads.size();

        std::cout << "checking the per-read streaming query on " << n << " reads, " << bases.size() << " bases..." << std::endl;
        std::vector<streaming_query_report> rows;
        const streaming_query_report total = dict.streaming_query_per_read(bases.data(), offsets.data(), n, rows);
        lookup_results per_kmer;
        const streaming_query_report by_lookup = dict.streaming_lookup(bases.data(), offsets.data(), n, per_kmer);
        bool ok = rows.size() == n;
        /* [A] */
        streaming_query_report sum;
        for (auto const& r : rows) {
            sum.num_kmers += r.num_kmers;
            sum.num_positive_kmers += r.num_positive_kmers;
            sum.num_negative_kmers += r.num_negative_kmers;
            sum.num_invalid_kmers += r.num_invalid_kmers;
            sum.num_searches += r.num_searches;
            sum.num_extensions += r.num_extensions;
        }
        if (!same(sum, total) || !same(total, by_lookup)) {
            std::cerr << "rows add up to " << sum << ", the call reports " << total << ", streaming_lookup " << by_lookup << std::endl;
            ok = false;
        }
        if (total.num_extensions == 0 || total.num_negative_kmers == 0 || total.num_invalid_kmers == 0) {
            std::cerr << "the reads exercise too little: " << total << std::endl;
            ok = false;
        }
        /* [B] */
        auto valid = [](char c) { return std::strchr("ACGTacgt", c) != nullptr && c != 0; };
        for (uint64_t r = 0; r < n && ok; ++r) {
            streaming_query_report want;
            const uint64_t lo = offsets[r], len = offsets[r + 1] - lo;
            bool before = false;  // the k-mer before this one was positive
            for (uint64_t j = 0; j + k <= len; ++j) {
                ++want.num_kmers;
                bool all_valid = true;
                for (uint64_t c = 0; c < k && all_valid; ++c) all_valid = valid(bases[lo + j + c]);
                const uint64_t p = lo + j;
                if (!all_valid) {
                    ++want.num_invalid_kmers;
                    before = false;
                } else if (per_kmer.kmer_id[p] == constants::invalid_uint64) {
                    ++want.num_negative_kmers;
                    before = false;
                } else {
                    ++want.num_positive_kmers;
                    const bool extension = before && per_kmer.string_id[p - 1] == per_kmer.string_id[p] &&
                                           per_kmer.kmer_id[p] == per_kmer.kmer_id[p - 1] + uint64_t(int64_t(per_kmer.kmer_orientation[p - 1]));
                    if (extension) ++want.num_extensions;
                    else ++want.num_searches;
                    before = true;
                }
            }
            if (!same(rows[r], want)) {
                std::cerr << "read " << r << " '" << reads[r] << "': row " << rows[r] << " but its k-mers say " << want << std::endl;
                ok = false;
            }
        }
        /* [C] */
        const std::string path = std::string(std::getenv("TMPDIR") ? std::getenv("TMPDIR") : "/tmp") + "/check_per_read." + std::to_string(uint64_t(rng())) + ".fastq";
        {
            std::ofstream f(path);
            for (uint64_t r = 0; r < n; ++r) f << "@" << r << "\n" << reads[r] << "\n+\n" << std::string(reads[r].size(), 'I') << "\n";
        }
        uint64_t expect = 0, calls = 0;
        bool file_ok = true;
        const streaming_query_report from_file = dict.streaming_query_from_file_per_read(path, false, [&](uint64_t first, streaming_query_report const* got, uint64_t count) {
            ++calls;
            if (first != expect || first + count > n) file_ok = false;
            for (uint64_t i = 0; i < count && file_ok; ++i) file_ok = same(got[i], rows[first + i]);
            expect = first + count;
            return 0;
        });
        if (!file_ok || expect != n || !same(from_file, total)) {
            std::cerr << "the file's rows differ from the in-memory call's (" << expect << " of " << n << " records seen, report " << from_file << ")" << std::endl;
            ok = false;
        }
        const streaming_query_report whole_file = dict.streaming_query_from_file(path, false);  // (the total alone, through the parallel FASTQ reader)
        if (!same(whole_file, total)) {
            std::cerr << "streaming_query_from_file reports " << whole_file << ", the in-memory call " << total << std::endl;
            ok = false;
        }
        bool stopped = false;
        uint64_t calls_after = 0;
        try {
            dict.streaming_query_from_file_per_read(path, false, [&](uint64_t, streaming_query_report const*, uint64_t) {
                ++calls_after;
                return 3;
            });
        } catch (std::runtime_error const&) { stopped = true; }
        std::remove(path.c_str());
        if (!stopped || calls_after != 1) {
            std::cerr << "a callback returning 3 did not stop the query (" << calls_after << " calls)" << std::endl;
            ok = false;
        }
        if (ok) std::cout << "EVERYTHING OK! " << total << std::endl;
        return ok ? 0 : 1;
    } catch (std::exception const& e) {
        std::cerr << "error: " << e.what() << std::endl;
        return 1;
    }
}
