// check_cover.cpp -- the streaming cover over the C++ facade (include/sshash_amd.hpp):
//   [A] the bitmap of streaming_cover is exactly the set of kmer_id values other than invalid_uint64 that streaming_lookup returns over
//       the same reads, word for word; no bit at or above num_kmers is set; its report is the batch's report of streaming_query_per_read;
//   [B] the bitmap is ORed into: a second batch into the bitmap of the first gives the union, bits set by the caller survive;
//   [C] the same bitmap out of the runs of streaming_runs (forward: [kmer_id, kmer_id + n), backward: (kmer_id - n, kmer_id]);
//   [D] cover_string_counts: per string the set bits among its ids, their sum the bitmap's popcount;
//   [E] streaming_cover_from_file over the second batch written as FASTA, into the bitmap of the first: the union of [B], the same report.
// Reads: those of check_runs.cpp (windows of the dictionary's own strings, either strand, with substitutions and N's; two windows glued
// together; random reads; reads shorter than k), a whole string, its reverse complement.
// Usage: check_cover <input.fa[.gz]> <k> <m> [--canonical]
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

/* the bitmap out of the per-k-mer ids of streaming_lookup */
static std::vector<uint64_t> cover_of_lookup(dictionary const& dict, batch const& b) {
    lookup_results per_kmer;
    dict.streaming_lookup(b.bases.data(), b.offsets.data(), b.size(), per_kmer);
    std::vector<uint64_t> cover(dict.cover_words(), 0);
    const uint64_t k = dict.k();
    for (uint64_t r = 0; r < b.size(); ++r) {
        const uint64_t lo = b.offsets[r], len = b.offsets[r + 1] - lo;
        for (uint64_t j = 0; j + k <= len; ++j) {
            const uint64_t id = per_kmer.kmer_id[lo + j];
            if (id != constants::invalid_uint64) cover[id >> 6] |= uint64_t(1) << (id & 63);
        }
    }
    return cover;
}

static bool same(std::vector<uint64_t> const& got, std::vector<uint64_t> const& want, char const* what) {
    if (got.size() != want.size()) {
        std::cerr << what << ": " << got.size() << " words, expected " << want.size() << std::endl;
        return false;
    }
    for (uint64_t w = 0; w < got.size(); ++w)
        if (got[w] != want[w]) {
            std::cerr << what << ": word " << w << " is " << std::hex << got[w] << ", expected " << want[w] << std::dec << std::endl;
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
        std::cout << "checking the streaming cover on " << one.size() + two.size() << " reads, " << one.bases.size() + two.bases.size() << " bases..." << std::endl;
        bool ok = dict.cover_words() == (dict.num_kmers() + 63) / 64;
        if (!ok) std::cerr << "cover_words() = " << dict.cover_words() << " for " << dict.num_kmers() << " k-mers" << std::endl;

        /* [A] */
        const std::vector<uint64_t> want_one = cover_of_lookup(dict, one), want_two = cover_of_lookup(dict, two);
        std::vector<uint64_t> cover;
        const streaming_query_report rep = dict.streaming_cover(one.bases.data(), one.offsets.data(), one.size(), cover);
        ok = ok && same(cover, want_one, "[A] the first batch");
        std::vector<streaming_query_report> rows;
        const streaming_query_report plain = dict.streaming_query_per_read(one.bases.data(), one.offsets.data(), one.size(), rows);
        if (rep.num_kmers != plain.num_kmers || rep.num_positive_kmers != plain.num_positive_kmers || rep.num_negative_kmers != plain.num_negative_kmers ||
            rep.num_invalid_kmers != plain.num_invalid_kmers || rep.num_searches != plain.num_searches || rep.num_extensions != plain.num_extensions) {
            std::cerr << "[A] the report differs from streaming_query_per_read's: " << rep.num_positive_kmers << " positive against " << plain.num_positive_kmers << std::endl;
            ok = false;
        }
        uint64_t set_bits = 0;
        for (uint64_t w : cover) set_bits += uint64_t(__builtin_popcountll(w));
        if (set_bits == 0 || set_bits >= dict.num_kmers() || set_bits > rep.num_positive_kmers) {
            std::cerr << "[A] " << set_bits << " bits set for " << rep.num_positive_kmers << " positive k-mers of " << dict.num_kmers() << std::endl;
            ok = false;
        }
        if (dict.num_kmers() % 64 && (cover.back() >> (dict.num_kmers() % 64))) {
            std::cerr << "[A] bits at or above num_kmers are set" << std::endl;
            ok = false;
        }

        /* [B] */
        std::vector<uint64_t> both = cover, want_both(cover.size());
        for (uint64_t w = 0; w < cover.size(); ++w) want_both[w] = want_one[w] | want_two[w];
        const streaming_query_report rep_two = dict.streaming_cover(two.bases.data(), two.offsets.data(), two.size(), both);
        ok = ok && same(both, want_both, "[B] the second batch into the bitmap of the first");
        std::vector<uint64_t> kept(cover.size(), 0), want_kept = want_two;
        for (uint64_t w = 0; w < kept.size(); w += 3) {
            const uint64_t mine = (uint64_t(0x8000000000000001) << (w % 7)) & (w + 1 == kept.size() && dict.num_kmers() % 64 ? (uint64_t(1) << (dict.num_kmers() % 64)) - 1 : ~uint64_t(0));
            kept[w] = mine;
            want_kept[w] |= mine;
        }
        dict.streaming_cover(two.bases.data(), two.offsets.data(), two.size(), kept);
        ok = ok && same(kept, want_kept, "[B] bits set before the call");

        /* [C] */
        std::vector<uint64_t> run_offsets, from_runs(cover.size(), 0);
        std::vector<sshash_streaming_run> runs;
        dict.streaming_runs(one.bases.data(), one.offsets.data(), one.size(), run_offsets, runs);
        uint64_t forward_runs = 0, backward_runs = 0;
        for (sshash_streaming_run const& run : runs) {
            const uint64_t count = run.num_kmers & ~SSHASH_RUN_BACKWARD;
            const bool backward = (run.num_kmers & SSHASH_RUN_BACKWARD) != 0;
            (backward ? backward_runs : forward_runs) += 1;
            const uint64_t lo = backward ? run.kmer_id + 1 - count : run.kmer_id;
            for (uint64_t id = lo; id < lo + count; ++id) from_runs[id >> 6] |= uint64_t(1) << (id & 63);
        }
        ok = ok && same(cover, from_runs, "[C] the bitmap of the runs");
        if (forward_runs < 50 || backward_runs < 50) {
            std::cerr << "the reads exercise too little: " << forward_runs << " forward runs, " << backward_runs << " backward" << std::endl;
            ok = false;
        }

        /* [D] */
        std::vector<uint64_t> counts, want_counts(dict.num_strings(), 0);
        const uint64_t total = dict.cover_string_counts(both, counts);
        uint64_t want_total = 0;
        for (uint64_t s = 0; s < dict.num_strings(); ++s) {
            const auto [begin, end] = dict.string_offsets(s);
            for (uint64_t id = begin - s * (k - 1); id < end - (s + 1) * (k - 1); ++id) want_counts[s] += (both[id >> 6] >> (id & 63)) & 1;
            want_total += want_counts[s];
        }
        ok = ok && same(counts, want_counts, "[D] counts per string (CPU)");
        if (total != want_total) {
            std::cerr << "[D] total " << total << ", expected " << want_total << std::endl;
            ok = false;
        }

        /* [E] */
        const std::string path = (std::filesystem::temp_directory_path() / ("check_cover_" + std::to_string(k) + (cfg.canonical ? "c" : "r") + ".fa")).string();
        {
            std::ofstream f(path);
            for (uint64_t r = 0; r < two.size(); ++r)
                if (two.offsets[r + 1] > two.offsets[r]) f << ">" << r << "\n" << two.bases.substr(two.offsets[r], two.offsets[r + 1] - two.offsets[r]) << "\n";
        }
        std::vector<uint64_t> from_file = cover;
        const streaming_query_report file_rep = dict.streaming_cover_from_file(path, false, from_file);
        std::remove(path.c_str());
        ok = ok && same(from_file, want_both, "[E] the file of the second batch into the bitmap of the first");
        if (file_rep.num_kmers != rep_two.num_kmers || file_rep.num_positive_kmers != rep_two.num_positive_kmers || file_rep.num_searches != rep_two.num_searches ||
            file_rep.num_extensions != rep_two.num_extensions || file_rep.num_positive_kmers == 0) {
            std::cerr << "[E] the file's report differs from the in-memory call's: " << file_rep.num_positive_kmers << " positive against " << rep_two.num_positive_kmers << std::endl;
            ok = false;
        }
        if (ok) std::cout << "EVERYTHING OK! " << set_bits << " of " << dict.num_kmers() << " k-mers covered by the first batch, " << want_total << " by both" << std::endl;
        return ok ? 0 : 1;
    } catch (std::exception const& e) {
        std::cerr << "error: " << e.what() << std::endl;
        return 1;
    }
}
