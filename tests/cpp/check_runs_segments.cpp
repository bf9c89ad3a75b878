// check_runs_segments.cpp -- the streaming runs over segments and from a file, over the C++ facade (include/sshash_amd.hpp):
//   [A] streaming_runs with the reads cut into segments of S k-mers (set_read_segments) gives run_offsets and records that are byte
//       for byte those of the same call with the segments off, for S = 1, 7 and 64, and the dictionary counts segmented launches;
//   [B] streaming_runs_from_file over the same reads written as a FASTA gives, batch after batch and stitched, the same again; every
//       record of the file has an entry; a callback that returns non-zero stops the call with an exception.
// Reads: windows of the dictionary's own strings, either strand, with substitutions and N's; a read that follows one string for
// several hundred k-mers; reads shorter than k; the last read a long one.
// Usage: check_runs_segments <input.fa[.gz]> <k> <m> [--canonical]
#include <algorithm>
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

static bool same(std::vector<uint64_t> const& a_offsets, std::vector<sshash_streaming_run> const& a, std::vector<uint64_t> const& b_offsets,
                 std::vector<sshash_streaming_run> const& b) {
    return a_offsets == b_offsets && a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(sshash_streaming_run)) == 0);
}

static bool operator==(streaming_query_report const& a, streaming_query_report const& b) {
    return a.num_kmers == b.num_kmers && a.num_positive_kmers == b.num_positive_kmers && a.num_negative_kmers == b.num_negative_kmers &&
           a.num_invalid_kmers == b.num_invalid_kmers && a.num_searches == b.num_searches && a.num_extensions == b.num_extensions;
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
        std::mt19937_64 rng(13);
        auto below = [&](uint64_t n) { return uint64_t(rng() % n); };
        uint64_t longest = 0;  // the string with the most k-mers among the first few hundred
        for (uint64_t s = 0, best = 0; s < std::min<uint64_t>(dict.num_strings(), 400); ++s) {
            const auto [begin, end] = dict.string_offsets(s);
            if (end - begin > best) best = end - begin, longest = s;
        }
        const std::string long_string = string_of(dict, longest, 1500);
        auto window = [&]() {
            const std::string s = string_of(dict, below(dict.num_strings()), 400);
            std::string r = s.substr(below(s.size() - k + 1), 60 + below(200));
            return below(2) ? reverse_complement(r) : r;
        };
        std::vector<std::string> reads;
        for (uint64_t i = 0; i < 120; ++i) {
            std::string r = window();
            for (char& c : r) {
                const uint64_t u = below(1000);
                if (u < 10) c = "ACGT"[below(4)];
                else if (u < 15) c = 'N';
            }
            reads.push_back(r);
            reads.push_back(window() + window());
            if (i % 7 == 0) reads.push_back(std::string(1 + below(k - 1), 'C'));
        }
        reads.push_back(reverse_complement(long_string));
        reads.push_back(long_string + window() + long_string);  // the last read is a long one
        std::string bases;
        std::vector<uint64_t> offsets{0};
        for (auto const& r : reads) {
            bases += r;
            offsets.push_back(bases.size());
        }
        const uint64_t n = reads.size();
        std::cout << "checking the streaming runs over segments on " << n << " reads, " << bases.size() << " bases..." << std::endl;

        /* [A] */
        std::vector<uint64_t> want_offsets, got_offsets;
        std::vector<sshash_streaming_run> want, got;
        dict.set_read_segments(SSHASH_SEGMENTS_OFF, false);
        const streaming_query_report want_report = dict.streaming_runs(bases.data(), offsets.data(), n, want_offsets, want);
        bool ok = want_offsets.size() == n + 1 && want_offsets[n] == want.size() && !want.empty();
        uint64_t long_runs = 0;
        for (auto const& run : want) long_runs += (run.num_kmers & ~SSHASH_RUN_BACKWARD) > 4 * 64;
        if (long_runs < 2) {
            std::cerr << "the reads exercise too little: " << long_runs << " runs of more than 256 k-mers" << std::endl;
            ok = false;
        }
        if (dict.read_segments().segmented_launches != 0) {
            std::cerr << "a segmented launch with the segments off" << std::endl;
            ok = false;
        }
        for (uint64_t S : {uint64_t(1), uint64_t(7), uint64_t(64)}) {
            const uint64_t before = dict.read_segments().segmented_launches;
            dict.set_read_segments(S, false);
            const streaming_query_report r = dict.streaming_runs(bases.data(), offsets.data(), n, got_offsets, got);
            if (!same(want_offsets, want, got_offsets, got) || !(r == want_report)) {
                std::cerr << "S = " << S << ": the runs over segments differ from the runs of the whole reads (" << got.size() << " records, " << want.size() << " wanted)" << std::endl;
                ok = false;
            }
            if (dict.read_segments().segmented_launches <= before) {
                std::cerr << "S = " << S << ": no segmented launch was counted" << std::endl;
                ok = false;
            }
        }
        /* [B] */
        const std::string path = (std::filesystem::temp_directory_path() / ("check_runs_segments." + std::to_string(uint64_t(rng())) + ".fa")).string();
        {
            std::ofstream out(path);
            for (uint64_t r = 0; r < n; ++r) out << ">" << r << "\n" << reads[r] << "\n";
        }
        for (uint64_t S : {uint64_t(SSHASH_SEGMENTS_OFF), uint64_t(7)}) {
            dict.set_read_segments(S, false);
            std::vector<uint64_t> file_offsets{0};
            std::vector<sshash_streaming_run> file_runs;
            uint64_t next_read = 0;
            bool in_order = true;
            const streaming_query_report r = dict.streaming_runs_from_file(path, false, [&](uint64_t first_read, uint64_t const* ro, sshash_streaming_run const* runs, uint64_t count) {
                in_order = in_order && first_read == next_read && ro[0] == 0;
                next_read += count;
                const uint64_t base = file_offsets.back();
                for (uint64_t i = 1; i <= count; ++i) file_offsets.push_back(base + ro[i]);
                file_runs.insert(file_runs.end(), runs, runs + ro[count]);
                return 0;
            });
            if (!in_order || next_read != n || !same(want_offsets, want, file_offsets, file_runs) || !(r == want_report)) {
                std::cerr << "the file call" << (S == 7 ? " over segments" : "") << " differs from streaming_runs: " << next_read << " records of the file, " << file_runs.size() << " runs" << std::endl;
                ok = false;
            }
        }
        uint64_t calls = 0;
        try {
            dict.streaming_runs_from_file(path, false, [&](uint64_t, uint64_t const*, sshash_streaming_run const*, uint64_t) { return int(++calls + 4); });
            std::cerr << "a callback that returned 5 did not stop the file call" << std::endl;
            ok = false;
        } catch (std::runtime_error const& e) {
            if (calls != 1 || std::string(e.what()).find("5") == std::string::npos) {
                std::cerr << "the stopped file call: " << calls << " calls, '" << e.what() << "'" << std::endl;
                ok = false;
            }
        }
        std::remove(path.c_str());
        if (ok) std::cout << "EVERYTHING OK! " << want.size() << " runs, " << long_runs << " of them above 256 k-mers, in " << n << " reads" << std::endl;
        return ok ? 0 : 1;
    } catch (std::exception const& e) {
        std::cerr << "error: " << e.what() << std::endl;
        return 1;
    }
}
