// check_segments.cpp -- long reads cut into segments over the C++ facade (include/sshash_amd.hpp): dictionary::set_read_segments(7)
// must give, for one long read among short ones, the report and every row that SSHASH_SEGMENTS_OFF gives, and read_segments() must
// say that the run kernel was launched over a segment table for it -- and was not before.
// The long read: several of the dictionary's own strings (rebuilt through access()) back to back, every second one reverse
// complemented, with a substitution and an N; the short reads: windows of strings, random reads, reads shorter than k.
// Usage: check_segments <input.fa[.gz]> <k> <m> [--canonical]
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
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
        std::mt19937_64 rng(7);
        auto below = [&](uint64_t n) { return uint64_t(rng() % n); };
        std::string long_read;
        for (uint64_t i = 0; long_read.size() < 20000; ++i) {
            const std::string s = string_of(dict, below(dict.num_strings()), 1500);
            long_read += i % 2 ? reverse_complement(s) : s;
        }
        long_read[long_read.size() / 3] = long_read[long_read.size() / 3] == 'A' ? 'C' : 'A';
        long_read[long_read.size() / 2] = 'N';
        std::vector<std::string> reads;
        uint64_t at_long = 0;  // where the long read stands in the batch
        for (uint64_t i = 0; i < 50; ++i) {
            const std::string s = string_of(dict, below(dict.num_strings()), 400);
            reads.push_back(s.substr(below(s.size() - k + 1), 60 + below(200)));
            std::string junk(1 + below(150), 'A');
            for (char& c : junk) c = "ACGT"[below(4)];
            reads.push_back(junk);
            if (i == 25) {
                at_long = reads.size();
                reads.push_back(long_read);
            }
        }
        reads.push_back("");
        std::string bases;
        std::vector<uint64_t> offsets{0};
        for (auto const& r : reads) {
            bases += r;
            offsets.push_back(bases.size());
        }
        const uint64_t n = reads.size();
        std::cout << "checking segments on " << n << " reads, one of " << long_read.size() << " bases..." << std::endl;

        bool ok = true;
        auto setting = dict.read_segments();
        if (setting.kmers_per_segment != SSHASH_SEGMENTS_OFF || setting.device_calls || setting.segmented_launches != 0) {
            std::cerr << "a new dictionary's setting: S " << setting.kmers_per_segment << ", launches " << setting.segmented_launches << std::endl;
            ok = false;
        }
        dict.set_read_segments(SSHASH_SEGMENTS_OFF);
        std::vector<streaming_query_report> rows_off, rows_on;
        const streaming_query_report off = dict.streaming_query_per_read(bases.data(), offsets.data(), n, rows_off);
        if (dict.read_segments().segmented_launches != 0 || dict.read_segments().kmers_per_segment != SSHASH_SEGMENTS_OFF) {
            std::cerr << "SSHASH_SEGMENTS_OFF launched over segments" << std::endl;
            ok = false;
        }
        dict.set_read_segments(7);
        const streaming_query_report on = dict.streaming_query_per_read(bases.data(), offsets.data(), n, rows_on);
        setting = dict.read_segments();
        if (setting.kmers_per_segment != 7 || setting.segmented_launches == 0) {
            std::cerr << "S = 7: S reads back as " << setting.kmers_per_segment << ", " << setting.segmented_launches << " segmented launches" << std::endl;
            ok = false;
        }
        if (!same(on, off)) {
            std::cerr << "S = 7 reports " << on << ", OFF " << off << std::endl;
            ok = false;
        }
        if (rows_on.size() != n || rows_off.size() != n) ok = false;
        for (uint64_t r = 0; r < n && ok; ++r) {
            if (!same(rows_on[r], rows_off[r])) {
                std::cerr << "read " << r << " (" << reads[r].size() << " bases): S = 7 gives " << rows_on[r] << ", OFF " << rows_off[r] << std::endl;
                ok = false;
            }
        }
        if (ok && (rows_off[at_long].num_kmers != long_read.size() - k + 1 || rows_off[at_long].num_extensions < 1000 /* (at S = 7: more than a hundred seams inside runs) */ || rows_off[at_long].num_searches < 2 ||
                   rows_off[at_long].num_invalid_kmers != k)) {
            std::cerr << "the long read exercises too little: " << rows_off[at_long] << std::endl;
            ok = false;
        }
        bool refused = false;
        try {
            dict.set_read_segments((uint64_t(1) << 30) + 1);
        } catch (std::runtime_error const&) { refused = true; }
        if (!refused || dict.read_segments().kmers_per_segment != 7) {
            std::cerr << "2^30 + 1 k-mers a segment was not refused" << std::endl;
            ok = false;
        }
        if (ok) std::cout << "EVERYTHING OK! " << on << std::endl;
        return ok ? 0 : 1;
    } catch (std::exception const& e) {
        std::cerr << "error: " << e.what() << std::endl;
        return 1;
    }
}
