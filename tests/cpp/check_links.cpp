// check_links.cpp -- the dictionary as a graph over the C++ facade (include/sshash_amd.hpp), against the navigational queries it had before:
//   [A] string_links(0, num_strings): for every string, its records are the found neighbours of string_neighbours(s), in that order,
//       with the id, the string and the orientation string_neighbours gives; a full lookup of the neighbour k-mer (access(to_kmer_id))
//       and string_size say whether it is the first or the last k-mer of its string (flag bits 4 and 5)
//   [B] kmer_adjacency(0, num_kmers): on every 97th id the byte names the neighbours that kmer_neighbours(access(id)) finds
// Needs a GPU (the lookups run there). Usage: check_links <input.fa[.gz]> <k> <m> [--canonical]
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <string>
#include <vector>

#include "sshash_amd.hpp"

using namespace sshash_amd;

static bool check_string_links(dictionary const& dict) {
    std::cout << "checking string links against string_neighbours..." << std::endl;
    const uint64_t k = dict.k(), n = dict.num_strings();
    const auto [offsets, links] = dict.string_links(0, n);
    if (offsets.size() != n + 1 || offsets[0] != 0 || offsets[n] != links.size()) {
        std::cerr << "link_offsets: " << offsets.size() << " words, the last says " << offsets.back() << ", " << links.size() << " records" << std::endl;
        return false;
    }
    std::string kmer(k, 0);
    uint64_t end_to_end = 0;
    for (uint64_t s = 0; s < n; ++s) {
        const neighbourhood nb = dict.string_neighbours(s);
        uint64_t at = offsets[s];
        for (uint32_t which = 0; which < 8; ++which) {
            lookup_result const& r = which < 4 ? nb.forward[which] : nb.backward[which - 4];
            if (r.kmer_id == constants::invalid_uint64) continue;
            if (at >= offsets[s + 1]) {
                std::cerr << "string " << s << ": fewer records than found neighbours" << std::endl;
                return false;
            }
            sshash_string_link const& l = links[at++];
            dict.access(l.to_kmer_id, kmer.data());
            const lookup_result full = dict.lookup(kmer.c_str());
            const bool first = full.kmer_id_in_string == 0, last = full.kmer_id_in_string + 1 == dict.string_size(full.string_id);
            const uint32_t flags = which | (r.kmer_orientation < 0 ? 8u : 0u) | (first ? 16u : 0u) | (last ? 32u : 0u);
            if (l.from_string != s || l.to_string != r.string_id || l.to_kmer_id != r.kmer_id || full.kmer_id != r.kmer_id || full.string_id != r.string_id ||
                l.flags != flags || l.reserved != 0) {
                std::cerr << "string " << s << ", neighbour " << which << ": record (" << l.from_string << ", " << l.to_string << ", " << l.to_kmer_id << ", "
                          << l.flags << "), expected (" << s << ", " << r.string_id << ", " << r.kmer_id << ", " << flags << ")" << std::endl;
                return false;
            }
            const bool at_start = (flags & 4) != 0, rc = (flags & 8) != 0;
            end_to_end += at_start ? (rc ? first : last) : (rc ? last : first);
        }
        if (at != offsets[s + 1]) {
            std::cerr << "string " << s << ": more records than found neighbours" << std::endl;
            return false;
        }
    }
    std::cout << links.size() << " links of " << n << " strings, " << end_to_end << " of them end to end" << std::endl;
    std::cout << "EVERYTHING OK!" << std::endl;
    return true;
}

static bool check_kmer_adjacency(dictionary const& dict) {
    std::cout << "checking k-mer adjacency against kmer_neighbours..." << std::endl;
    const uint64_t k = dict.k(), n = dict.num_kmers();
    const std::vector<uint8_t> masks = dict.kmer_adjacency(0, n);
    if (masks.size() != n) return false;
    std::string kmer(k, 0);
    uint64_t checked = 0;
    for (uint64_t id = 0; id < n; id += 97, ++checked) {
        dict.access(id, kmer.data());
        const neighbourhood nb = dict.kmer_neighbours(kmer.c_str());
        uint32_t want = 0;
        for (uint32_t c = 0; c < 4; ++c) {
            want |= uint32_t(nb.forward[c].kmer_id != constants::invalid_uint64) << c;
            want |= uint32_t(nb.backward[c].kmer_id != constants::invalid_uint64) << (4 + c);
        }
        if (masks[id] != want) {
            std::cerr << "k-mer " << id << ": mask " << uint32_t(masks[id]) << ", kmer_neighbours says " << want << std::endl;
            return false;
        }
    }
    std::cout << checked << " of " << n << " k-mers" << std::endl;
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
    cfg.num_threads = 4;
    cfg.canonical = argc > 4 && std::strcmp(argv[4], "--canonical") == 0;
    try {
        dictionary dict;
        dict.build(argv[1], cfg);
        dict.to_device(0);
        if (!check_string_links(dict) || !check_kmer_adjacency(dict)) return 1;
    } catch (std::exception const& e) {
        std::cerr << "error: " << e.what() << std::endl;
        return 1;
    }
    return 0;
}
