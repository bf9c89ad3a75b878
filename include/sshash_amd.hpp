// sshash_amd.hpp -- header-only C++17 facade over the C ABI (sshash_amd.h), shaped like the
// reference's `sshash::dictionary` (reference include/dictionary.hpp:10-181) so that drivers and
// checkers written against the reference read the same: same method names, same argument
// meaning, results by value, errors as std::runtime_error (the reference's only error channel:
// include/util.hpp:191-195, src/query.cpp:128), "not found" == constants::invalid_uint64.
//
// Additions over the reference interface are the batched overloads (the GPU engine wants
// batches) and `to_device`. Everything else is a one-element batch. `streaming_query` below mirrors
// reference include/streaming_query.hpp (one k-mer per call, the reference's shape) and adds the batched
// lookup_read().
#pragma once

#include <algorithm>
#include <array>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "sshash_amd.h"

namespace sshash_amd {

namespace constants {  // reference include/constants.hpp:5,17-18
constexpr uint64_t invalid_uint64 = uint64_t(-1);
constexpr int forward_orientation = 1;
constexpr int backward_orientation = -1;
}  // namespace constants

struct lookup_result {  // reference include/util.hpp:38-62
    uint64_t kmer_id = constants::invalid_uint64;
    uint64_t kmer_id_in_string = constants::invalid_uint64;
    uint64_t kmer_offset = constants::invalid_uint64;
    int64_t kmer_orientation = constants::forward_orientation;
    uint64_t string_id = constants::invalid_uint64;
    uint64_t string_begin = constants::invalid_uint64;
    uint64_t string_end = constants::invalid_uint64;
    bool minimizer_found = true;
};

struct streaming_query_report {  // reference include/util.hpp:21-36
    uint64_t num_kmers = 0, num_positive_kmers = 0, num_negative_kmers = 0, num_invalid_kmers = 0, num_searches = 0,
             num_extensions = 0;
};

struct build_configuration {  // reference include/util.hpp:143-159
    uint64_t k = 31, m = 20, seed = 1, num_threads = 1;
    double lambda = 5.0;
    bool canonical = false, verbose = false;
};

/* the `Kmer` of the reference's typed overloads lookup(Kmer, bool) / is_member(Kmer, bool) (include/dictionary.hpp:42,76):
   a 2-bit packed k-mer, first base in the least-significant bits (include/kmer.hpp:80,194) -- one word for k <= 31,
   two for k <= 63 (the reference's uint64_t / __uint128_t kmer_t) */
struct uint_kmer_t {
    uint64_t bits[2] = {0, 0};
    uint_kmer_t() = default;
    uint_kmer_t(uint64_t lo) : bits{lo, 0} {}
    uint_kmer_t(unsigned __int128 v) : bits{uint64_t(v), uint64_t(v >> 64)} {}
};

/* reference include/util.hpp:76-80: the four forward and the four backward neighbours of a k-mer, indexed by the 2-bit
   code of the added character (alphabet order "ACTG", include/kmer.hpp:118) */
struct neighbourhood {
    std::array<lookup_result, 4> forward, backward;
};

/* struct-of-arrays batch result */
struct lookup_results {
    std::vector<uint64_t> kmer_id, kmer_id_in_string, kmer_offset, string_id, string_begin, string_end;
    std::vector<int8_t> kmer_orientation;
    std::vector<uint8_t> minimizer_found;
    size_t size() const { return kmer_id.size(); }
    lookup_result operator[](size_t i) const {
        lookup_result r;
        r.kmer_id = kmer_id[i];
        r.kmer_id_in_string = kmer_id_in_string[i];
        r.kmer_offset = kmer_offset[i];
        r.kmer_orientation = kmer_orientation[i];
        r.string_id = string_id[i];
        r.string_begin = string_begin[i];
        r.string_end = string_end[i];
        r.minimizer_found = minimizer_found[i] != 0;
        return r;
    }
};

class dictionary {
public:
    dictionary() = default;
    dictionary(dictionary const&) = delete;
    dictionary& operator=(dictionary const&) = delete;
    dictionary(dictionary&& o) noexcept : m_h(o.m_h), m_info(o.m_info) { o.m_h = nullptr; }
    ~dictionary() { sshash_free(m_h); }

    /* dictionary::build(input_filename, build_config) -- include/dictionary.hpp:28 */
    void build(std::string const& input_filename, build_configuration const& c) {
        sshash_build_config cfg;
        sshash_build_config_default(&cfg);
        cfg.k = uint32_t(c.k);
        cfg.m = uint32_t(c.m);
        cfg.seed = c.seed;
        cfg.canonical = c.canonical;
        cfg.num_threads = uint32_t(c.num_threads);
        cfg.lambda = c.lambda;
        cfg.verbose = c.verbose;
        reset();
        check(sshash_build_from_fasta(input_filename.c_str(), &cfg, &m_h));
        check(sshash_get_info(m_h, &m_info));
    }
    /* essentials::load(dict, filename) / essentials::save -- tools/common.hpp:19-22, tools/build.cpp:90-95 */
    void load(std::string const& index_filename) {
        reset();
        check(sshash_load(index_filename.c_str(), &m_h));
        check(sshash_get_info(m_h, &m_info));
    }
    void save(std::string const& index_filename) const { check(sshash_save(m_h, index_filename.c_str())); }

    /* no reference counterpart: make the dictionary resident in the HBM of `device` */
    void to_device(int device = 0) { check(sshash_to_device(m_h, device)); }

    uint64_t num_kmers() const { return m_info.num_kmers; }
    uint64_t num_strings() const { return m_info.num_strings; }
    uint64_t k() const { return m_info.k; }
    uint64_t m() const { return m_info.m; }
    bool canonical() const { return m_info.canonical != 0; }
    uint64_t num_bits() const { return m_info.num_bits; }

    /* Lookup queries -- include/dictionary.hpp:40-42 */
    lookup_result lookup(char const* string_kmer, bool check_reverse_complement = true) const {
        return lookup_batch(string_kmer, 1, check_reverse_complement)[0];
    }
    lookup_result lookup(uint_kmer_t uint_kmer, bool check_reverse_complement = true) const {
        return lookup_batch(uint_kmer.bits, 1, check_reverse_complement)[0];
    }
    lookup_result lookup_packed(uint64_t const* uint_kmer_words, bool check_reverse_complement = true) const {
        return lookup_batch(uint_kmer_words, 1, check_reverse_complement)[0];
    }
    /* batched: n k-mers of k chars back to back (no terminators) */
    lookup_results lookup_batch(char const* kmers, uint64_t n, bool check_reverse_complement = true) const {
        lookup_results r;
        sshash_results out = bind(r, n);
        check(sshash_lookup_ascii(m_h, kmers, n, check_reverse_complement, &out));
        return r;
    }
    /* batched: n packed k-mers, words_per_kmer words each */
    lookup_results lookup_batch(uint64_t const* kmers, uint64_t n, bool check_reverse_complement = true) const {
        lookup_results r;
        sshash_results out = bind(r, n);
        check(sshash_lookup_packed(m_h, kmers, n, check_reverse_complement, &out));
        return r;
    }
    std::vector<uint64_t> lookup_ids(uint64_t const* kmers, uint64_t n, bool check_reverse_complement = true) const {
        std::vector<uint64_t> ids(n);
        sshash_results out{};
        out.kmer_id = ids.data();
        check(sshash_lookup_packed(m_h, kmers, n, check_reverse_complement, &out));
        return ids;
    }

    /* Navigational query -- include/dictionary.hpp:59-61 (kmer_neighbours): ids of the forward neighbours
       suffix + A,C,T,G at [8*i .. 8*i+3] and of the backward neighbours A,C,T,G + prefix at [8*i+4 .. 8*i+7]
       (the reference's alphabet order "ACTG": index = 2-bit code of the character)
       of packed k-mer i; INVALID for a neighbour that is not in the dictionary. */
    std::vector<uint64_t> neighbours_ids(uint64_t const* kmers, uint64_t n, bool check_reverse_complement = true) const {
        std::vector<uint64_t> ids(8 * n);
        sshash_results out{};
        out.kmer_id = ids.data();
        check(sshash_neighbours_packed(m_h, kmers, n, check_reverse_complement, &out));
        return ids;
    }

    /* include/dictionary.hpp:48-62, src/dictionary.cpp:111-201: the reference's navigational queries with its own
       signatures -- forward neighbours = suffix + each character, backward = each character + prefix; the *_forward_ /
       *_backward_ variants leave the other half default-constructed (not found), as the reference does */
    neighbourhood kmer_neighbours(uint_kmer_t uint_kmer, bool check_reverse_complement = true) const {
        return neighbours_of(uint_kmer, check_reverse_complement, true, true);
    }
    neighbourhood kmer_neighbours(char const* string_kmer, bool check_reverse_complement = true) const {
        return neighbours_of(pack(string_kmer), check_reverse_complement, true, true);
    }
    neighbourhood kmer_forward_neighbours(uint_kmer_t uint_kmer, bool check_reverse_complement = true) const {
        return neighbours_of(uint_kmer, check_reverse_complement, true, false);
    }
    neighbourhood kmer_forward_neighbours(char const* string_kmer, bool check_reverse_complement = true) const {
        return neighbours_of(pack(string_kmer), check_reverse_complement, true, false);
    }
    neighbourhood kmer_backward_neighbours(uint_kmer_t uint_kmer, bool check_reverse_complement = true) const {
        return neighbours_of(uint_kmer, check_reverse_complement, false, true);
    }
    neighbourhood kmer_backward_neighbours(char const* string_kmer, bool check_reverse_complement = true) const {
        return neighbours_of(pack(string_kmer), check_reverse_complement, false, true);
    }
    neighbourhood string_neighbours(uint64_t string_id, bool check_reverse_complement = true) const {
        lookup_results r;
        sshash_results out = bind(r, 8);
        check(sshash_string_neighbours(m_h, &string_id, 1, check_reverse_complement, &out));
        neighbourhood n;
        for (int c = 0; c < 4; ++c) {
            n.forward[c] = r[c];
            n.backward[c] = r[4 + c];
        }
        return n;
    }

    /* Return the number of kmers in string -- include/dictionary.hpp:44-46 */
    uint64_t string_size(uint64_t string_id) const {
        uint64_t size = 0;
        check(sshash_string_size(m_h, &string_id, 1, &size));
        return size;
    }

    /* [begin, end) of a string in bases -- include/dictionary.hpp:105-108 */
    std::pair<uint64_t, uint64_t> string_offsets(uint64_t string_id) const {
        uint64_t begin = 0, end = 0;
        check(sshash_string_offsets(m_h, &string_id, 1, &begin, &end));
        return {begin, end};
    }

    /* Return the weight of the kmer given its id -- include/dictionary.hpp (weight), src/dictionary.cpp:96-100 */
    bool weighted() const { return m_info.weighted != 0; }
    uint64_t weight(uint64_t kmer_id) const {
        uint64_t w = 0;
        check(sshash_weight(m_h, &kmer_id, 1, &w));
        return w;
    }

    /* include/dictionary.hpp:62 (string_neighbours): same layout, forward neighbours of the string's last k-mer and
       backward neighbours of its first one */
    std::vector<uint64_t> string_neighbours_ids(uint64_t const* string_ids, uint64_t n, bool check_reverse_complement = true) const {
        std::vector<uint64_t> ids(8 * n);
        sshash_results out{};
        out.kmer_id = ids.data();
        check(sshash_string_neighbours(m_h, string_ids, n, check_reverse_complement, &out));
        return ids;
    }

    /* The dictionary as a graph (sshash_string_links, sshash_kmer_adjacency in sshash_amd.h): the links of the strings [begin, end) as
       CSR -- the records of string begin + i are second[first[i] .. first[i + 1]) -- by a counting call and the exact one; and which
       of its eight neighbours every k-mer of the ids [begin, end) has in the dictionary, a byte per k-mer. */
    std::pair<std::vector<uint64_t>, std::vector<sshash_string_link>> string_links(uint64_t begin, uint64_t end, bool check_reverse_complement = true) const {
        std::vector<uint64_t> offsets(end >= begin ? end - begin + 1 : 1);
        check(sshash_string_links(m_h, begin, end, check_reverse_complement, offsets.data(), nullptr, 0));
        std::vector<sshash_string_link> links(offsets.back());
        if (!links.empty()) check(sshash_string_links(m_h, begin, end, check_reverse_complement, offsets.data(), links.data(), links.size()));
        return {std::move(offsets), std::move(links)};
    }
    std::vector<uint8_t> kmer_adjacency(uint64_t begin, uint64_t end, bool check_reverse_complement = true) const {
        std::vector<uint8_t> masks(end >= begin ? end - begin : 0);
        check(sshash_kmer_adjacency(m_h, begin, end, check_reverse_complement, masks.empty() ? nullptr : masks.data()));
        return masks;
    }

    /* Membership queries -- include/dictionary.hpp:74-76 */
    bool is_member(char const* string_kmer, bool check_reverse_complement = true) const {
        uint8_t out = 0;
        check(sshash_is_member_ascii(m_h, string_kmer, 1, check_reverse_complement, &out));
        return out != 0;
    }
    bool is_member(uint_kmer_t uint_kmer, bool check_reverse_complement = true) const {
        uint8_t out = 0;
        check(sshash_is_member_packed(m_h, uint_kmer.bits, 1, check_reverse_complement, &out));
        return out != 0;
    }
    std::vector<uint8_t> is_member_batch(char const* kmers, uint64_t n, bool check_reverse_complement = true) const {
        std::vector<uint8_t> out(n);
        check(sshash_is_member_ascii(m_h, kmers, n, check_reverse_complement, out.data()));
        return out;
    }

    /* Return the string of the kmer whose id is kmer_id -- include/dictionary.hpp:68-69 */
    void access(uint64_t kmer_id, char* string_kmer) const { check(sshash_access(m_h, kmer_id, string_kmer)); }

    /* include/dictionary.hpp:81-82 */
    streaming_query_report streaming_query_from_file(std::string const& filename, bool multiline) const {
        return reported([&](sshash_streaming_report* s) { return sshash_streaming_query_from_file(m_h, filename.c_str(), multiline, s); });
    }

    /* The streaming query's report for every read on its own (sshash_streaming_query_per_read; no reference counterpart as a call:
       the reference's state is reset at every read, src/query.cpp:78-108, so it is what the reference would report for that read
       alone): rows[r] for read r = bases[read_offsets[r] .. read_offsets[r + 1]), six zeros for a read shorter than k. Returns the
       batch's report, the column sums of the rows. */
    streaming_query_report streaming_query_per_read(char const* bases, uint64_t const* read_offsets, uint64_t num_reads,
                                                    std::vector<streaming_query_report>& rows) const {
        std::vector<sshash_streaming_report> raw(num_reads);
        sshash_streaming_report s;
        check(sshash_streaming_query_per_read(m_h, bases, read_offsets, num_reads, raw.data(), &s));
        rows.resize(num_reads);
        for (uint64_t r = 0; r < num_reads; ++r) rows[r] = to_report(raw[r]);
        return to_report(s);
    }

    /* device buffers, asynchronous on hip_stream (sshash_streaming_query_per_read_device): d_rows gets num_reads rows of six
       uint64 (overwritten), d_report -- may be null -- six counters (accumulated into) */
    void streaming_query_per_read_device(int device, char const* d_bases, uint64_t const* d_read_offsets, uint64_t num_reads,
                                         uint64_t total_bases, sshash_streaming_report* d_rows, uint64_t* d_report, void* hip_stream) const {
        check(sshash_streaming_query_per_read_device(m_h, device, d_bases, d_read_offsets, num_reads, total_bases, d_rows, d_report, hip_stream));
    }

    /* WHERE the reads hit: the maximal runs of the streaming query (sshash_streaming_runs; the record and the rule are in
       include/sshash_amd.h). run_offsets gets num_reads + 1 entries, runs the records of read r at run_offsets[r] .. run_offsets[r + 1],
       in increasing read_pos. Two calls: the counting one sizes `runs`. Returns the batch's report. */
    streaming_query_report streaming_runs(char const* bases, uint64_t const* read_offsets, uint64_t num_reads,
                                          std::vector<uint64_t>& run_offsets, std::vector<sshash_streaming_run>& runs) const {
        run_offsets.assign(num_reads + 1, 0);
        sshash_streaming_report s;
        check(sshash_streaming_runs(m_h, bases, read_offsets, num_reads, run_offsets.data(), nullptr, 0, &s));
        runs.resize(run_offsets[num_reads]);
        if (!runs.empty()) check(sshash_streaming_runs(m_h, bases, read_offsets, num_reads, run_offsets.data(), runs.data(), runs.size(), &s));
        return to_report(s);
    }

    /* device buffers, asynchronous on hip_stream (sshash_streaming_runs_device): d_run_offsets gets num_reads + 1 uint64 (overwritten),
       d_runs the records below runs_capacity (null with capacity 0: the counting call), d_report -- may be null -- six counters
       (accumulated into) */
    void streaming_runs_device(int device, char const* d_bases, uint64_t const* d_read_offsets, uint64_t num_reads, uint64_t total_bases,
                               uint64_t* d_run_offsets, sshash_streaming_run* d_runs, uint64_t runs_capacity, uint64_t* d_report,
                               void* hip_stream) const {
        check(sshash_streaming_runs_device(m_h, device, d_bases, d_read_offsets, num_reads, total_bases, d_run_offsets, d_runs, runs_capacity, d_report, hip_stream));
    }
    /* a query file, the runs of every record, handed over in file order: fn(first_read, run_offsets, runs, n) for one batch after the
       other -- run_offsets has n + 1 words, [0] = 0, local to the batch; both arrays are valid during the call of fn only --; a non-zero
       return stops the query (std::runtime_error). Fn: int(uint64_t, uint64_t const*, sshash_streaming_run const*, uint64_t). */
    template <typename Fn>
    streaming_query_report streaming_runs_from_file(std::string const& filename, bool multiline, Fn&& fn) const {
        struct runs_callback {
            typename std::remove_reference<Fn>::type* fn;
            static int thunk(void* ctx, uint64_t first_read, uint64_t n, const uint64_t* run_offsets, const sshash_streaming_run* runs) {
                return int((*static_cast<runs_callback*>(ctx)->fn)(first_read, run_offsets, runs, n));
            }
        } cb{&fn};
        return reported([&](sshash_streaming_report* s) { return sshash_streaming_runs_from_file(m_h, filename.c_str(), multiline, runs_callback::thunk, &cb, s); });
    }

    /* WHICH k-mers of the dictionary the reads hold (sshash_streaming_cover; the bit layout is in include/sshash_amd.h): k-mer id i is
       bit i & 63 of cover[i >> 6]. `cover` is sized to cover_words() if it is not (new words zero) and ORed into. Returns the batch's
       report. */
    uint64_t cover_words() const {
        uint64_t words = 0;
        check(sshash_cover_words(m_h, &words));
        return words;
    }
    streaming_query_report streaming_cover(char const* bases, uint64_t const* read_offsets, uint64_t num_reads, std::vector<uint64_t>& cover) const {
        cover.resize(cover_words(), 0);
        return reported([&](sshash_streaming_report* s) { return sshash_streaming_cover(m_h, bases, read_offsets, num_reads, cover.data(), s); });
    }
    /* device buffers, asynchronous on hip_stream (sshash_streaming_cover_device): d_cover -- cover_words() uint64 -- is ORed into,
       d_report -- may be null -- six counters (accumulated into) */
    void streaming_cover_device(int device, char const* d_bases, uint64_t const* d_read_offsets, uint64_t num_reads, uint64_t total_bases,
                                uint64_t* d_cover, uint64_t* d_report, void* hip_stream) const {
        check(sshash_streaming_cover_device(m_h, device, d_bases, d_read_offsets, num_reads, total_bases, d_cover, d_report, hip_stream));
    }
    /* a query file into one bitmap (sshash_streaming_cover_from_file) */
    streaming_query_report streaming_cover_from_file(std::string const& filename, bool multiline, std::vector<uint64_t>& cover) const {
        cover.resize(cover_words(), 0);
        return reported([&](sshash_streaming_report* s) { return sshash_streaming_cover_from_file(m_h, filename.c_str(), multiline, cover.data(), s); });
    }
    /* covered k-mers per string and in all (sshash_cover_string_counts: CPU, no GPU needed; _device: device buffers, asynchronous) */
    uint64_t cover_string_counts(std::vector<uint64_t> const& cover, std::vector<uint64_t>& counts) const {
        if (cover.size() < cover_words()) throw std::invalid_argument("cover has fewer than cover_words() words");
        counts.assign(num_strings(), 0);
        uint64_t total = 0;
        std::vector<uint64_t> none(1);
        check(sshash_cover_string_counts(m_h, cover.empty() ? none.data() : cover.data(), counts.empty() ? none.data() : counts.data(), &total));
        return total;
    }
    void cover_string_counts_device(int device, uint64_t const* d_cover, uint64_t* d_counts, uint64_t* d_total, void* hip_stream) const {
        check(sshash_cover_string_counts_device(m_h, device, d_cover, d_counts, d_total, hip_stream));
    }

    /* HOW OFTEN the reads hold each k-mer of the dictionary (sshash_streaming_depth; the definitions are in include/sshash_amd.h): depth[i]
       grows by the occurrences of k-mer id i in the reads, either strand, modulo 2^32. `depth` is sized to num_kmers() if it is not (new
       words zero) and added into. Returns the batch's report. */
    streaming_query_report streaming_depth(char const* bases, uint64_t const* read_offsets, uint64_t num_reads, std::vector<uint32_t>& depth) const {
        depth.resize(num_kmers(), 0);
        return reported([&](sshash_streaming_report* s) { return sshash_streaming_depth(m_h, bases, read_offsets, num_reads, depth.data(), s); });
    }
    /* device buffers, asynchronous on hip_stream (sshash_streaming_depth_device): d_deltas -- num_kmers() uint32, a difference array -- is
       added into, d_report -- may be null -- six counters (accumulated into); depth_finish_device turns deltas into depths (d_depth may
       be d_deltas) */
    void streaming_depth_device(int device, char const* d_bases, uint64_t const* d_read_offsets, uint64_t num_reads, uint64_t total_bases,
                                uint32_t* d_deltas, uint64_t* d_report, void* hip_stream) const {
        check(sshash_streaming_depth_device(m_h, device, d_bases, d_read_offsets, num_reads, total_bases, d_deltas, d_report, hip_stream));
    }
    /* long reads cut into segments of `kmers_per_segment` k-mers for the run kernel (sshash_set_read_segments), opt-in: 0 = the default S,
       SSHASH_SEGMENTS_OFF = never, which is where a new dictionary stands; `device_calls`: the device entry points segment as well. Same results either way. */
    struct read_segments_setting {
        uint64_t kmers_per_segment;   // S, or SSHASH_SEGMENTS_OFF
        bool device_calls;
        uint64_t segmented_launches;  // launches of the run kernel over a segment table so far
    };
    void set_read_segments(uint64_t kmers_per_segment = 0, bool device_calls = false) {
        check(sshash_set_read_segments(m_h, kmers_per_segment, device_calls ? 1 : 0));
    }
    read_segments_setting read_segments() const {
        read_segments_setting r{};
        int device_calls = 0;
        check(sshash_get_read_segments(m_h, &r.kmers_per_segment, &device_calls, &r.segmented_launches));
        r.device_calls = device_calls != 0;
        return r;
    }
    void depth_finish_device(int device, uint32_t const* d_deltas, uint32_t* d_depth, void* hip_stream) const {
        check(sshash_depth_finish_device(m_h, device, d_deltas, d_depth, hip_stream));
    }
    /* a query file into one depth array (sshash_streaming_depth_from_file) */
    streaming_query_report streaming_depth_from_file(std::string const& filename, bool multiline, std::vector<uint32_t>& depth) const {
        depth.resize(num_kmers(), 0);
        return reported([&](sshash_streaming_report* s) { return sshash_streaming_depth_from_file(m_h, filename.c_str(), multiline, depth.data(), s); });
    }
    /* the sum of depth over every string's ids, and over all (sshash_depth_string_sums: CPU, no GPU needed; _device: device buffers,
       asynchronous); the mean depth of string s is sums[s] / string_size(s) */
    uint64_t depth_string_sums(std::vector<uint32_t> const& depth, std::vector<uint64_t>& sums) const {
        if (depth.size() < num_kmers()) throw std::invalid_argument("depth has fewer than num_kmers() words");
        sums.assign(num_strings(), 0);
        uint64_t total = 0;
        std::vector<uint32_t> no_depth(1);
        std::vector<uint64_t> none(1);
        check(sshash_depth_string_sums(m_h, depth.empty() ? no_depth.data() : depth.data(), sums.empty() ? none.data() : sums.data(), &total));
        return total;
    }
    void depth_string_sums_device(int device, uint32_t const* d_depth, uint64_t* d_sums, uint64_t* d_total, void* hip_stream) const {
        check(sshash_depth_string_sums_device(m_h, device, d_depth, d_sums, d_total, hip_stream));
    }

    /* SCORING reads against a value per k-mer (sshash_streaming_sums; the definitions are in include/sshash_amd.h): per read, the sum of
       values[id] over the read's positive k-mers -- at_least >= 1: the number of those with values[id] >= at_least -- and their number.
       `values`: num_kmers() words; `sums` is sized to num_reads and overwritten. Returns the batch's report. */
    streaming_query_report streaming_sums(char const* bases, uint64_t const* read_offsets, uint64_t num_reads, std::vector<uint32_t> const& values,
                                          uint32_t at_least, std::vector<sshash_read_sum>& sums) const {
        if (values.size() < num_kmers()) throw std::invalid_argument("values has fewer than num_kmers() words");
        sums.assign(num_reads, sshash_read_sum{0, 0});
        std::vector<uint32_t> no_values(1);
        return reported([&](sshash_streaming_report* s) {
            return sshash_streaming_sums(m_h, bases, read_offsets, num_reads, values.empty() ? no_values.data() : values.data(), at_least, sums.data(), s);
        });
    }
    /* device buffers, asynchronous on hip_stream: d_prefix (num_kmers() + 1 uint64) out of d_values (sshash_value_prefix_device), and the
       rows out of d_prefix (sshash_streaming_sums_device): d_sums -- num_reads rows -- is overwritten, d_report -- may be null -- six
       counters (accumulated into) */
    void value_prefix_device(int device, uint32_t const* d_values, uint32_t at_least, uint64_t* d_prefix, void* hip_stream) const {
        check(sshash_value_prefix_device(m_h, device, d_values, at_least, d_prefix, hip_stream));
    }
    void streaming_sums_device(int device, char const* d_bases, uint64_t const* d_read_offsets, uint64_t num_reads, uint64_t total_bases,
                               uint64_t const* d_prefix, sshash_read_sum* d_sums, uint64_t* d_report, void* hip_stream) const {
        check(sshash_streaming_sums_device(m_h, device, d_bases, d_read_offsets, num_reads, total_bases, d_prefix, d_sums, d_report, hip_stream));
    }
    /* a query file, one row per record, handed over in file order: fn(first_read, sums, n) for one batch after the other; a non-zero
       return stops the query (std::runtime_error). Fn: int(uint64_t, sshash_read_sum const*, uint64_t). */
    template <typename Fn>
    streaming_query_report streaming_sums_from_file(std::string const& filename, bool multiline, std::vector<uint32_t> const& values, uint32_t at_least,
                                                    Fn&& fn) const {
        if (values.size() < num_kmers()) throw std::invalid_argument("values has fewer than num_kmers() words");
        auto cb = callback_of<sshash_read_sum>(fn);
        std::vector<uint32_t> no_values(1);
        return reported([&](sshash_streaming_report* s) {
            return sshash_streaming_sums_from_file(m_h, filename.c_str(), multiline, values.empty() ? no_values.data() : values.data(), at_least, cb.thunk, &cb, s);
        });
    }

    /* CLASSES (sshash_streaming_classes; the definitions are in include/sshash_amd.h): per read, its positive k-mers by class of string.
       `labels`: num_strings() words, a label >= num_classes is no class; `rows` is sized to num_reads x num_classes, row-major, and
       overwritten. Returns the batch's report. */
    streaming_query_report streaming_classes(char const* bases, uint64_t const* read_offsets, uint64_t num_reads, std::vector<uint32_t> const& labels,
                                             uint32_t num_classes, std::vector<uint32_t>& rows) const {
        if (labels.size() < num_strings()) throw std::invalid_argument("labels has fewer than num_strings() words");
        rows.assign(num_reads * uint64_t(num_classes), 0u);
        std::vector<uint32_t> spare(1);
        return reported([&](sshash_streaming_report* s) {
            return sshash_streaming_classes(m_h, bases, read_offsets, num_reads, labels.empty() ? spare.data() : labels.data(), num_classes,
                                            rows.empty() ? spare.data() : rows.data(), s);
        });
    }
    /* device buffers, asynchronous on hip_stream: d_rows -- num_reads x num_classes uint32 -- is overwritten, d_labels -- num_strings()
       uint32 -- only read, d_report -- may be null -- six counters (accumulated into) */
    void streaming_classes_device(int device, char const* d_bases, uint64_t const* d_read_offsets, uint64_t num_reads, uint64_t total_bases,
                                  uint32_t const* d_labels, uint32_t num_classes, uint32_t* d_rows, uint64_t* d_report, void* hip_stream) const {
        check(sshash_streaming_classes_device(m_h, device, d_bases, d_read_offsets, num_reads, total_bases, d_labels, num_classes, d_rows, d_report, hip_stream));
    }
    /* a query file, one row per record, handed over in file order: fn(first_read, rows, n) for one batch after the other, rows n x
       num_classes words; a non-zero return stops the query (std::runtime_error). Fn: int(uint64_t, uint32_t const*, uint64_t). */
    template <typename Fn>
    streaming_query_report streaming_classes_from_file(std::string const& filename, bool multiline, std::vector<uint32_t> const& labels,
                                                       uint32_t num_classes, Fn&& fn) const {
        if (labels.size() < num_strings()) throw std::invalid_argument("labels has fewer than num_strings() words");
        auto cb = callback_of<uint32_t>(fn);
        std::vector<uint32_t> spare(1);
        return reported([&](sshash_streaming_report* s) {
            return sshash_streaming_classes_from_file(m_h, filename.c_str(), multiline, labels.empty() ? spare.data() : labels.data(), num_classes, cb.thunk, &cb, s);
        });
    }
    /* the finish of the rows (sshash_class_best, sshash_class_totals): on the host over host arrays, or device buffers, asynchronous */
    static std::vector<sshash_read_class> class_best(std::vector<uint32_t> const& rows, uint32_t num_classes) {
        if (num_classes == 0 || rows.size() % num_classes) throw std::invalid_argument("rows is not a whole number of rows");
        std::vector<sshash_read_class> best(rows.size() / num_classes);
        check(sshash_class_best(rows.data(), best.size(), num_classes, best.data()));
        return best;
    }
    static std::vector<uint64_t> class_totals(std::vector<uint32_t> const& rows, uint32_t num_classes) {
        if (num_classes == 0 || rows.size() % num_classes) throw std::invalid_argument("rows is not a whole number of rows");
        std::vector<uint64_t> totals(num_classes);
        check(sshash_class_totals(rows.data(), rows.size() / num_classes, num_classes, totals.data()));
        return totals;
    }
    void class_best_device(int device, uint32_t const* d_rows, uint64_t num_reads, uint32_t num_classes, sshash_read_class* d_best, void* hip_stream) const {
        check(sshash_class_best_device(m_h, device, d_rows, num_reads, num_classes, d_best, hip_stream));
    }
    void class_totals_device(int device, uint32_t const* d_rows, uint64_t num_reads, uint32_t num_classes, uint64_t* d_totals, void* hip_stream) const {
        check(sshash_class_totals_device(m_h, device, d_rows, num_reads, num_classes, d_totals, hip_stream));
    }

    /* ANCHORS (sshash_streaming_best_run; the definition is in include/sshash_amd.h): per read its longest run, among equals the first in
       read order; a read without a hit has a record of zeros (num_kmers == 0). `best` is sized to num_reads and overwritten. Never
       over segments; throws on a minimizer shard. Returns the batch's report. */
    streaming_query_report streaming_best_run(char const* bases, uint64_t const* read_offsets, uint64_t num_reads, std::vector<sshash_streaming_run>& best) const {
        best.assign(num_reads, sshash_streaming_run{});
        return reported([&](sshash_streaming_report* s) { return sshash_streaming_best_run(m_h, bases, read_offsets, num_reads, best.data(), s); });
    }
    /* device buffers, asynchronous on hip_stream: d_best -- num_reads records -- is overwritten, d_report -- may be null -- six counters
       (accumulated into) */
    void streaming_best_run_device(int device, char const* d_bases, uint64_t const* d_read_offsets, uint64_t num_reads, uint64_t total_bases,
                                   sshash_streaming_run* d_best, uint64_t* d_report, void* hip_stream) const {
        check(sshash_streaming_best_run_device(m_h, device, d_bases, d_read_offsets, num_reads, total_bases, d_best, d_report, hip_stream));
    }
    /* a query file, one record per record of the file, handed over in file order: fn(first_read, best, n) for one batch after the other;
       a non-zero return stops the query (std::runtime_error). Fn: int(uint64_t, sshash_streaming_run const*, uint64_t). */
    template <typename Fn>
    streaming_query_report streaming_best_run_from_file(std::string const& filename, bool multiline, Fn&& fn) const {
        auto cb = callback_of<sshash_streaming_run>(fn);
        return reported([&](sshash_streaming_report* s) { return sshash_streaming_best_run_from_file(m_h, filename.c_str(), multiline, cb.thunk, &cb, s); });
    }
    /* the finish over a complete CSR of run records (sshash_runs_best): on the host over host arrays, or device buffers, asynchronous */
    static std::vector<sshash_streaming_run> runs_best(std::vector<uint64_t> const& run_offsets, std::vector<sshash_streaming_run> const& runs) {
        if (run_offsets.empty() || run_offsets.back() > runs.size()) throw std::invalid_argument("run_offsets is no CSR over runs");
        std::vector<sshash_streaming_run> best(run_offsets.size() - 1);
        check(sshash_runs_best(run_offsets.data(), runs.data(), best.size(), best.data()));
        return best;
    }
    void runs_best_device(int device, uint64_t const* d_run_offsets, sshash_streaming_run const* d_runs, uint64_t num_reads, sshash_streaming_run* d_best,
                          void* hip_stream) const {
        check(sshash_runs_best_device(m_h, device, d_run_offsets, d_runs, num_reads, d_best, hip_stream));
    }

    /* a query file, one row per record, handed over in file order: fn(first_read, rows, n) for one batch after the other; a
       non-zero return stops the query (std::runtime_error). Fn: int(uint64_t, streaming_query_report const*, uint64_t). */
    template <typename Fn>
    streaming_query_report streaming_query_from_file_per_read(std::string const& filename, bool multiline, Fn&& fn) const {
        static_assert(sizeof(streaming_query_report) == sizeof(sshash_streaming_report), "the same six counters");
        auto converted = [&fn](uint64_t first_read, const sshash_streaming_report* rows, uint64_t n) {  // (the C rows as this header's type)
            std::vector<streaming_query_report> mine(n);
            for (uint64_t i = 0; i < n; ++i) mine[i] = to_report(rows[i]);
            return fn(first_read, static_cast<streaming_query_report const*>(mine.data()), n);
        };
        auto cb = callback_of<sshash_streaming_report>(converted);
        return reported([&](sshash_streaming_report* s) { return sshash_streaming_query_from_file_per_read(m_h, filename.c_str(), multiline, cb.thunk, &cb, s); });
    }

    /* streaming_query::lookup for every k-mer of every read, batched (sshash_streaming_lookup): `r` gets one entry per
       base of `bases` -- entry read_offsets[i] + j = the k-mer starting at base j of read i; places where no k-mer starts
       keep a default (not found) result. */
    streaming_query_report streaming_lookup(char const* bases, uint64_t const* read_offsets, uint64_t num_reads, lookup_results& r) const {
        const uint64_t total = num_reads ? read_offsets[num_reads] : 0;
        sshash_results out = bind(r, total);
        out.minimizer_found = nullptr;  // not part of what streaming results are compared on (include/util.hpp:107-141)
        std::fill(r.kmer_id.begin(), r.kmer_id.end(), constants::invalid_uint64);
        std::fill(r.kmer_id_in_string.begin(), r.kmer_id_in_string.end(), constants::invalid_uint64);
        std::fill(r.kmer_offset.begin(), r.kmer_offset.end(), constants::invalid_uint64);
        std::fill(r.string_id.begin(), r.string_id.end(), constants::invalid_uint64);
        std::fill(r.string_begin.begin(), r.string_begin.end(), constants::invalid_uint64);
        std::fill(r.string_end.begin(), r.string_end.end(), constants::invalid_uint64);
        std::fill(r.kmer_orientation.begin(), r.kmer_orientation.end(), int8_t(constants::forward_orientation));
        std::fill(r.minimizer_found.begin(), r.minimizer_found.end(), uint8_t(1));
        return reported([&](sshash_streaming_report* s) { return sshash_streaming_lookup(m_h, bases, read_offsets, num_reads, &out, s); });
    }

    /* dictionary::iterator -- include/dictionary.hpp:84-94: (kmer id, k-mer) pairs of an id range in id order. It decodes
       ITERATOR_BUFFER k-mers at a time into a buffer of its own (sshash_iterate_packed) and hands them out one by one. */
    static constexpr uint64_t ITERATOR_BUFFER = uint64_t(1) << 16;
    class iterator {
    public:
        bool has_next() const { return m_next != m_end; }
        /* (kmer-id, encoded kmer) */
        std::pair<uint64_t, uint_kmer_t> next() {
            if (m_pos == m_filled) refill();
            uint_kmer_t x;
            for (uint32_t q = 0; q < m_W; ++q) x.bits[q] = m_buf[m_pos * m_W + q];
            ++m_pos;
            return {m_next++, x};
        }

    private:
        friend class dictionary;
        iterator(sshash_dict const* h, uint32_t W, uint64_t begin, uint64_t end)
            : m_h(h), m_W(W), m_next(begin), m_end(end) {}
        void refill() {
            if (m_next == m_end) throw std::out_of_range("iterator: next() past the end of its range");
            const uint64_t n = std::min(ITERATOR_BUFFER, m_end - m_next);
            m_buf.resize(n * m_W);
            check(sshash_iterate_packed(m_h, m_next, m_next + n, m_buf.data()));
            m_pos = 0;
            m_filled = n;
        }
        sshash_dict const* m_h;
        uint32_t m_W;
        uint64_t m_next, m_end;  // id of the next k-mer handed out; one past the last
        std::vector<uint64_t> m_buf;
        uint64_t m_pos = 0, m_filled = 0;  // m_buf holds the k-mers of ids m_next - m_pos .. m_next - m_pos + m_filled
    };

    /* include/dictionary.hpp:96-104 */
    iterator begin() const { return at_kmer_id(0); }
    iterator at_kmer_id(uint64_t kmer_id) const {
        if (kmer_id > num_kmers()) throw std::out_of_range("at_kmer_id: kmer_id out of range");
        return iterator(m_h, words_per_kmer(), kmer_id, num_kmers());
    }
    /* include/dictionary.hpp:113-121 */
    iterator at_string_id(uint64_t string_id) const {
        auto [begin, end] = string_offsets(string_id);
        const uint64_t begin_kmer_id = begin - string_id * (k() - 1);
        return iterator(m_h, words_per_kmer(), begin_kmer_id, begin_kmer_id + (end - begin) - k() + 1);
    }

    /* no reference counterpart: the reference's `sshash check` (tools/sshash.cpp:20-36) on the replica of `device`, the
       counts of sshash_check_device: {k-mers, forward not found, forward with another id, reverse complement wrong,
       not is_member, smallest failing id or invalid_uint64, 0, 0} */
    std::array<uint64_t, 8> check(int device) const {
        std::array<uint64_t, 8> out{};
        check(sshash_check_device(m_h, device, out.data()));
        return out;
    }

    sshash_dict* handle() const { return m_h; }
    uint32_t words_per_kmer() const { return m_info.words_per_kmer; }

private:
    static streaming_query_report to_report(sshash_streaming_report const& s) {
        streaming_query_report r;
        r.num_kmers = s.num_kmers;
        r.num_positive_kmers = s.num_positive_kmers;
        r.num_negative_kmers = s.num_negative_kmers;
        r.num_invalid_kmers = s.num_invalid_kmers;
        r.num_searches = s.num_searches;
        r.num_extensions = s.num_extensions;
        return r;
    }
    static void check(sshash_status s) {
        if (s != SSHASH_OK) throw std::runtime_error(sshash_last_error());
    }
    /* a streaming call of the C ABI, `call(report)`: checked, its report by value */
    template <typename Call>
    static streaming_query_report reported(Call&& call) {
        sshash_streaming_report s;
        check(call(&s));
        return to_report(s);
    }
    /* any callable fn(first_read, rows, n) as the (function, ctx) pair of a sshash_*_fn with rows of Row: `thunk` is the function, the
       object itself the ctx; it points at `fn`, which outlives the call */
    template <typename Row, typename Fn>
    struct row_callback {
        Fn* fn;
        static int thunk(void* ctx, uint64_t first_read, uint64_t n, const Row* rows) {
            return int((*static_cast<row_callback*>(ctx)->fn)(first_read, rows, n));
        }
    };
    template <typename Row, typename Fn>
    static row_callback<Row, Fn> callback_of(Fn& fn) {
        return {&fn};
    }
    void reset() {
        sshash_free(m_h);
        m_h = nullptr;
    }
    /* util::string_to_uint_kmer (include/util.hpp:207-213): k characters, (c >> 1) & 3 each, no validation */
    uint_kmer_t pack(char const* string_kmer) const {
        uint_kmer_t x;
        for (uint64_t i = 0; i < m_info.k; ++i) x.bits[i >> 5] |= uint64_t((string_kmer[i] >> 1) & 3) << (2 * (i & 31));
        return x;
    }
    neighbourhood neighbours_of(uint_kmer_t x, bool check_reverse_complement, bool forward, bool backward) const {
        lookup_results r;
        sshash_results out = bind(r, 8);
        check(sshash_neighbours_packed(m_h, x.bits, 1, check_reverse_complement, &out));
        neighbourhood n;
        for (int c = 0; c < 4; ++c) {
            if (forward) n.forward[c] = r[c];
            if (backward) n.backward[c] = r[4 + c];
        }
        return n;
    }
    static sshash_results bind(lookup_results& r, uint64_t n) {
        r.kmer_id.resize(n);
        r.kmer_id_in_string.resize(n);
        r.kmer_offset.resize(n);
        r.string_id.resize(n);
        r.string_begin.resize(n);
        r.string_end.resize(n);
        r.kmer_orientation.resize(n);
        r.minimizer_found.resize(n);
        sshash_results out;
        out.kmer_id = r.kmer_id.data();
        out.kmer_id_in_string = r.kmer_id_in_string.data();
        out.kmer_offset = r.kmer_offset.data();
        out.string_id = r.string_id.data();
        out.string_begin = r.string_begin.data();
        out.string_end = r.string_end.data();
        out.kmer_orientation = r.kmer_orientation.data();
        out.minimizer_found = r.minimizer_found.data();
        return out;
    }
    sshash_dict* m_h = nullptr;
    sshash_info m_info{};
};

/* streaming_query<Dict, canonical> -- reference include/streaming_query.hpp:9-198: a stateful cursor over the k-mers of
   a read. lookup(kmer) takes a pointer to k characters, the k-mer following the previous call's; reset() starts a new
   read. Same counters, same error (canonical mismatch -> std::runtime_error, :40-45), non-owning pointer to the
   dictionary (:118). The reference asserts that what lookup returns equals the point lookup (:107): here it IS the
   point lookup, with the reference's bookkeeping around it -- a k-mer with an invalid character resets the state
   (:59-65); a positive k-mer is an extension when the previous one was positive in the same string and the id moved by
   the orientation carried along (:86-100), else a search (:144-197). One call = one device round trip: this class is
   the reference's shape; lookup_read() is the form meant for the GPU (one batched call per read). */
template <bool canonical>
struct streaming_query {
    explicit streaming_query(dictionary const* dict) : m_dict(dict), m_k(dict->k()) {
        if (canonical != dict->canonical())
            throw std::runtime_error(std::string("dict.canonical() = ") + (dict->canonical() ? "true" : "false") + " but required " +
                                     (canonical ? "true" : "false"));
        reset();
    }

    void reset() {
        m_res = lookup_result();
        m_positive = false;
    }

    lookup_result lookup(char const* kmer) {
        for (uint64_t i = 0; i != m_k; ++i) {
            if (!is_valid(kmer[i])) {
                m_num_invalid += 1;
                reset();
                return m_res;
            }
        }
        account(m_dict->lookup(kmer));
        return m_res;
    }

    /* every k-mer of `read` (reset() first, as src/query.cpp:78-108 does per read): one batched call */
    std::vector<lookup_result> lookup_read(char const* read, uint64_t length) {
        reset();
        std::vector<lookup_result> out;
        if (length < m_k) return out;
        const uint64_t offsets[2] = {0, length};
        lookup_results r;
        const streaming_query_report rep = m_dict->streaming_lookup(read, offsets, 1, r);
        m_num_searches += rep.num_searches;
        m_num_extensions += rep.num_extensions;
        m_num_negative += rep.num_negative_kmers;
        m_num_invalid += rep.num_invalid_kmers;
        out.reserve(length - m_k + 1);
        for (uint64_t i = 0; i + m_k <= length; ++i) out.push_back(r[i]);
        return out;
    }

    uint64_t num_searches() const { return m_num_searches; }
    uint64_t num_extensions() const { return m_num_extensions; }
    uint64_t num_positive_lookups() const { return num_searches() + num_extensions(); }
    uint64_t num_negative_lookups() const { return m_num_negative; }
    uint64_t num_invalid_lookups() const { return m_num_invalid; }

private:
    static bool is_valid(char c) {  // include/kmer.hpp:209-219,253-255
        switch (c) {
            case 'A': case 'C': case 'G': case 'T': case 'a': case 'c': case 'g': case 't': return true;
            default: return false;
        }
    }
    void account(lookup_result const& now) {
        if (now.kmer_id == constants::invalid_uint64) {
            m_num_negative += 1;
            m_res = now;
            m_positive = false;
            return;
        }
        const bool extension = m_positive && now.string_id == m_res.string_id &&
                               now.kmer_id == m_res.kmer_id + uint64_t(m_res.kmer_orientation);
        const int64_t carried = m_res.kmer_orientation;
        m_res = now;
        if (extension) {
            m_num_extensions += 1;
            m_res.kmer_orientation = carried;  // :94-95
        } else {
            m_num_searches += 1;
        }
        m_positive = true;
    }

    dictionary const* m_dict;
    uint64_t m_k;
    lookup_result m_res;
    bool m_positive = false;
    uint64_t m_num_searches = 0, m_num_extensions = 0, m_num_invalid = 0, m_num_negative = 0;
};

}  // namespace sshash_amd
