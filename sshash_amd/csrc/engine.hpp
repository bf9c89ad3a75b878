// engine.hpp -- host-side owner of the device-resident dictionary replicas and kernel launchers.
#pragma once

#include <atomic>
#include <functional>
#include <memory>
#include <mutex>
#include <shared_mutex>
#include <string>
#include <vector>

#include "device_layout.hpp"
#include "index.hpp"
#include "segments.hpp"

namespace sshash_amd {

struct device_replica;  // defined in engine.hip

enum class out_mode : int { ids = 0, full = 1, member = 2 };

/* the one collective step of the sharded lookup, supplied by the caller (sshash_exchange in include/sshash_amd.h) */
struct exchange_ops {
    void* ctx;
    int (*counts)(void* ctx, const uint64_t* send, uint64_t* recv);
    int (*data)(void* ctx, const void* send, const uint64_t* send_counts, void* recv, const uint64_t* recv_counts, uint32_t elem_bytes,
                void* hip_stream);
};

struct streaming_report {  // streaming_query_report, include/util.hpp:21-36
    uint64_t num_kmers = 0, num_positive_kmers = 0, num_negative_kmers = 0, num_invalid_kmers = 0,
             num_searches = 0, num_extensions = 0;
    /* the six counters as the device accumulates them (streaming_query_device: d_report), in this order */
    static streaming_report from_device(uint64_t const words[6]) { return {words[0], words[1], words[2], words[3], words[4], words[5]}; }
    streaming_report& operator+=(streaming_report const& o) {
        num_kmers += o.num_kmers;
        num_positive_kmers += o.num_positive_kmers;
        num_negative_kmers += o.num_negative_kmers;
        num_invalid_kmers += o.num_invalid_kmers;
        num_searches += o.num_searches;
        num_extensions += o.num_extensions;
        return *this;
    }
};

/* where the runs of a streaming call go (streaming.hip), device pointers: run_offsets -- n_reads + 1 words, CSR --, the records
   (sshash_streaming_run, include/sshash_amd.h) and how many of them there is room for. The sums form alone reads the two members
   behind them: the prefix sums of the values (num_kmers + 1 words) -- its rows, two words a read, are at `records` -- and, for reads cut
   into segments, the read of every entry of the segment table (null: an entry is a read). The classes form keeps its rows at `records`
   as well and `read_of` as the sums form; the struct is not grown for it (every instantiation of the run kernel takes it by value, and
   its size and offsets are what they were): the number of classes shares the word of `capacity` and the labels, one 32-bit word per
   string, the word of `values_prefix`. A sink is of one form from its making on -- class_sink (streaming.hip) makes the classes form's --,
   so only the member that was written is ever read. */
struct run_sink {
    uint64_t* run_offsets;
    void* records;
    union {
        uint64_t capacity;     // the records form: room for so many records
        uint64_t num_classes;  // the classes form: words in a row
    };
    union {
        uint64_t const* values_prefix;  // the sums form
        uint32_t const* labels;         // the classes form
    };
    uint64_t const* read_of;
    run_sink(uint64_t* offsets, void* recs, uint64_t room, uint64_t const* prefix = nullptr, uint64_t const* reads = nullptr)
        : run_offsets(offsets), records(recs), capacity(room), values_prefix(prefix), read_of(reads) {}
};
static_assert(sizeof(run_sink) == 40, "the run kernel takes the sink by value: its layout is part of every instantiation");

class engine;

/* One device array of `count` elements of T (never fewer than one is allocated) in the HBM of every resident replica, for the length of
   a host call or of a whole query file (streaming.hip). The constructor allocates on one replica after the other and hands every array
   and its size in bytes, with its device current, to `fill`; when anything throws, what was allocated is freed again. The caller's
   current device is restored. Throws no_device when no replica is resident. */
template <class T>
class replica_arrays {
public:
    using fill_fn = std::function<void(int device, T* array, uint64_t bytes)>;  // done with the array when it returns: the lanes' streams do not wait for the null stream
    replica_arrays(engine const& eng, uint64_t count, char const* none_here /* what on() throws with */, fill_fn const& fill);
    ~replica_arrays();
    replica_arrays(replica_arrays const&) = delete;
    replica_arrays& operator=(replica_arrays const&) = delete;
    T* on(int device) const;  // the array on `device` (device pointer)
protected:
    uint64_t m_count;
    std::vector<int> m_devices;
    std::vector<T*> m_arrays;
private:
    void free_all(int then_device);
    char const* m_none_here;
};
extern template class replica_arrays<uint32_t>;
extern template class replica_arrays<uint64_t>;

/* One cover bitmap (ceil(num_kmers / 64) words, zeroed) on every resident replica. */
struct cover_bitmaps : replica_arrays<uint64_t> {
    explicit cover_bitmaps(engine const& eng);
    void or_into(uint64_t* h_cover) const;  // every replica's bitmap ORed into the caller's host bitmap; the lanes' work is done
};

/* The deltas of one depth array (num_kmers words of 32 bits, zeroed) on every resident replica. */
struct depth_arrays : replica_arrays<uint32_t> {
    explicit depth_arrays(engine const& eng);
    void add_into(uint32_t* h_depth) const;  // ONCE, when the lanes' work is done: every replica finishes its deltas in place and its depths are added to the caller's host array
private:
    engine const& m_eng;
};

/* The 64-bit exclusive prefix sums of one array of values (num_kmers + 1 words, 8 bytes per k-mer) on every resident replica: `h_values`
   (host, num_kmers words of 32 bits) is uploaded to every replica, the prefix is built there (engine::value_prefix_device) and the
   4-byte copy is freed again. */
struct value_prefixes : replica_arrays<uint64_t> {
    value_prefixes(engine const& eng, uint32_t const* h_values, uint32_t at_least);
};

/* The labels of a classes call (num_strings words of 32 bits) on every resident replica, uploaded once. */
struct class_labels_on_devices : replica_arrays<uint32_t> {
    class_labels_on_devices(engine const& eng, uint32_t const* h_labels);
};

/* What the per-k-mer pipeline fills out of its results beside the arrays of its result_view and the six counters
   (engine::streaming_lookup_device): device pointers, null = not asked for. */
struct per_kmer_outputs {
    uint64_t* rows = nullptr;        // one report per read, n_reads x 6 words, ADDED to
    run_sink const* runs = nullptr;  // the reads' runs, compacted out of the per-k-mer results: run_offsets overwritten, records below its capacity written
    uint64_t* cover = nullptr;       // a cover bitmap: the ids of the positive k-mers ORed into it
    uint32_t* deltas = nullptr;      // the deltas of a depth array: +1 / -1 around every positive k-mer's id added to them
    /* with the prefix sums of a value per k-mer: the value of every positive k-mer and 1 ADDED to the two words of its read's row */
    uint64_t const* prefix = nullptr;
    uint64_t* sums = nullptr;
    /* with a label per string: 1 ADDED, for every positive k-mer, to the column of its string's label in its read's row of num_classes words */
    uint32_t const* labels = nullptr;
    uint32_t num_classes = 0;
    uint32_t* class_rows = nullptr;
};

class engine {
public:
    explicit engine(std::shared_ptr<host_index> idx);
    ~engine();

    host_index const& index() const { return *m_idx; }

    /* Copy the dictionary into the HBM of `device` (no-op when already there). */
    /* table_shards > 1: this replica's super-k-mer table holds only its share of the keys (device_layout.hpp (5)) */
    void to_device(int device, uint32_t table_shards = 1, uint32_t table_shard_id = 0);
    bool on_device(int device) const;
    std::vector<int> devices() const;
    uint64_t device_bytes(int device) const;
    /* {bytes in HBM, directory sectors, directory sectors flagged overflow, keys held by the directory,
        super-k-mer table slots (0 = disabled), its keys, its inline keys, its keys left to the complete path} */
    void device_stats(int device, uint64_t out[16]) const;
    void device_table_histogram(int device, uint64_t out[32]) const;
    /* the replica's super-k-mer table as it lies in HBM, for tests and diagnosis: info = {bytes, buckets of the keys' region, of the
       k-mers' region, bytes per bucket of either, key length, table shards, shard id}; out == nullptr: info only */
    void device_table_export(int device, uint64_t info[8], void* out, uint64_t capacity_bytes) const;

    /* Device-pointer entry points: queries and outputs already live in the HBM of `device`;
       the launch is asynchronous on `stream` (a hipStream_t, may be null = default stream).
       `packed`: n*W u64 words (W = 1 for k<=31, 2 otherwise). `ascii`: n*k chars, no NUL. */
    void lookup_packed_device(int device, uint64_t const* d_kmers, uint64_t n, bool check_rc, out_mode mode,
                              result_view const& d_out, uint8_t* d_member, void* stream) const;
    void lookup_ascii_device(int device, char const* d_kmers, uint64_t n, bool check_rc, out_mode mode,
                             result_view const& d_out, uint8_t* d_member, void* stream) const;

    /* kmer_neighbours (src/dictionary.cpp:111-187) for a batch: the 8 lookups per query, results at 8*i + which
       (which = 0..3 forward with A,C,T,G -- the character's 2-bit code --; 4..7 backward likewise). Device buffers / host buffers. */
    void neighbours_packed_device(int device, uint64_t const* d_kmers, uint64_t n, bool check_rc, out_mode mode,
                                  result_view const& d_out, void* stream) const;
    void neighbours_packed_host(uint64_t const* h_kmers, uint64_t n, bool check_rc, out_mode mode,
                                result_view const& h_out) const;

    /* string_neighbours (src/dictionary.cpp:189-201): forward neighbours of the last k-mer and backward neighbours
       of the first k-mer of every string; same 8-entry layout. Host buffers. */
    void string_neighbours_host(uint64_t const* h_string_ids, uint64_t n, bool check_rc, out_mode mode,
                                result_view const& h_out) const;

    /* The same on the device (sshash_string_neighbours_device): `d_string_ids` null = the strings first_string + i; an id
       >= num_strings gives an all-ones query. Asynchronous; the expanded queries come out of the replica's pool. */
    void string_neighbours_device(int device, uint64_t const* d_string_ids, uint64_t first_string, uint64_t n, bool check_rc, out_mode mode,
                                  result_view const& d_out, void* stream) const;

    /* The links of the strings [begin, end) as CSR (sshash_string_links[_device] in include/sshash_amd.h): one record of 32 bytes per
       found neighbour among the eight of string_neighbours(s). Count -> scan -> write, in rounds of at most 2^22 strings:
       `d_link_offsets` (end - begin + 1 words) is always complete, record i is written iff i < links_capacity. Asynchronous, no host
       synchronisation. Throws on a minimizer shard. The host form runs on the first resident replica. */
    void string_links_device(int device, uint64_t begin, uint64_t end, bool check_rc, uint64_t* d_link_offsets, void* d_links,
                             uint64_t links_capacity, void* stream) const;
    void string_links_host(uint64_t begin, uint64_t end, bool check_rc, uint64_t* link_offsets, void* links, uint64_t links_capacity) const;

    /* Which of its eight neighbours every k-mer of the ids [begin, end) has in the dictionary (sshash_kmer_adjacency[_device]): bit c of
       byte i - begin forward neighbour c, bit 4 + c backward neighbour c. Iterate -> expand -> ids-only lookup -> fold, in rounds
       of at most 2^22 k-mers. Asynchronous. Throws on a minimizer shard. The host form runs on the first resident replica. */
    void kmer_adjacency_device(int device, uint64_t begin, uint64_t end, bool check_rc, uint8_t* d_masks, void* stream) const;
    void kmer_adjacency_host(uint64_t begin, uint64_t end, bool check_rc, uint8_t* masks) const;

    /* access(kmer_id) for a batch of ids, device buffers: out gets n*W packed words
       (all-ones for an id >= num_kmers). */
    void access_packed_device(int device, uint64_t const* d_ids, uint64_t n, uint64_t* d_out, void* stream) const;

    /* the k-mers of the ids [begin, end) in id order (dictionary::at_kmer_id(begin) advanced to end), device buffer: n*W
       packed words; throws unless begin <= end <= num_kmers (engine.hip) */
    void iterate_packed_device(int device, uint64_t begin, uint64_t end, uint64_t* d_out, void* stream) const;
    /* `sshash check` on the replica of `device` (engine.hip; sshash_check_device in include/sshash_amd.h). Synchronous. */
    void check_device(int device, uint64_t out[8]) const;

    /* weight(kmer_id) for a batch of ids, device buffers (all-ones for an id >= num_kmers); throws when the
       dictionary stores no weights */
    void weight_device(int device, uint64_t const* d_ids, uint64_t n, uint64_t* d_out, void* stream) const;

    /* owner shards of every query's forward / reverse-complement minimizer (shard_of_minimizer) */
    void route_packed_device(int device, uint64_t const* d_kmers, uint64_t n, uint32_t num_shards, uint32_t* d_owner_fwd,
                             uint32_t* d_owner_rc, void* stream) const;

    /* the same routing, bucketed on the device (see sshash_route_bucket_device in include/sshash_amd.h) */
    void route_bucket_device(int device, uint64_t const* d_kmers, uint64_t n, uint32_t num_shards, bool check_rc,
                             bool by_table_key, uint64_t* d_cursors, uint64_t* d_send, uint32_t* d_slots, void* stream,
                             uint32_t* d_known_owners = nullptr) const;  // n words kept between the counting and the scattering launch
    void route_combine_device(int device, uint64_t const* d_replies, uint32_t const* d_slots, uint64_t m, uint64_t* d_out,
                              void* stream, bool one_reply_per_query = false) const;

    /* lookup_packed_device over the places i with bit 0 of d_lane_valid[i] set; the outputs of the other places are
       left untouched (the position-parallel streaming lookup, streaming.hip) */
    void lookup_packed_masked_device(int device, uint64_t const* d_kmers, uint8_t const* d_lane_valid, uint64_t n, bool check_rc,
                                     out_mode mode, result_view const& d_out, void* stream) const;

    /* Host-buffer entry points: shard the batch over every replica, stream chunks through
       pinned staging buffers, results land in the caller's arrays. */
    void lookup_packed_host(uint64_t const* h_kmers, uint64_t n, bool check_rc, out_mode mode,
                            result_view const& h_out, uint8_t* h_member) const;
    void lookup_ascii_host(char const* h_kmers, uint64_t n, bool check_rc, out_mode mode, result_view const& h_out,
                           uint8_t* h_member) const;

    /* Batched streaming query over `n_reads` reads stored back to back in `bases`
       (read r = bases[read_offsets[r] .. read_offsets[r+1])). Host buffers. */
    streaming_report streaming_query_host(char const* bases, uint64_t const* read_offsets, uint64_t n_reads) const;
    /* The same with one report PER READ: `rows` (host, n_reads x 6 words in the order of the device report, row r for read r; null:
       the totals only) is overwritten; returns the totals. A piece that holds a read of more than S k-mers takes the run kernel over
       segments (set_read_segments; off: above 2^16 bases the position-parallel pipeline), the others the run kernel; all give the same rows. */
    streaming_report streaming_query_per_read_host(char const* bases, uint64_t const* read_offsets, uint64_t n_reads, uint64_t* rows) const;
    /* An uncompressed FASTQ file, read and parsed by the lanes themselves (reads.hpp: fastq_pieces): every lane takes pieces of
       the file from a shared counter, parses a piece straight into its pinned block, uploads it and runs the streaming
       kernels -- no single reader thread, no intermediate batch. Returns false when the file turned out not to be four lines
       per record (or holds reads longer than a piece): the caller then takes the sequential reader, `total` is untouched. */
    bool streaming_query_fastq_pieces(std::string const& filename, streaming_report& total) const;
    /* Device buffers, asynchronous; `d_report` receives 6 u64 counters (accumulated). */
    /* `segment_kmers` (here and in the three calls like it below): 0 -- one lane walks one read --, S -- the reads are cut into segments
       of S k-mers, one lane a segment, same results (streaming.hip, "long reads: SEGMENTS") --, or SEGMENTS_AS_SET: as
       set_read_segments says for the device calls. */
    static constexpr uint64_t SEGMENTS_AS_SET = ~uint64_t(0) - 1;  // (not SEGMENTS_OFF, which a caller may pass for 0)
    void streaming_query_device(int device, char const* d_bases, uint64_t const* d_read_offsets, uint64_t n_reads,
                                uint64_t total_bases, uint64_t* d_report, void* stream, uint64_t segment_kmers = SEGMENTS_AS_SET) const;
    /* Device buffers, asynchronous, always the run kernel; `d_rows` (n_reads x 6 words) is overwritten, every row of it; `d_report`
       (nullable) is accumulated into. */
    void streaming_query_per_read_device(int device, char const* d_bases, uint64_t const* d_read_offsets, uint64_t n_reads,
                                         uint64_t total_bases, uint64_t* d_rows, uint64_t* d_report, void* stream,
                                         uint64_t segment_kmers = SEGMENTS_AS_SET) const;

    /* Long reads (sshash_set_read_segments in include/sshash_amd.h): `kmers_per_segment` 0 = the default S, SEGMENTS_OFF = never -- the state of
       a new dictionary --, else 1 .. 2^30 (throws otherwise). The host and file calls -- counters, rows, cover, depth, sums, classes -- send a piece that holds a read of more
       than S k-mers through the run kernel over segments; `device_calls`: the six device entry points segment as well. Never on a
       minimizer shard, never the run records. Not to be changed while a call is in flight. */
    void set_read_segments(uint64_t kmers_per_segment, bool device_calls);
    uint64_t read_segment_kmers() const { return m_segment_kmers; }  // S, or SEGMENTS_OFF
    bool read_segments_device_calls() const { return m_segment_device_calls; }
    uint64_t segmented_launches() const { return m_segmented_launches; }  // how often the run kernel was launched over a segment table
    uint64_t host_segments() const;                                        // what the host calls segment with: S, or 0 (off, or a shard)

    /* The maximal runs of every read (sshash_streaming_runs[_device] in include/sshash_amd.h): a run is a search and the extensions
       behind it. Device buffers, asynchronous, always the run kernel: count -> scan -> write; `d_run_offsets` (n_reads + 1 words) is
       overwritten, record i is written iff i < runs_capacity, `d_report` (nullable) is accumulated into. Every read below 2^31
       bases (a record's read_pos and length are 31 bits wide; the host call checks, this one does not). `segment_kmers` as above: over
       segments the runs that span seams are merged in place, the offsets and the records are those of the whole reads. */
    void streaming_runs_device(int device, char const* d_bases, uint64_t const* d_read_offsets, uint64_t n_reads, uint64_t total_bases,
                               uint64_t* d_run_offsets, void* d_runs, uint64_t runs_capacity, uint64_t* d_report, void* stream,
                               uint64_t segment_kmers = SEGMENTS_AS_SET) const;
    /* Host buffers, over all resident replicas; a piece that holds a long read takes the run kernel over segments (set_read_segments;
       off: above 2^16 bases the position-parallel pipeline and a compaction behind it), which give the same records. Throws at a read
       of 2^31 bases or more. Returns the totals. */
    streaming_report streaming_runs_host(char const* bases, uint64_t const* read_offsets, uint64_t n_reads, uint64_t* run_offsets, void* runs,
                                         uint64_t runs_capacity) const;
    /* The same with every record, however many there are: `run_offsets` becomes n_reads + 1 words, `records` four words a record --
       one counting pass for a caller that cannot size its array before (the file call). */
    streaming_report streaming_runs_host(char const* bases, uint64_t const* read_offsets, uint64_t n_reads, std::vector<uint64_t>& run_offsets,
                                         std::vector<uint64_t>& records) const;

    /* WHICH k-mers of the dictionary the reads hold (sshash_streaming_cover[_device] in include/sshash_amd.h): bit i & 63 of word i >> 6
       of `d_cover` (ceil(num_kmers / 64) words) for k-mer id i, ORed into. Device buffers, asynchronous, always the run kernel, its cover
       form: one launch; `d_report` (nullable) is accumulated into. */
    void streaming_cover_device(int device, char const* d_bases, uint64_t const* d_read_offsets, uint64_t n_reads, uint64_t total_bases,
                                uint64_t* d_cover, uint64_t* d_report, void* stream, uint64_t segment_kmers = SEGMENTS_AS_SET) const;
    /* Host buffers, over all resident replicas, into the bitmaps `cover` keeps on them (the caller ORs those into its own when it is
       done: cover_bitmaps::or_into); a piece that holds a long read takes the run kernel over segments (set_read_segments; off: above 2^16
       bases the position-parallel pipeline, which marks from its per-k-mer ids), which gives the same bits. Returns the totals. */
    streaming_report streaming_cover_host(char const* bases, uint64_t const* read_offsets, uint64_t n_reads, cover_bitmaps const& cover) const;
    /* Covered k-mers per string out of a cover bitmap, device buffers, asynchronous: `d_counts` (num_strings words) and `d_total`
       (one word, nullable) are overwritten. */
    void cover_string_counts_device(int device, uint64_t const* d_cover, uint64_t* d_counts, uint64_t* d_total, void* stream) const;

    /* HOW OFTEN the reads hold each k-mer of the dictionary (sshash_streaming_depth[_device] in include/sshash_amd.h), as a difference
       array: for every run of ids [lo, hi) +1 is added to `d_deltas[lo]` and, if hi < num_kmers, -1 to `d_deltas[hi]` (num_kmers words of
       32 bits, modulo 2^32, accumulated into). Device buffers, asynchronous, always the run kernel, its depth form: one launch; `d_report`
       (nullable) is accumulated into. Throws on a minimizer shard (streaming.hip). */
    void streaming_depth_device(int device, char const* d_bases, uint64_t const* d_read_offsets, uint64_t n_reads, uint64_t total_bases,
                                uint32_t* d_deltas, uint64_t* d_report, void* stream, uint64_t segment_kmers = SEGMENTS_AS_SET) const;
    /* d_depth[i] = d_deltas[0] + .. + d_deltas[i] modulo 2^32 for the num_kmers ids; d_depth == d_deltas is allowed, no other overlap.
       Asynchronous; the tile sums (4 bytes per 4096 k-mers) are allocated and freed by the call, stream-ordered, from the replica's pool. */
    void depth_finish_device(int device, uint32_t const* d_deltas, uint32_t* d_depth, void* stream) const;
    /* Host buffers, over all resident replicas, into the deltas `depth` keeps on them (the caller adds the finished depths into its own
       array when it is done: depth_arrays::add_into); a piece that holds a long read takes the run kernel over segments (set_read_segments; off: above 2^16 bases the
       position-parallel pipeline, marked from its per-k-mer ids), which gives the same depths -- every piece of a minimizer shard takes that pipeline. Returns the totals. */
    streaming_report streaming_depth_host(char const* bases, uint64_t const* read_offsets, uint64_t n_reads, depth_arrays const& depth) const;
    /* The 64-bit sum of a depth array over the ids of every string, device buffers, asynchronous: `d_sums` (num_strings words) and
       `d_total` (one word, nullable) are overwritten. */
    void depth_string_sums_device(int device, uint32_t const* d_depth, uint64_t* d_sums, uint64_t* d_total, void* stream) const;

    /* The 64-bit exclusive prefix sums of a value per k-mer (sshash_value_prefix_device in include/sshash_amd.h): d_prefix[i] = the sum of
       d_values[j], j < i -- or, at_least >= 1, the number of j < i with d_values[j] >= at_least --, num_kmers + 1 words, overwritten.
       Asynchronous: one widening launch, then the 64-bit scan in place; its tile sums are allocated and freed by the call,
       stream-ordered, from the replica's pool. */
    void value_prefix_device(int device, uint32_t const* d_values, uint32_t at_least, uint64_t* d_prefix, void* stream) const;
    /* PER READ, the sum of a value per k-mer over the read's positive k-mers and their number (sshash_streaming_sums[_device]): row r of
       `d_sums` (two words a read) is overwritten, `d_prefix` (value_prefix_device) is only read. Device buffers, asynchronous, always
       the run kernel, its sums form: a memset and one launch; `d_report` (nullable) is accumulated into. Throws on a minimizer shard. */
    void streaming_sums_device(int device, char const* d_bases, uint64_t const* d_read_offsets, uint64_t n_reads, uint64_t total_bases,
                               uint64_t const* d_prefix, uint64_t* d_sums, uint64_t* d_report, void* stream,
                               uint64_t segment_kmers = SEGMENTS_AS_SET) const;
    /* Host buffers, over all resident replicas, out of the prefixes `prefix` keeps on them; `sums` (host, n_reads x 2 words) is
       overwritten. A piece that holds a long read takes the run kernel over segments (set_read_segments; off: above 2^16 bases the
       position-parallel pipeline, summed from its per-k-mer ids), which gives the same rows -- every piece of a minimizer shard takes
       that pipeline. Returns the totals. */
    streaming_report streaming_sums_host(char const* bases, uint64_t const* read_offsets, uint64_t n_reads, value_prefixes const& prefix,
                                         uint64_t* sums) const;

    /* PER READ, its positive k-mers by CLASS OF STRING (sshash_streaming_classes[_device]): word c of row r of `d_rows` (num_classes words
       of 32 bits a read, overwritten) = the positive k-mers of read r in strings s with d_labels[s] == c (num_strings words, only read; a
       label >= num_classes is no class). Device buffers, asynchronous, always the run kernel, its classes form: a memset and one launch;
       `d_report` (nullable) is accumulated into. Throws on a minimizer shard. */
    static constexpr uint32_t MAX_CLASSES = 4096;  // SSHASH_MAX_CLASSES
    void streaming_classes_device(int device, char const* d_bases, uint64_t const* d_read_offsets, uint64_t n_reads, uint64_t total_bases,
                                  uint32_t const* d_labels, uint32_t num_classes, uint32_t* d_rows, uint64_t* d_report, void* stream,
                                  uint64_t segment_kmers = SEGMENTS_AS_SET) const;
    /* Host buffers, over all resident replicas, with the labels `labels` keeps on them; `rows` (host, n_reads x num_classes words) is
       overwritten. Pieces as the sums, and no piece of more reads than make 64 MiB of rows; a piece with a long read and every piece of
       a minimizer shard is counted from the per-k-mer ids (classes_add_ids_kernel). Returns the totals. */
    streaming_report streaming_classes_host(char const* bases, uint64_t const* read_offsets, uint64_t n_reads, class_labels_on_devices const& labels,
                                            uint32_t num_classes, uint32_t* rows) const;
    /* The finish of the rows (sshash_class_best_device, sshash_class_totals_device): device buffers, asynchronous, outputs overwritten. */
    void class_best_device(int device, uint32_t const* d_rows, uint64_t n_reads, uint32_t num_classes, uint32_t* d_best /* four words a read */, void* stream) const;
    void class_totals_device(int device, uint32_t const* d_rows, uint64_t n_reads, uint32_t num_classes, uint64_t* d_totals, void* stream) const;

    /* PER READ, its LONGEST RUN (sshash_streaming_best_run[_device]): record r of `d_best` (one sshash_streaming_run of 32 bytes a read,
       overwritten) = the run of read r with the most k-mers, among equals the first in read order; 32 zero bytes for a read without a
       hit. Device buffers, asynchronous, always the run kernel, its best-run form: a memset and one launch, never over segments;
       `d_report` (nullable) is accumulated into. Throws on a minimizer shard. */
    void streaming_best_run_device(int device, char const* d_bases, uint64_t const* d_read_offsets, uint64_t n_reads, uint64_t total_bases, void* d_best,
                                   uint64_t* d_report, void* stream) const;
    /* Host buffers, over all resident replicas; `best` (host, n_reads records) is overwritten. A piece with a read above 2^16 bases
       goes through the per-k-mer pipeline's run records and runs_best_device. Throws on a minimizer shard. Returns the totals. */
    streaming_report streaming_best_run_host(char const* bases, uint64_t const* read_offsets, uint64_t n_reads, void* best) const;
    /* no_device unless a replica is resident, then argument on a minimizer shard: what the file call asks before it opens its file */
    void best_run_ready() const;
    /* The finish of a complete CSR of run records (sshash_runs_best_device): per read the longest of d_runs[d_run_offsets[r] ..
       d_run_offsets[r + 1]), among equals the first; zero bytes for an empty range. Device buffers, asynchronous, `d_best` overwritten. */
    void runs_best_device(int device, uint64_t const* d_run_offsets, void const* d_runs, uint64_t n_reads, void* d_best, void* stream) const;

    /* Per-k-mer results of the streaming query (streaming_query::lookup for every k-mer of every read,
       include/streaming_query.hpp:56-109): entry read_offsets[r] + j of every non-null array of `d_out` = the k-mer
       starting at base j of read r; places where no k-mer starts are left untouched. `d_report` (nullable): the six
       counters, accumulated. Device buffers, asynchronous. */
    void streaming_lookup_device(int device, char const* d_bases, uint64_t const* d_read_offsets, uint64_t n_reads,
                                 uint64_t total_bases, result_view const& d_out, uint64_t* d_report, void* stream,
                                 per_kmer_outputs const& more = {}) const;
    streaming_report streaming_lookup_host(char const* bases, uint64_t const* read_offsets, uint64_t n_reads,
                                           result_view const& h_out) const;

    /* Lookup against a dictionary partitioned over `num_ranks` GPUs (minimizer shards, or table shards with
       by_table_key): route -> exchange -> lookup -> return -> combine (sharded.cpp). Collective: every rank calls it, with
       its own local batch (n may be 0). d_out: n ids. */
    void sharded_lookup_device(int device, uint32_t num_ranks, bool by_table_key, uint64_t const* d_kmers, uint64_t n, bool check_rc,
                               uint64_t* d_out, exchange_ops const& x, void* stream) const;
    void sharded_lookup_rccl(int device, void* nccl_comm, bool by_table_key, uint64_t const* d_kmers, uint64_t n, bool check_rc,
                             uint64_t* d_out, void* stream) const;

    /* the replica resident on `device` (throws when there is none); internal to the .hip files */
    device_replica const* replica(int device) const;

private:
    uint64_t segments_for(uint64_t asked) const;  // (streaming.hip)
    /* what the streaming_*_device entry points share behind their own argument checks (streaming.hip) */
    template <class Launch>
    void run_kernel_call(int device, uint64_t const* d_read_offsets, uint64_t n_reads, uint64_t total_bases, void* stream, uint64_t segment_kmers,
                         void* d_rows, uint64_t row_bytes, Launch const& launch) const;
    std::shared_ptr<host_index> m_idx;
    std::atomic<uint64_t> m_segment_kmers{SEGMENTS_OFF};  // (opt-in: a new dictionary takes the routes it always took)
    std::atomic<bool> m_segment_device_calls{false};
    mutable std::atomic<uint64_t> m_segmented_launches{0};
    /* to_device may run while other host threads query: readers share, the upload's final push_back is exclusive */
    mutable std::shared_mutex m_replicas_mutex;
    std::mutex m_upload_mutex;
    std::vector<std::unique_ptr<device_replica>> m_replicas;
};

int visible_device_count();  // 0 when no GPU / no driver
char const* isa_guard_state();  // "guarded": device code built through tools/isa_guard.py; "plain": by hipcc alone (engine.hip)

}  // namespace sshash_amd
