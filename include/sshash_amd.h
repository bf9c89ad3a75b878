/* sshash_amd.h -- C ABI of the MI355X-native batched k-mer Lookup engine for SSHash.
 *
 * The reference (jermp/sshash) has no FFI layer: its boundary for this path is the C++ class
 * `sshash::dictionary<Kmer, Offsets>` (reference include/dictionary.hpp:10-181). Each entry
 * point below names the reference interface it stands in for. Conventions:
 *   - opaque handle, plain pointers and sizes, no exceptions across the ABI;
 *   - every function returns an sshash_status; sshash_last_error() gives the message of the
 *     last failure on the calling thread;
 *   - "not found" is NOT an error: kmer_id == SSHASH_INVALID_U64 (include/constants.hpp:5);
 *   - lookups run on the GPU only. Without a visible HIP device they fail with
 *     SSHASH_ERR_NO_DEVICE; there is no CPU fallback.
 *   - k-mers are 2-bit packed, first base in the least-significant bits, A=0 C=1 T=2 G=3
 *     (include/kmer.hpp:80,194); W = 1 64-bit word per k-mer for k <= 31, W = 2 for k <= 63.
 */
#ifndef SSHASH_AMD_H
#define SSHASH_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SSHASH_INVALID_U64 UINT64_MAX

typedef enum sshash_status {
    SSHASH_OK = 0,
    SSHASH_ERR_ARGUMENT = 1,  /* null pointer, bad k/m, id out of range ...                    */
    SSHASH_ERR_IO = 2,        /* "error in opening the file" (src/query.cpp:128, tools/build.cpp) */
    SSHASH_ERR_FORMAT = 3,    /* not an index file / corrupt                                     */
    SSHASH_ERR_VERSION = 4,   /* "MAJOR index version mismatch" (include/util.hpp:191-195)       */
    SSHASH_ERR_NO_DEVICE = 5, /* no HIP device visible, or dictionary not resident on the device  */
    SSHASH_ERR_HIP = 6,       /* a HIP runtime call failed                                       */
    SSHASH_ERR_BUILD = 7,     /* index construction failed                                       */
    SSHASH_ERR_INTERNAL = 8
} sshash_status;

typedef struct sshash_dict sshash_dict; /* stands for sshash::dictionary_type (include/dictionary_types.hpp:9) */

/* build_configuration (include/util.hpp:143-159); zero-initialise then override. */
typedef struct sshash_build_config {
    uint32_t k;           /* default 31 */
    uint32_t m;           /* default 20 */
    uint64_t seed;        /* default 1  */
    uint32_t canonical;   /* default 0  */
    uint32_t num_threads; /* default 1; 0 = hardware concurrency */
    double lambda;        /* default 5.0 */
    uint32_t verbose;
    uint32_t weighted;    /* build_configuration::weighted: FASTA headers carry '>[id] LN:i:[len] ab:Z:[weights]'
                             (src/builder/encode_strings.cpp:83-135); sshash_build_from_fasta only */
    /* minimizer-sharded build for dictionaries larger than one GPU's HBM: keep only the buckets of the
     * minimizers owned by shard `shard_id` of `num_shards` (strings stay complete). 0/1 = whole index. */
    uint32_t num_shards;
    uint32_t shard_id;
} sshash_build_config;

/* accessors of dictionary (include/dictionary.hpp:31-38) */
typedef struct sshash_info {
    uint8_t version[3];
    uint8_t canonical;
    uint32_t k, m;
    uint32_t words_per_kmer;
    uint64_t num_kmers, num_strings, num_bases, num_minimizers;
    uint64_t num_bits;      /* dictionary::num_bits(), host representation */
    uint32_t skew_partitions;
    uint32_t weighted;   /* dictionary::weighted() */
    uint32_t num_shards; /* 1 unless built as one shard of a minimizer-partitioned index */
    uint32_t shard_id;
} sshash_info;

/* lookup_result (include/util.hpp:38-62) as a struct of arrays: one entry per query.
 * kmer_id is mandatory for sshash_lookup_*; any other pointer may be NULL (field not produced).
 * A query that is not found has every u64 field == SSHASH_INVALID_U64. */
typedef struct sshash_results {
    uint64_t* kmer_id;
    uint64_t* kmer_id_in_string;
    uint64_t* kmer_offset;
    uint64_t* string_id;
    uint64_t* string_begin;
    uint64_t* string_end;
    int8_t* kmer_orientation;  /* +1 forward, -1 backward (include/constants.hpp:17-18) */
    uint8_t* minimizer_found;
} sshash_results;

/* streaming_query_report (include/util.hpp:21-36) */
typedef struct sshash_streaming_report {
    uint64_t num_kmers;
    uint64_t num_positive_kmers;
    uint64_t num_negative_kmers;
    uint64_t num_invalid_kmers;
    uint64_t num_searches;
    uint64_t num_extensions;
} sshash_streaming_report;

const char* sshash_last_error(void);
/* how the library was built, "key=value;..." (no reference counterpart): isa_guard=guarded|plain -- whether the device code went
 * through tools/isa_guard.py, which keeps a gfx950 register hazard out of the kernels (a plain build also warns at the first upload) */
const char* sshash_build_info(void);
void sshash_build_config_default(sshash_build_config* cfg);

/* ---- construction / persistence: dictionary::build (src/builder/build.cpp:10-28),
 *      essentials::save / load (tools/build.cpp:90-95, tools/common.hpp:19-22) ------------- */
sshash_status sshash_build_from_fasta(const char* filename, const sshash_build_config* cfg, sshash_dict** out);
/* strings already 2-bit packed back to back: `words` holds endpoints[num_strings] bases. */
sshash_status sshash_build_from_packed(const uint64_t* words, const uint64_t* endpoints, uint64_t num_strings,
                                       const sshash_build_config* cfg, sshash_dict** out);
sshash_status sshash_save(const sshash_dict* d, const char* filename);
sshash_status sshash_load(const char* filename, sshash_dict** out);
void sshash_free(sshash_dict* d);
sshash_status sshash_get_info(const sshash_dict* d, sshash_info* info);

/* The bucket statistics `sshash build --verbose` prints (src/builder/build_sparse_and_skew_index.cpp:64-99,
 * include/buckets_statistics.hpp: "num_buckets_larger_than_1_not_in_skew_index", "num_buckets_in_skew_index",
 * "max_bucket_size", "num kmers in skew index", "buckets with s minimizer positions"), recomputed from the finished index:
 * out = { [0] minimizers, [1] minimizer positions, [2] buckets of 2..64 positions, [3] positions in them, [4] buckets in the
 *         skew index, [5] positions in them, [6] k-mers in the skew index, [7] largest bucket, [8..15] k-mers per skew
 *         partition, [16..31] buckets of exactly 1..16 positions, [32] k-mers, [33] strings, [34] bases, [35] skew
 *         partitions, [36] longest string, [37..63] zero } */
sshash_status sshash_bucket_stats(const sshash_dict* d, uint64_t out[64]);

/* ---- device residency (no reference counterpart: the reference is host-only) ------------- */
int sshash_device_count(void);
sshash_status sshash_to_device(sshash_dict* d, int device);
/* The same, with the super-k-mer table (the largest device structure) partitioned over several
 * GPUs: this replica builds the slots of the keys it owns only (shard `table_shard_id` of `num_table_shards`); queries
 * are meant to reach it through sshash_route_bucket_by_key_device, but any query is still answered correctly (a key
 * of another shard takes the complete path). Everything else is resident in full. */
sshash_status sshash_to_device_table_shard(sshash_dict* d, int device, uint32_t num_table_shards, uint32_t table_shard_id);
sshash_status sshash_device_bytes(const sshash_dict* d, int device, uint64_t* bytes);
/* out = { [0] bytes in HBM, [1] minimizer-directory sectors (0 = disabled), [2] sectors flagged overflow, [3] keys in the
 *         directory, [4] super-k-mer table slots (0 = no table), [5] its keys, [6] keys held inline (<= 4 occurrences),
 *         [7] items left to the complete path (no free slot in any of their buckets), [8] slots in use (load factor =
 *         [8] / [4]), [9] heavy keys (a marker + one slot per k-mer), [10] k-mers entered one by one, [11] why there is no
 *         table: 0 = there is one, 1 = disabled (SSHASH_AMD_SKTABLE=0), 2 = minimizer shard (keeps the directory path),
 *         3 = more than 2^39 bases, 4 = more items than one build pass holds (2^31 super-k-mers), 5 = not enough free HBM
 *         -- in all these cases lookups take the directory / MPHF path, about half as fast --, [12] bytes of the table,
 *         [13..15] reserved } */
sshash_status sshash_device_stats(const sshash_dict* d, int device, uint64_t out[16]);
/* The keys of the super-k-mer table by number of occurrences -- the table-side counterpart of sshash_bucket_stats (a key
 * with more than 4 occurrences is "heavy": one slot per k-mer, one more bucket read per lookup):
 * out = { [0..9) keys with 1, 2, 3, 4, 5-8, 9-16, 17-64, 65-1024, > 1024 occurrences, [9..18) the occurrences (super-k-mers)
 *         in each of these bins, [18] super-k-mers in all, [19] slots asked for (inline occurrences + markers + k-mers of heavy
 *         keys), [20..31] zero }; all zero when the replica has no table. */
sshash_status sshash_device_table_histogram(const sshash_dict* d, int device, uint64_t out[32]);
/* A read-only copy of the replica's super-k-mer table as it lies in HBM, for tests and diagnosis -- the whole
 * table crosses to the host, so it is sized for small replicas:
 * info = { [0] bytes of the table, [1] buckets of the keys' region, [2] buckets of the k-mers' region, [3] bytes per bucket of the
 *          keys' region (64, or 128 at k > 31), [4] bytes per bucket of the k-mers' region (64), [5] length of the table's keys,
 *          [6] table shards, [7] shard id }; all zero (and nothing copied) when the replica has no table.
 * out == NULL: info only. Otherwise the device is synchronised and info[0] bytes are copied to `out`; SSHASH_ERR_ARGUMENT if
 * capacity_bytes < info[0]. The keys' region comes first, the k-mers' region behind it. */
sshash_status sshash_device_table_export(const sshash_dict* d, int device, uint64_t info[8], void* out, uint64_t capacity_bytes);

/* ---- dictionary::lookup(Kmer, bool) / lookup(char const*, bool): include/dictionary.hpp:41-42,
 *      src/dictionary.cpp:58-78. Batched. ------------------------------------------------------
 * *_device: `kmers` and every non-NULL array of `out` are DEVICE pointers in the HBM of `device`;
 *           the launch is asynchronous on `hip_stream` (hipStream_t as void*, NULL = default stream).
 * host variants: caller-owned host buffers; the batch is sharded over all resident devices. Page-locked buffers (hipHostMalloc /
 *           hipHostRegister; input AND every requested output) are copied from and to directly: 4.3 G lookups/s over PCIe
 *           against 1.5 G/s for pageable memory, which is staged through the library's own pinned lanes.
 * Cost of the fields: NULL arrays are skipped. kmer_id alone is answered by the device's super-k-mer table at full speed (DESIGN.md
 * section 6: 38-40 G lookups/s); the position fields come from the same probe (all seven: 25 G/s at 50 % positives -- seven output
 * streams, and string_begin / string_end cost a hit one more random read). `minimizer_found` is true for a hit; for a miss only the
 * MPHF can reproduce it -- the flag of an absent minimizer depends on which bucket the MPHF maps that minimizer to
 * (include/spectrum_preserving_string_set.hpp:46-65) --, so the misses of a batch that asks for it go through the MPHF path in a
 * last pass that stores that one byte (one probe: the reference's result for a miss is that of its last probe): 20 G/s at 100 %
 * positives, 14 at 50 %, 11 at 0 %. The eight-field result is an extension: the reference's own comparator of lookup results ignores
 * that flag (include/util.hpp:107-141), and for an absent minimizer its value is an artefact of this build's MPHF. */
sshash_status sshash_lookup_packed_device(const sshash_dict* d, int device, const uint64_t* kmers, uint64_t n,
                                          int check_reverse_complement, const sshash_results* out, void* hip_stream);
sshash_status sshash_lookup_ascii_device(const sshash_dict* d, int device, const char* kmers, uint64_t n,
                                         int check_reverse_complement, const sshash_results* out, void* hip_stream);
sshash_status sshash_lookup_packed(const sshash_dict* d, const uint64_t* kmers, uint64_t n, int check_reverse_complement,
                                   const sshash_results* out);
sshash_status sshash_lookup_ascii(const sshash_dict* d, const char* kmers, uint64_t n, int check_reverse_complement,
                                  const sshash_results* out);

/* ---- dictionary::is_member: include/dictionary.hpp:75-76, src/dictionary.cpp:80-88 -------- */
sshash_status sshash_is_member_packed_device(const sshash_dict* d, int device, const uint64_t* kmers, uint64_t n,
                                             int check_reverse_complement, uint8_t* out, void* hip_stream);
sshash_status sshash_is_member_packed(const sshash_dict* d, const uint64_t* kmers, uint64_t n, int check_reverse_complement,
                                      uint8_t* out);
sshash_status sshash_is_member_ascii(const sshash_dict* d, const char* kmers, uint64_t n, int check_reverse_complement,
                                     uint8_t* out);

/* ---- dictionary::access (include/dictionary.hpp:69, src/dictionary.cpp:90-94): host side,
 *      used to draw positive queries as tools/perf.hpp:38-51 does ---------------------------- */
sshash_status sshash_access(const sshash_dict* d, uint64_t kmer_id, char* out_k_chars);
sshash_status sshash_access_packed(const sshash_dict* d, const uint64_t* kmer_ids, uint64_t n, uint64_t* out_words);
/* the same on the GPU: device pointers, asynchronous; an id >= num_kmers yields all-ones words */
sshash_status sshash_access_packed_device(const sshash_dict* d, int device, const uint64_t* kmer_ids, uint64_t n,
                                          uint64_t* out_words, void* hip_stream);

/* ---- dictionary::begin / at_kmer_id / at_string_id (include/dictionary.hpp:84-121) and the iterator behind them
 *      (include/spectrum_preserving_string_set.hpp:120-183), a whole id range per call:
 *      out_words[(i - begin)*W ..) = the k-mer with id i, for i in [begin_kmer_id, end_kmer_id) -- the value sshash_access_packed
 *      gives for i. at_string_id(s) is the range [string_offsets(s).begin - s*(k-1), string_offsets(s).end - (s+1)*(k-1)).
 *      SSHASH_ERR_ARGUMENT when begin > end, end > num_kmers, or out_words is NULL and the range is not empty; begin == end writes
 *      nothing. The device variant is asynchronous on hip_stream (device pointer; ids are 64-bit, a range is not limited to 2^32
 *      ids); the host variant decodes the host index on the CPU (no GPU needed), sliding one base at a time inside every string. */
sshash_status sshash_iterate_packed_device(const sshash_dict* d, int device, uint64_t begin_kmer_id, uint64_t end_kmer_id,
                                           uint64_t* out_words, void* hip_stream);
sshash_status sshash_iterate_packed(const sshash_dict* d, uint64_t begin_kmer_id, uint64_t end_kmer_id, uint64_t* out_words);

/* The reference's `sshash check` (tools/sshash.cpp:20-36, test/check.hpp:7-75) on the replica of `device`: every k-mer of the
 * dictionary, taken by the iterator, is looked up (check_reverse_complement = 1) forward and reverse-complemented, and is_member
 * is asked. out = { [0] k-mers checked, [1] forward lookups not found, [2] forward lookups with another id, [3] reverse-complement
 * lookups not found or with another id, [4] is_member false, [5] smallest failing id or UINT64_MAX, [6..8) 0 }. Runs 2^25 k-mers
 * at a time with scratch of its own, freed before it returns. Synchronous: returns when the counts are on the host.
 * SSHASH_ERR_ARGUMENT on a minimizer shard (num_shards > 1), which answers only the k-mers it owns; table-shard replicas answer
 * every query and are checked. */
sshash_status sshash_check_device(const sshash_dict* d, int device, uint64_t out[8]);

/* ---- dictionary::weight(kmer_id): include/dictionary.hpp (weight), src/dictionary.cpp:96-100,
 *      include/weights.hpp:147-152. Batched; SSHASH_ERR_ARGUMENT when the dictionary stores no weights
 *      (the reference's checker refuses it the same way, test/check_from_file.hpp:234-237) or an id is
 *      >= num_kmers (host variant; the device variant writes UINT64_MAX for such an id). */
sshash_status sshash_weight(const sshash_dict* d, const uint64_t* kmer_ids, uint64_t n, uint64_t* out_weights);
sshash_status sshash_weight_device(const sshash_dict* d, int device, const uint64_t* kmer_ids, uint64_t n,
                                   uint64_t* out_weights, void* hip_stream);

/* ---- dictionary::kmer_neighbours(Kmer, bool): include/dictionary.hpp:59-61, src/dictionary.cpp:111-126,176-187.
 *      Batched: every array of `out` holds 8*n entries; entry 8*i + c (c = 0..3) is the lookup of the forward
 *      neighbour suffix(kmer i) + "ACTG"[c], entry 8*i + 4 + c the backward neighbour "ACTG"[c] + prefix(kmer i): c is
 *      the 2-bit code of the character, the reference's alphabet order (include/kmer.hpp:118; its own checker indexes
 *      forward[char_to_uint(next)], test/check_from_file.hpp:198-216)
 *      (neighbourhood::forward / ::backward, include/util.hpp:78-81). Same pointer rules as the lookups. */
sshash_status sshash_neighbours_packed_device(const sshash_dict* d, int device, const uint64_t* kmers, uint64_t n,
                                              int check_reverse_complement, const sshash_results* out, void* hip_stream);
sshash_status sshash_neighbours_packed(const sshash_dict* d, const uint64_t* kmers, uint64_t n,
                                       int check_reverse_complement, const sshash_results* out);

/* dictionary::string_size(string_id): include/dictionary.hpp:44-46, src/dictionary.cpp:102-109 -- the number of
 * k-mers of each string (its length is size + k - 1). Host arrays. */
sshash_status sshash_string_size(const sshash_dict* d, const uint64_t* string_ids, uint64_t n, uint64_t* out_sizes);
/* dictionary::string_offsets(string_id) -> [begin, end) in bases (include/dictionary.hpp:105-108): what lookup_result's
 * string_begin / string_end refer to */
sshash_status sshash_string_offsets(const sshash_dict* d, const uint64_t* string_ids, uint64_t n, uint64_t* out_begin, uint64_t* out_end);

/* dictionary::string_neighbours(string_id, bool): include/dictionary.hpp:62, src/dictionary.cpp:189-201 -- the
 * forward neighbours of the string's last k-mer and the backward neighbours of its first one, same layout. */
sshash_status sshash_string_neighbours(const sshash_dict* d, const uint64_t* string_ids, uint64_t n,
                                       int check_reverse_complement, const sshash_results* out);
/* The same on the device, asynchronous on hip_stream: string_ids is a device pointer, or NULL for the strings first_string + i
 * (first_string + n > num_strings is then SSHASH_ERR_ARGUMENT). Same layout -- every array of `out` holds 8*n entries, entry 8*i + c
 * the forward neighbour "ACTG"[c] of the string's last k-mer, entry 8*i + 4 + c the backward neighbour of its first -- and the same
 * pointer rules as sshash_neighbours_packed_device; any field may be asked for. One kernel decodes both end k-mers of every string
 * out of the replica and expands them, the batched lookup follows. A string id >= num_strings in string_ids gives an all-ones
 * query, as sshash_access_packed_device writes for an id past the end: eight not-found results (unless the dictionary holds the
 * k-mer of k G's, which those words spell). */
sshash_status sshash_string_neighbours_device(const sshash_dict* d, int device, const uint64_t* string_ids, uint64_t first_string, uint64_t n,
                                              int check_reverse_complement, const sshash_results* out, void* hip_stream);

/* ---- The dictionary as a graph: the LINKS between its strings, as CSR.
 * One record per found neighbour among the eight of string_neighbours(s): the records of string begin_string + i are
 * links[link_offsets[i] .. link_offsets[i + 1]), in increasing flags & 7, at most 8 per string. The layout is canonical: two calls
 * over the same range give byte-identical arrays.
 * Capacity, exactly as sshash_streaming_runs_device: link_offsets (end - begin + 1 words, [0] = 0) is always complete and exact,
 * record i is written iff i < links_capacity, nothing at or beyond links + links_capacity is touched; links == NULL with capacity 0 is
 * the counting call.
 * Orientation (for a GFA): from_sign is '+' iff bit 2 is clear; to_sign is '+' iff (bit 3 clear) == (bit 2 clear). A link is END-TO-END --
 * it joins two string ends, an L line -- iff
 *     bit 2 clear and (bit 3 clear and bit 4 set, or bit 3 set and bit 5 set), or
 *     bit 2 set   and (bit 3 clear and bit 5 set, or bit 3 set and bit 4 set);
 * any other link lands inside to_string (a junction inside a stitched string).
 * SSHASH_ERR_ARGUMENT, before anything runs: begin > end, end > num_strings, link_offsets NULL, links NULL with capacity > 0, or a
 * minimizer shard (num_shards > 1: it answers only the k-mers it owns, as sshash_check_device). Table-shard replicas work. The device
 * form is asynchronous on hip_stream with no host synchronisation: rounds of at most 2^22 strings -- the ends' neighbours, an
 * ids-only lookup, a count per string --, a prefix sum over link_offsets and, with capacity > 0, the rounds again with the lookup of
 * the record's fields and a scatter; scratch of one round out of the replica's stream-ordered pool. links: 16-byte aligned.
 * The host form takes host arrays and runs on the first resident replica. */
typedef struct sshash_string_link {
    uint64_t from_string; /* the string whose end the link leaves */
    uint64_t to_string;   /* lookup_result::string_id of the neighbour k-mer */
    uint64_t to_kmer_id;  /* lookup_result::kmer_id of the neighbour k-mer */
    uint32_t flags;       /* bits 0-1: the base's 2-bit code c; bit 2: leaves the string's START (backward neighbour; clear: its END);
                             bit 3: neighbour found as reverse complement (orientation -1); bit 4: it is the FIRST k-mer of to_string;
                             bit 5: it is the LAST k-mer of to_string (both set: a string of one k-mer) */
    uint32_t reserved;    /* 0 */
} sshash_string_link;     /* 32 bytes */
sshash_status sshash_string_links_device(const sshash_dict* d, int device, uint64_t begin_string, uint64_t end_string, int check_reverse_complement,
                                         uint64_t* link_offsets, sshash_string_link* links, uint64_t links_capacity, void* hip_stream);
sshash_status sshash_string_links(const sshash_dict* d, uint64_t begin_string, uint64_t end_string, int check_reverse_complement,
                                  uint64_t* link_offsets, sshash_string_link* links, uint64_t links_capacity);

/* ---- The ADJACENCY of every k-mer of the ids [begin_kmer_id, end_kmer_id): bit c of masks[i - begin] is set iff the forward neighbour
 * "ACTG"[c] of k-mer i is in the dictionary, bit 4 + c the same for its backward neighbour (a k-mer that is its own neighbour
 * counts: the lookup finds it). This tells a junction inside a stitched string from a non-branching position, which no per-string
 * call can. masks: end - begin bytes. Range errors as sshash_iterate_packed_device; SSHASH_ERR_ARGUMENT on a minimizer shard. The
 * device form is asynchronous: rounds of at most 2^22 k-mers -- the iterator, the 8 neighbours, an ids-only lookup, 8 ids folded
 * into a byte. The host form takes a host array and runs on the first resident replica. */
sshash_status sshash_kmer_adjacency_device(const sshash_dict* d, int device, uint64_t begin_kmer_id, uint64_t end_kmer_id, int check_reverse_complement,
                                           uint8_t* masks, void* hip_stream);
sshash_status sshash_kmer_adjacency(const sshash_dict* d, uint64_t begin_kmer_id, uint64_t end_kmer_id, int check_reverse_complement, uint8_t* masks);

/* ---- dictionary::streaming_query_from_file (include/dictionary.hpp:81-82, src/query.cpp:118-175)
 *      and streaming_query<Dict,canonical> over reads in memory (include/streaming_query.hpp) --
 * The file (.fa/.fasta/.fq/.fastq, optionally .gz) is read ~256 MiB of bases at a time by a reader thread while the
 * devices work on the previous batch: host memory stays bounded whatever the size of the file. The call runs at the reader's
 * pace (the devices are busy a tenth of the time): a plain file at ~9 GB/s, a .gz at one thread's inflate (0.28 G bases/s), a BGZF
 * .gz (bgzip's gzip members, recognised by the first header) inflated on min(16, cores) threads (SSHASH_AMD_READER_THREADS). */
sshash_status sshash_streaming_query_from_file(const sshash_dict* d, const char* filename, int multiline,
                                               sshash_streaming_report* report);
/* reads stored back to back: read r = bases[read_offsets[r] .. read_offsets[r+1]) ; host buffers */
sshash_status sshash_streaming_query(const sshash_dict* d, const char* bases, const uint64_t* read_offsets,
                                     uint64_t num_reads, sshash_streaming_report* report);
/* device buffers; `report` is a device pointer to 6 uint64 counters, accumulated into. `total_bases` = read_offsets[num_reads] (as
 * sshash_streaming_lookup_device takes it): the size of the 2-bit packed copy of the reads the call makes in scratch the replica keeps
 * per stream. With it the call only enqueues work on `hip_stream` and returns. 0 = "not known to the caller": the call then reads
 * read_offsets[num_reads] back (8 bytes) and so waits for what the stream holds at that moment -- its one synchronisation. */
sshash_status sshash_streaming_query_device(const sshash_dict* d, int device, const char* bases,
                                            const uint64_t* read_offsets, uint64_t num_reads, uint64_t total_bases,
                                            uint64_t* report, void* hip_stream);

/* ---- LONG READS: segments. The streaming calls run on the run kernel, where one lane walks one read: a batch of few long reads -- ONT
 *      or HiFi reads, contigs, chromosomes -- is few lanes, and takes as long as its longest read. A k-mer is positive, negative or
 *      invalid whatever lies around it, so such a read can be cut: with S = kmers_per_segment a read of K k-mers becomes ceil(K / S)
 *      SEGMENTS of S k-mers (neighbours overlap by k - 1 bases; nothing is copied), one lane each. What differs is put right on the
 *      device: a segment's first k-mer counts as a search where in the whole read it may be an extension -- the rule of the runs
 *      below --, and a pass over the seams moves those back. The six counters, every per-read row, the cover, the depth, the sums and
 *      the classes are word for word what the uncut reads give, and so are the run records: a run that goes on over a seam is merged on
 *      the device, without moving a record.
 *      Segmenting is OPT-IN: a new dictionary is at SSHASH_SEGMENTS_OFF with device_calls = 0 and takes the routes it always took.
 *      kmers_per_segment: 0 = the library's default S (256, RESULTS.md: best of 256, 1024, 4096 through the host call; the device calls
 *      favour 1024 slightly); SSHASH_SEGMENTS_OFF = never segment; otherwise 1 .. 2^30 (tiny values are allowed and only slow: tests
 *      put seams into small reads with them). Anything else, or a NULL dictionary, is SSHASH_ERR_ARGUMENT. Needs no device. Not to be changed while a call
 *      on the dictionary is in flight.
 *      Host and file calls (sshash_streaming_query, _per_read, _runs, _cover, _depth, _sums, _classes and their _from_file forms), once an S is set: a piece of
 *      the batch that holds a read of more than S k-mers takes the run kernel over segments; pieces of shorter reads take exactly the launches they took
 *      before. With SSHASH_SEGMENTS_OFF a piece that holds a read above 2^16 bases goes through the position-parallel pipeline of
 *      sshash_streaming_lookup instead (one point lookup per k-mer, the same results).
 *      Device calls (sshash_streaming_query_device, _per_read_device, _runs_device, _cover_device, _depth_device, _sums_device, _classes_device): segment only with device_calls != 0
 *      -- they cannot see the reads' lengths without a synchronisation, and building the table costs a batch of short reads three small
 *      launches and a scan. With it: scratch of 24 bytes per segment (72 with rows; the run records 13 more: the place of a segment's
 *      first record, the length it hands to the record before, its seam flag) for at most num_reads + total_bases / S segments,
 *      sized from that bound without a synchronisation; the entries past the true count are empty and lie behind the last segment, so
 *      on reads shorter than S the last waves of the launch find nothing to do while the others carry all of it (150-base reads at
 *      S = 256: two fifths of the waves, 4.5 -> 6.3 ms) -- switch it on for long reads. Without it they are launch for launch what they were.
 *      Never segmented: sshash_streaming_best_run[_device] (a longest run is not additive), sshash_streaming_lookup[_device], and
 *      every call on a minimizer shard (num_shards > 1: a shard's run kernel follows a run through k-mers it does not own, which a look
 *      at a seam would miss) -- those keep their routes whatever is set here.
 *      sshash_get_read_segments: the setting (S with the default resolved, or SSHASH_SEGMENTS_OFF), device_calls, and how many
 *      launches of the run kernel over a segment table the dictionary has made so far; each pointer may be NULL. ---- */
#define SSHASH_SEGMENTS_OFF UINT64_MAX
sshash_status sshash_set_read_segments(sshash_dict* d, uint64_t kmers_per_segment, int device_calls);
sshash_status sshash_get_read_segments(const sshash_dict* d, uint64_t* kmers_per_segment, int* device_calls, uint64_t* segmented_launches);

/* ---- the streaming query PER READ (no reference counterpart as a call; the reference's state machine is reset at every read,
 *      src/query.cpp:78-108, so the report it would give for read r alone is well defined). Rows are sshash_streaming_report
 *      structs, one per read, row r for read r of the call; the six counters of sshash_streaming_query over the same reads are the
 *      column sums of the rows. A read shorter than k (an empty one included) has a row of six zeros. Same preconditions and status
 *      codes as the calls above; per_read == NULL with num_reads > 0 is SSHASH_ERR_ARGUMENT, num_reads == 0 writes nothing. ---- */
/* device buffers, asynchronous on hip_stream. per_read: num_reads rows, OVERWRITTEN (every row is written). report: 6 uint64
 * counters, ACCUMULATED into as sshash_streaming_query_device does; may be NULL. total_bases as for sshash_streaming_query_device.
 * Like that call it always takes the run kernel -- one lane walks one read, whatever its length, unless sshash_set_read_segments has
 * switched segments on for the device calls: then one lane walks one segment, and a read of megabases costs what its bases cost. */
sshash_status sshash_streaming_query_per_read_device(const sshash_dict* d, int device, const char* bases,
                                                     const uint64_t* read_offsets, uint64_t num_reads, uint64_t total_bases,
                                                     sshash_streaming_report* per_read, uint64_t* report, void* hip_stream);
/* host buffers; sharded over all resident replicas like sshash_streaming_query (a piece that holds a long read takes the run kernel
 * over segments -- sshash_set_read_segments; with segments off, above 2^16 bases, the position-parallel pipeline of
 * sshash_streaming_lookup --, which gives the same rows); report may be NULL */
sshash_status sshash_streaming_query_per_read(const sshash_dict* d, const char* bases, const uint64_t* read_offsets,
                                              uint64_t num_reads, sshash_streaming_report* per_read,
                                              sshash_streaming_report* report);
/* a query file: rows are handed over in batches, IN FILE ORDER, one call at a time (never concurrently): rows[0 .. n) belong to
 * records first_read .. first_read + n of the file. There is a row for EVERY record of the file, those shorter than k included (six
 * zeros), so that row i is record i: a FASTQ read, a single-line FASTA record (header line + one sequence line), or -- multiline -- a
 * non-empty segment of a multiline FASTA (the lines up to an empty line or the end of the file, which is what the reader treats as one
 * read). A non-zero return of `fn` stops the query: the call returns SSHASH_ERR_ARGUMENT, sshash_last_error() carries the value and
 * `fn` is not called again. report may be NULL. Every kind of file, a plain FASTQ included, takes the sequential reader here (a
 * reader thread ahead of the devices, as described for sshash_streaming_query_from_file): host memory stays bounded, and the call
 * runs at that reader's pace. */
typedef int (*sshash_per_read_fn)(void* ctx, uint64_t first_read, uint64_t n, const sshash_streaming_report* rows);
sshash_status sshash_streaming_query_from_file_per_read(const sshash_dict* d, const char* filename, int multiline,
                                                        sshash_per_read_fn fn, void* ctx, sshash_streaming_report* report);

/* ---- WHERE a read hits: the maximal runs of the streaming query (no reference counterpart as a call; it is the reference's state
 *      machine, include/streaming_query.hpp:56-109, written down). Every positive k-mer of a read is a search or an extension; a RUN
 *      is one search together with the extensions that follow it directly. Equivalently, on the per-k-mer results of the read: a
 *      positive k-mer continues the run of the k-mer before it iff that k-mer is positive, lies in the same string and
 *      kmer_id == previous kmer_id + previous orientation; otherwise it starts a run. Invalid and negative k-mers belong to no run.
 *      So, per read, the number of runs is num_searches and the sum of the runs' lengths num_positive_kmers of the read's row of
 *      sshash_streaming_query_per_read, and the runs give back the result of every positive k-mer exactly:
 *      k-mer j of a run (j = 0 .. n-1) starts at base read_pos + j of the read and has kmer_id +/- j, kmer_id_in_string +/- j
 *      (+ forward, - backward), the run's string_id and orientation -- the streaming_query::lookup results of those k-mers.
 *      Output layout: CSR. run_offsets[num_reads + 1], run_offsets[0] = 0; the runs of read r are records run_offsets[r] ..
 *      run_offsets[r+1], in increasing read_pos. The layout is canonical: two calls over the same reads give byte-identical
 *      run_offsets and records. A read shorter than k, an empty read and a read without a hit have an empty range.
 *      Preconditions and status codes as the per-read calls: a null dictionary / bases / read_offsets / run_offsets with
 *      num_reads > 0, or runs == NULL with runs_capacity > 0, is SSHASH_ERR_ARGUMENT before anything runs; num_reads == 0 succeeds
 *      and writes run_offsets[0] = 0 if run_offsets is not NULL. ---- */
typedef struct sshash_streaming_run {
    uint64_t kmer_id;            /* lookup_result::kmer_id of the run's FIRST k-mer in read order */
    uint64_t string_id;          /* the string all k-mers of the run lie in */
    uint64_t kmer_id_in_string;  /* lookup_result::kmer_id_in_string of that first k-mer */
    uint32_t read_pos;           /* base of the read (0-based, relative to the read's start) where that k-mer starts */
    uint32_t num_kmers;          /* bits 0..30: k-mers in the run (>= 1); bit 31: set = orientation backward (-1) */
} sshash_streaming_run;
#define SSHASH_RUN_BACKWARD 0x80000000u
/* device buffers, asynchronous on hip_stream. run_offsets: num_reads + 1 words, OVERWRITTEN, always complete and exact whatever the
 * capacity. runs: room for runs_capacity records; record i is written iff i < runs_capacity, nothing at or beyond
 * runs + runs_capacity is touched; runs == NULL with runs_capacity == 0 is the counting call. The caller sees whether everything
 * fitted from run_offsets[num_reads] <= runs_capacity (no status for it: the call only enqueues). report: 6 uint64 counters,
 * ACCUMULATED into as sshash_streaming_query_device does; may be NULL. total_bases as for sshash_streaming_query_device.
 * PRECONDITION: every read is shorter than 2^31 bases -- read_pos and the length in num_kmers are 31 bits wide, and this call, which
 * only enqueues, does not look at the reads' lengths (the host call below does and refuses); a longer read gets wrapped fields. Always the
 * run kernel, as sshash_streaming_query_per_read_device: a counting launch (the runs of every read), a prefix sum, and -- with
 * runs_capacity > 0 -- a second launch that writes the records; scratch beyond that of sshash_streaming_query_device: 8 bytes per
 * 4096 reads. One lane walks one read, whatever its length, unless sshash_set_read_segments has switched segments on for the device
 * calls: then one lane walks one segment -- the counting launch counts per segment, a pass over the seams tells which segments begin
 * inside a run, the prefix sum gives every record that STARTS in a segment its final place, the writing launch stores those, and one
 * 32-bit add per joined seam gives a run that goes on over it its whole length. run_offsets and every record are byte for byte those
 * of the uncut call, at every capacity. */
sshash_status sshash_streaming_runs_device(const sshash_dict* d, int device, const char* bases, const uint64_t* read_offsets,
                                           uint64_t num_reads, uint64_t total_bases, uint64_t* run_offsets,
                                           sshash_streaming_run* runs, uint64_t runs_capacity, uint64_t* report, void* hip_stream);
/* host buffers, sharded over all resident replicas like sshash_streaming_query_per_read (a piece that holds a read above 2^16 bases
 * takes the run kernel over segments -- sshash_set_read_segments, both the counting and the writing pass; with segments off it goes
 * through the position-parallel pipeline of sshash_streaming_lookup and a compaction behind it --, which gives the same
 * records); same capacity rule; report may be NULL. A read of 2^31 bases or more is SSHASH_ERR_ARGUMENT (read_pos / num_kmers could
 * not hold it). */
sshash_status sshash_streaming_runs(const sshash_dict* d, const char* bases, const uint64_t* read_offsets, uint64_t num_reads,
                                    uint64_t* run_offsets, sshash_streaming_run* runs, uint64_t runs_capacity,
                                    sshash_streaming_report* report);
/* a query file -- a multiline FASTA of contigs mapped onto the unitigs without loading it first: the runs are handed over in batches, IN
 * FILE ORDER, one call of `fn` at a time, as the rows of sshash_streaming_query_from_file_per_read are. run_offsets (n + 1 words,
 * run_offsets[0] = 0) is LOCAL TO THE BATCH: the runs of record first_read + i of the file are runs[run_offsets[i] ..
 * run_offsets[i + 1]). There is an entry for EVERY record of the file; one shorter than k has an empty range. Both arrays are the
 * library's and valid during the call of `fn` only. A non-zero return of `fn` stops the query: the call returns SSHASH_ERR_ARGUMENT,
 * sshash_last_error() carries the value and `fn` is not called again. report may be NULL. A NULL dictionary, filename or fn is
 * SSHASH_ERR_ARGUMENT before anything runs; a record of 2^31 bases or more is SSHASH_ERR_ARGUMENT. Every kind of file takes the
 * sequential reader: host memory stays bounded by a batch and its runs. Batches go through the route of sshash_streaming_runs -- long
 * records over segments once sshash_set_read_segments has set an S --, counted once. */
typedef int (*sshash_read_runs_fn)(void* ctx, uint64_t first_read, uint64_t n,
                                   const uint64_t* run_offsets /* n + 1 words, [0] = 0, local to the batch */,
                                   const sshash_streaming_run* runs);
sshash_status sshash_streaming_runs_from_file(const sshash_dict* d, const char* filename, int multiline,
                                              sshash_read_runs_fn fn, void* ctx, sshash_streaming_report* report);

/* ---- WHICH k-mers of the dictionary a read set holds: the streaming query seen from the dictionary's side (no reference counterpart
 *      as a call). A COVER is a bitmap over the k-mer ids: ceil(num_kmers / 64) words of 64 bits (sshash_cover_words); k-mer id i is bit
 *      i & 63 of word i >> 6 (bit 0 = the least significant); the bits of the last word at or above num_kmers are never set by these
 *      calls. After a call the bitmap holds, besides what it held before, exactly the set of kmer_id values other than
 *      SSHASH_INVALID_U64 that sshash_streaming_lookup returns over the same reads -- every positive k-mer of every read, whatever its
 *      strand. The calls OR into the bitmap (a sample of many batches, or of several files, marks one bitmap; the caller zeroes it
 *      first), so the result does not depend on the order of the reads, of the batches or of the calls.
 *      Preconditions and status codes as the runs calls: a null dictionary, or null bases / read_offsets / cover with num_reads > 0,
 *      is SSHASH_ERR_ARGUMENT before anything runs; num_reads == 0 succeeds and touches nothing; a dictionary that is not resident
 *      is SSHASH_ERR_NO_DEVICE. A minimizer shard (num_shards > 1) behaves as with sshash_streaming_runs: it finds the k-mers it owns
 *      and no others, under the ids of the whole index (strings stay complete), so it marks its share of the cover and the shards'
 *      bitmaps ORed together are the cover of the whole index. ---- */
sshash_status sshash_cover_words(const sshash_dict* d, uint64_t* words);
/* device buffers, asynchronous on hip_stream. cover: sshash_cover_words words, ACCUMULATED into (OR); nothing at or beyond them is
 * touched. report: 6 uint64 counters, ACCUMULATED into as sshash_streaming_query_device does -- the same six counters --; may be
 * NULL. total_bases as for sshash_streaming_query_device. Always the run kernel (one lane walks one read, whatever its length, or
 * one segment: sshash_set_read_segments -- the bits are the same, OR is idempotent), in ONE launch: where sshash_streaming_runs_device writes a run's record this call ORs the run's id range into the bitmap, one 64-bit
 * atomic for the first and for the last word it touches; no scratch beyond that of sshash_streaming_query_device. */
sshash_status sshash_streaming_cover_device(const sshash_dict* d, int device, const char* bases, const uint64_t* read_offsets,
                                            uint64_t num_reads, uint64_t total_bases, uint64_t* cover, uint64_t* report, void* hip_stream);
/* host buffers, sharded over all resident replicas like sshash_streaming_query: every replica marks a bitmap of its own in HBM (8
 * bytes per 64 k-mers, for the length of the call) and those are ORed into `cover` (host, sshash_cover_words words) at the end. A piece
 * that holds a long read takes the run kernel over segments (sshash_set_read_segments; with segments off, above 2^16 bases, the
 * position-parallel pipeline of sshash_streaming_lookup, marked from its per-k-mer ids), which gives the same bits. report may be NULL. */
sshash_status sshash_streaming_cover(const sshash_dict* d, const char* bases, const uint64_t* read_offsets, uint64_t num_reads,
                                     uint64_t* cover, sshash_streaming_report* report);
/* a query file (.fa/.fasta/.fq/.fastq, optionally .gz; `multiline` as for sshash_streaming_query_from_file): every replica keeps ONE
 * bitmap in HBM for the whole file, and they are ORed into `cover` (host) once, at the end. Every kind of file takes the sequential
 * reader (a reader thread a batch ahead of the devices): host memory stays bounded whatever the size of the file, and the call runs
 * at that reader's pace. report may be NULL. */
sshash_status sshash_streaming_cover_from_file(const sshash_dict* d, const char* filename, int multiline, uint64_t* cover,
                                               sshash_streaming_report* report);
/* Covered k-mers per string: counts[s] = the set bits of `cover` among the k-mer ids of string s, [string_offsets(s).begin - s*(k-1),
 * string_offsets(s).end - (s+1)*(k-1)) -- at most sshash_string_size(s) --; counts: num_strings uint64, OVERWRITTEN; total (may be
 * NULL): one uint64, overwritten with their sum, the number of covered k-mers. Bits at or above num_kmers are not counted. NULL
 * dictionary, cover or counts: SSHASH_ERR_ARGUMENT. The device variant (device pointers, asynchronous on hip_stream) goes over the
 * bitmap's words, one lane a word; the host variant is plain CPU code and needs no GPU. */
sshash_status sshash_cover_string_counts_device(const sshash_dict* d, int device, const uint64_t* cover, uint64_t* counts,
                                                uint64_t* total, void* hip_stream);
sshash_status sshash_cover_string_counts(const sshash_dict* d, const uint64_t* cover, uint64_t* counts, uint64_t* total);

/* ---- HOW OFTEN a read set holds each k-mer of the dictionary: k-mer counting restricted to the dictionary (no reference counterpart as a
 *      call; what `ab:Z:` abundances of a weighted build are made from). A DEPTH ARRAY holds num_kmers words of uint32_t, word i for
 *      k-mer id i. After a call depth[i] has grown by the number of places in the reads where sshash_streaming_lookup over the same reads
 *      returns kmer_id == i: every strand counts, every occurrence counts. All arithmetic is modulo 2^32: a result is exact when the true
 *      count is below 2^32, whatever the intermediate values were; a k-mer held 2^32 times or more WRAPS (nothing saturates).
 *      The device side works on a DELTA ARRAY of the same size and type, a difference array: a maximal run of consecutive ids [lo, hi)
 *      adds 1 to delta[lo] and, if hi < num_kmers, subtracts 1 from delta[hi], whatever its length; depth[i] = delta[0] + .. + delta[i]
 *      (sshash_depth_finish_device). Deltas of many calls add up -- one array takes a sample of many batches or files --, and the
 *      order of the reads, of the batches and of the calls does not matter.
 *      Preconditions and status codes as the cover calls: a null dictionary, or null bases / read_offsets / output with num_reads > 0,
 *      is SSHASH_ERR_ARGUMENT before anything runs; num_reads == 0 succeeds and touches nothing; a dictionary that is not resident is
 *      SSHASH_ERR_NO_DEVICE. A minimizer shard (num_shards > 1) counts the k-mers it owns and no others, under the ids of the whole
 *      index, and the shards' depth arrays added together are the depth array of the whole index. For that a shard's host and file
 *      calls look every k-mer up on its own (the pipeline of sshash_streaming_lookup, whatever the reads' lengths): the run kernel
 *      measures a run along the string, which a shard holds whole, so it would follow a k-mer of its own through k-mers of other
 *      shards and those would be counted once per shard. sshash_streaming_depth_device, which is that kernel, is SSHASH_ERR_ARGUMENT
 *      on a minimizer shard. ---- */
/* device buffers, asynchronous on hip_stream. deltas: num_kmers uint32, ACCUMULATED into (the caller zeroes it before the first call);
 * nothing at or beyond deltas + num_kmers is touched. report and total_bases as for sshash_streaming_cover_device. Always the run kernel,
 * in ONE launch: where sshash_streaming_cover_device ORs a run's id range into the bitmap this call issues one or two 32-bit atomic
 * adds; no scratch beyond that of sshash_streaming_query_device. Over segments (sshash_set_read_segments) a run that spans a seam arrives
 * as two, [lo, mid) and [mid, hi): the +1 and the -1 at mid cancel, the deltas are those of [lo, hi). */
sshash_status sshash_streaming_depth_device(const sshash_dict* d, int device, const char* bases, const uint64_t* read_offsets,
                                            uint64_t num_reads, uint64_t total_bases, uint32_t* deltas, uint64_t* report, void* hip_stream);
/* deltas -> depths: depth[i] = deltas[0] + .. + deltas[i] modulo 2^32 over the num_kmers words (device pointers, asynchronous on
 * hip_stream; three launches, none of which waits for another workgroup). depth == deltas (in place) is allowed; any other overlap is the
 * caller's error. The scratch for the tile sums (4 bytes per 4096 k-mers) is sized, allocated and freed by the call itself, stream-ordered
 * on hip_stream, out of the replica's own memory pool. NULL dictionary, deltas or depth: SSHASH_ERR_ARGUMENT. */
sshash_status sshash_depth_finish_device(const sshash_dict* d, int device, const uint32_t* deltas, uint32_t* depth, void* hip_stream);
/* host buffers, sharded over all resident replicas like sshash_streaming_cover: every replica keeps one delta array in HBM (4 bytes per
 * k-mer, zeroed, for the length of the call), finishes it on the device, and the results are ADDED into `depth` (host, num_kmers uint32;
 * the caller zeroes it for a fresh count). A piece that holds a long read takes the run kernel over segments (sshash_set_read_segments;
 * with segments off, above 2^16 bases, the position-parallel pipeline of sshash_streaming_lookup, marked from its per-k-mer ids), which
 * gives the same depths. report may be NULL. */
sshash_status sshash_streaming_depth(const sshash_dict* d, const char* bases, const uint64_t* read_offsets, uint64_t num_reads,
                                     uint32_t* depth, sshash_streaming_report* report);
/* a query file, as sshash_streaming_cover_from_file (the sequential reader, bounded host memory): every replica keeps ONE delta array in
 * HBM for the whole file; they are finished and added into `depth` (host) once, at the end. report may be NULL. */
sshash_status sshash_streaming_depth_from_file(const sshash_dict* d, const char* filename, int multiline, uint32_t* depth,
                                               sshash_streaming_report* report);
/* Depth per string: sums[s] = the 64-bit sum of `depth` over the k-mer ids of string s (the id range of sshash_cover_string_counts);
 * sums: num_strings uint64, OVERWRITTEN; total (may be NULL): one uint64, overwritten with their sum. The mean depth of string s is
 * sums[s] / sshash_string_size(s). NULL dictionary, depth or sums: SSHASH_ERR_ARGUMENT. The device variant (device pointers,
 * asynchronous on hip_stream) goes over the ids, one lane each; the host variant is plain CPU code and needs no GPU. */
sshash_status sshash_depth_string_sums_device(const sshash_dict* d, int device, const uint32_t* depth, uint64_t* sums, uint64_t* total,
                                              void* hip_stream);
sshash_status sshash_depth_string_sums(const sshash_dict* d, const uint32_t* depth, uint64_t* sums, uint64_t* total);

/* ---- SCORING reads against a value per k-mer: per read, the sum of values[id] over the read's positive k-mers, and their number (no
 *      reference counterpart as a call). `values` holds num_kmers words of uint32_t, word i for k-mer id i: a depth array
 *      (sshash_streaming_depth), the weights of a weighted build expanded per id, or anything else. Row r of the output belongs to
 *      read r of the call:
 *          sums[r].sum            = the sum of value(id) over every place of read r where sshash_streaming_lookup returns a k-mer id,
 *          sums[r].positive_kmers = the number of those places (num_positive_kmers of the read's row of sshash_streaming_query_per_read);
 *      every strand counts, every occurrence counts. sum / positive_kmers is the mean value over the read's hits. A read shorter than
 *      k, an empty read and a read without a hit have the row {0, 0}. Rows are OVERWRITTEN, every one of them. All arithmetic is modulo
 *      2^64 (num_kmers values below 2^32 cannot reach it in a prefix; a read of 2^32 k-mers of value 2^32 - 1 could in a sum).
 *      The device side works on the 64-bit exclusive PREFIX SUMS P of the values, num_kmers + 1 words: a maximal run of consecutive ids
 *      [lo, hi) is worth P[hi] - P[lo], two 8-byte reads whatever its length. With at_least >= 1 the prefix counts instead of summing
 *      -- value(id) = 1 if values[id] >= at_least, else 0 --, so that `sum` is the number of the read's SOLID k-mers (depth >= t).
 *      A row is 16 bytes; 8-byte alignment is all that is asked of `sums`.
 *      Preconditions and status codes as the depth calls: a null dictionary, or null bases / read_offsets / prefix (values) / sums with
 *      num_reads > 0, is SSHASH_ERR_ARGUMENT before anything runs; num_reads == 0 succeeds and touches nothing; a dictionary that is not
 *      resident is SSHASH_ERR_NO_DEVICE. A minimizer shard (num_shards > 1) adds the k-mers it owns and no others, so the shards' rows
 *      added together are the rows of the whole index; for that a shard's host and file calls look every k-mer up on its own (the
 *      pipeline of sshash_streaming_lookup), and sshash_streaming_sums_device, which is the run kernel, is SSHASH_ERR_ARGUMENT on a
 *      minimizer shard -- as sshash_streaming_depth_device and for its reason.
 *      Segments (sshash_set_read_segments): the host and file calls segment a piece that holds a read of more than S k-mers, the device
 *      call with device_calls != 0; many lanes then add into one row, and the rows are word for word what the uncut reads give. ---- */
typedef struct sshash_read_sum {
    uint64_t sum;            /* of value(kmer_id) over the read's positive k-mers, modulo 2^64 */
    uint64_t positive_kmers; /* how many those are */
} sshash_read_sum;
/* values -> prefix (device pointers, asynchronous on hip_stream): prefix[0] = 0, prefix[i] = values[0] + .. + values[i - 1] -- at_least
 * >= 1: the number of j < i with values[j] >= at_least --, prefix[num_kmers] the total; num_kmers + 1 uint64, OVERWRITTEN; values is
 * only read. One widening launch and a three-launch 64-bit scan in place; the scratch for the tile sums (8 bytes per 4096 k-mers) is
 * sized, allocated and freed by the call itself, stream-ordered on hip_stream, out of the replica's own memory pool. NULL dictionary,
 * values or prefix: SSHASH_ERR_ARGUMENT. */
sshash_status sshash_value_prefix_device(const sshash_dict* d, int device, const uint32_t* values, uint32_t at_least, uint64_t* prefix,
                                         void* hip_stream);
/* device buffers, asynchronous on hip_stream. prefix: num_kmers + 1 uint64 from sshash_value_prefix_device, only read. sums: num_reads
 * rows, OVERWRITTEN; nothing outside sums[0 .. num_reads) is written. report and total_bases as for sshash_streaming_depth_device.
 * Always the run kernel: the rows are zeroed (one memset) and ONE launch adds every run's P[hi] - P[lo] and its length to its read's
 * row, two 64-bit atomic adds that nothing waits for; no scratch beyond that of sshash_streaming_query_device. */
sshash_status sshash_streaming_sums_device(const sshash_dict* d, int device, const char* bases, const uint64_t* read_offsets,
                                           uint64_t num_reads, uint64_t total_bases, const uint64_t* prefix, sshash_read_sum* sums,
                                           uint64_t* report, void* hip_stream);
/* host buffers, sharded over all resident replicas like sshash_streaming_depth. values: host, num_kmers uint32, uploaded once per call to
 * every resident replica, which builds the prefix and frees the 4-byte copy again: 8 bytes per k-mer (+ 8) stay in the HBM of every
 * replica for the length of the call, 12 per k-mer at the peak. A piece that holds a read above 2^16 bases, with segments off, goes
 * through the position-parallel pipeline of sshash_streaming_lookup and is summed from its per-k-mer ids, which gives the same rows.
 * report may be NULL. */
sshash_status sshash_streaming_sums(const sshash_dict* d, const char* bases, const uint64_t* read_offsets, uint64_t num_reads,
                                    const uint32_t* values, uint32_t at_least, sshash_read_sum* sums, sshash_streaming_report* report);
/* a query file: the contract of sshash_streaming_query_from_file_per_read -- rows are handed over in batches, IN FILE ORDER, one row for
 * EVERY record of the file, one call of `fn` at a time; a non-zero return of `fn` stops the query (SSHASH_ERR_ARGUMENT,
 * sshash_last_error() carries the value). The prefix is built once and stays in the HBM of every replica (8 bytes per k-mer) for the
 * whole file. report may be NULL. */
typedef int (*sshash_read_sums_fn)(void* ctx, uint64_t first_read, uint64_t n, const sshash_read_sum* sums);
sshash_status sshash_streaming_sums_from_file(const sshash_dict* d, const char* filename, int multiline, const uint32_t* values,
                                              uint32_t at_least, sshash_read_sums_fn fn, void* ctx, sshash_streaming_report* report);

/* ---- CLASSES: per read, its positive k-mers by class of string -- WHOSE a read's hits are (no reference counterpart as a call). `labels`
 *      holds num_strings words of uint32_t, word s the class of string s (sshash_lookup_result.string_id): a reference genome, a taxon, a
 *      colour-set id, host / target / contaminant, plasmid / chromosome. With C = num_classes, 1 <= C <= SSHASH_MAX_CLASSES, the output is
 *      num_reads x C words of uint32_t, row-major:
 *          rows[r * C + c] = the number of places of read r where sshash_streaming_lookup returns a k-mer whose string_id s has
 *                            labels[s] == c;
 *      every strand counts, every occurrence counts. A label >= C means "no class": its k-mers are positive in the report and counted in
 *      no column, which doubles as a mask. A read shorter than k, an empty read and a read without a hit have a row of zeros. Rows are
 *      OVERWRITTEN, every one of them; nothing outside rows[0 .. num_reads * C) is written. All arithmetic is modulo 2^32. 4-byte
 *      alignment is all that is asked of `rows`. Above SSHASH_MAX_CLASSES a dense row is the wrong shape: sshash_streaming_runs stays
 *      the route.
 *      Preconditions and status codes as the sums calls: a null dictionary, or null bases / read_offsets / labels / rows with
 *      num_reads > 0, is SSHASH_ERR_ARGUMENT, and so is num_classes == 0 or above SSHASH_MAX_CLASSES, all before anything runs;
 *      num_reads == 0 succeeds and touches nothing; a dictionary that is not resident is SSHASH_ERR_NO_DEVICE. A minimizer shard
 *      (num_shards > 1) counts the k-mers it owns and no others, so the shards' rows added together are the rows of the whole index;
 *      for that a shard's host and file calls look every k-mer up on its own (the pipeline of sshash_streaming_lookup), and
 *      sshash_streaming_classes_device, which is the run kernel, is SSHASH_ERR_ARGUMENT on a minimizer shard -- as
 *      sshash_streaming_sums_device and for its reason.
 *      Segments (sshash_set_read_segments): as the sums calls; many lanes then add into one row, and the rows are word for word what the
 *      uncut reads give. ---- */
#define SSHASH_MAX_CLASSES 4096u
/* device buffers, asynchronous on hip_stream. labels: num_strings uint32, only read. rows: num_reads * num_classes uint32, OVERWRITTEN.
 * report and total_bases as for sshash_streaming_depth_device. Always the run kernel: the rows are zeroed (one memset) and ONE launch
 * adds every run's length to the column of its string's label in its read's row -- a run lies in one string: one 4-byte load and one
 * 32-bit atomic add that nothing waits for, whatever the run's length; no scratch beyond that of sshash_streaming_query_device. */
sshash_status sshash_streaming_classes_device(const sshash_dict* d, int device, const char* bases, const uint64_t* read_offsets,
                                              uint64_t num_reads, uint64_t total_bases, const uint32_t* labels, uint32_t num_classes,
                                              uint32_t* rows, uint64_t* report, void* hip_stream);
/* host buffers, sharded over all resident replicas like sshash_streaming_sums. labels: host, num_strings uint32, uploaded once per call to
 * every resident replica. A piece of the batch holds no more reads than make 64 MiB of rows (4096 reads at 4096 classes) and travels
 * through the lanes' pinned blocks. A piece that holds a read above 2^16 bases, with segments off, goes through the position-parallel
 * pipeline of sshash_streaming_lookup and is counted from its per-k-mer string ids, which gives the same rows. report may be NULL. */
sshash_status sshash_streaming_classes(const sshash_dict* d, const char* bases, const uint64_t* read_offsets, uint64_t num_reads,
                                       const uint32_t* labels, uint32_t num_classes, uint32_t* rows, sshash_streaming_report* report);
/* a query file: the contract of sshash_streaming_sums_from_file -- rows are handed over in batches, IN FILE ORDER, one row of num_classes
 * words for EVERY record of the file, one call of `fn` at a time; a non-zero return of `fn` stops the query (SSHASH_ERR_ARGUMENT,
 * sshash_last_error() carries the value). The labels stay in the HBM of every replica for the whole file. report may be NULL. */
typedef int (*sshash_read_classes_fn)(void* ctx, uint64_t first_read, uint64_t n, const uint32_t* rows);
sshash_status sshash_streaming_classes_from_file(const sshash_dict* d, const char* filename, int multiline, const uint32_t* labels,
                                                 uint32_t num_classes, sshash_read_classes_fn fn, void* ctx, sshash_streaming_report* report);

/* The finish of the rows. BEST: one sshash_read_class per read -- the class with the largest count (among equals the smallest class), that
 * count, the largest count among the OTHER classes (equal to `best` on a tie), and the row's sum modulo 2^32; a row of zeros gives
 * {SSHASH_NO_CLASS, 0, 0, 0}. TOTALS: totals[c] = the 64-bit sum of column c over the reads, num_classes uint64 -- the sample's profile
 * by class. Both OVERWRITE their output. The _device forms take device pointers and are asynchronous on hip_stream (best: a group of
 * min(64, the power of two at or above num_classes) lanes per read; totals: one 64-bit atomic per column and workgroup); the others are
 * plain host code over host arrays and need no dictionary. NULL rows or output with num_reads > 0 (totals: a NULL output always),
 * num_classes == 0 or above SSHASH_MAX_CLASSES: SSHASH_ERR_ARGUMENT. */
#define SSHASH_NO_CLASS 0xFFFFFFFFu
typedef struct sshash_read_class {
    uint32_t best_class; /* SSHASH_NO_CLASS: the row is all zeros */
    uint32_t best;
    uint32_t second;
    uint32_t total;
} sshash_read_class;
sshash_status sshash_class_best_device(const sshash_dict* d, int device, const uint32_t* rows, uint64_t num_reads, uint32_t num_classes,
                                       sshash_read_class* best, void* hip_stream);
sshash_status sshash_class_best(const uint32_t* rows, uint64_t num_reads, uint32_t num_classes, sshash_read_class* best);
sshash_status sshash_class_totals_device(const sshash_dict* d, int device, const uint32_t* rows, uint64_t num_reads, uint32_t num_classes,
                                         uint64_t* totals, void* hip_stream);
sshash_status sshash_class_totals(const uint32_t* rows, uint64_t num_reads, uint32_t num_classes, uint64_t* totals);

/* ---- ANCHORS: per read, its LONGEST RUN -- the one place of a read a mapper extends from, and the length of its longest exact match
 *      (no reference counterpart as a call). For read r, best[r] is a sshash_streaming_run, the 32-byte record of sshash_streaming_runs
 *      with the same field meanings: the record of read r with the largest num_kmers & 0x7FFFFFFF (bit 31, the strand, takes no part
 *      in the comparison); among equals the one with the smallest read_pos, that is, the first in read order. A read shorter than k, an
 *      empty read and a read without a hit get a record of 32 zero bytes: num_kmers == 0 is the sign, a real run has at least 1.
 *      Every record of best[0 .. num_reads) is OVERWRITTEN; nothing outside that range is written. Equivalently: best[r] is that
 *      argmax over runs[run_offsets[r] : run_offsets[r + 1]] of sshash_streaming_runs on the same reads -- sshash_runs_best below
 *      computes it from those --, but its size is known before the call and it takes one launch, not a count, a prefix sum and a
 *      second launch. The six counters are accumulated into `report` as sshash_streaming_cover_device does; report may be NULL.
 *      Preconditions and status codes: a null dictionary, or null bases / read_offsets / best with num_reads > 0, is
 *      SSHASH_ERR_ARGUMENT, and so is a null `fn`, all before anything runs and with nothing written; num_reads == 0 succeeds and
 *      touches nothing; a dictionary that is not resident is SSHASH_ERR_NO_DEVICE. Segments never apply, whatever
 *      sshash_set_read_segments says: a longest run is not additive over segments, so these calls do not cut a read and do not
 *      count as segmented launches. A minimizer shard (num_shards > 1) is SSHASH_ERR_ARGUMENT from the device, host and file calls:
 *      the run kernel of a shard follows a run through k-mers it does not own, and the shards' longest runs do not combine into the
 *      whole index's; sshash_streaming_runs on the whole index is the route. ---- */
/* device buffers, asynchronous on hip_stream. best: num_reads records, OVERWRITTEN (16-byte aligned, as the records of
 * sshash_streaming_runs_device). report and total_bases as for sshash_streaming_cover_device. PRECONDITION, that of
 * sshash_streaming_runs_device: every read is shorter than 2^31 bases. Always the run kernel: the records are zeroed (one memset) and
 * ONE launch follows in which the lane that owns a read keeps the length of the read's longest run so far in a register and stores a
 * run's record over the read's when the run is longer -- plain stores, no atomics, no scratch beyond that of
 * sshash_streaming_query_device. */
sshash_status sshash_streaming_best_run_device(const sshash_dict* d, int device, const char* bases, const uint64_t* read_offsets,
                                               uint64_t num_reads, uint64_t total_bases, sshash_streaming_run* best, uint64_t* report,
                                               void* hip_stream);
/* host buffers, sharded over all resident replicas like sshash_streaming_sums; a piece's records travel through the lanes' pinned blocks.
 * A piece that holds a read above 2^16 bases goes the way it goes in sshash_streaming_runs -- the position-parallel pipeline of
 * sshash_streaming_lookup and its compaction into run records -- and sshash_runs_best_device over those, which gives the same
 * records. A read of 2^31 bases or more is SSHASH_ERR_ARGUMENT. report may be NULL. */
sshash_status sshash_streaming_best_run(const sshash_dict* d, const char* bases, const uint64_t* read_offsets, uint64_t num_reads,
                                        sshash_streaming_run* best, sshash_streaming_report* report);
/* a query file: the contract of sshash_streaming_sums_from_file -- records are handed over in batches, IN FILE ORDER, one record for
 * EVERY record of the file, one call of `fn` at a time; a non-zero return of `fn` stops the query (SSHASH_ERR_ARGUMENT,
 * sshash_last_error() carries the value). report may be NULL. */
typedef int (*sshash_read_best_run_fn)(void* ctx, uint64_t first_read, uint64_t n, const sshash_streaming_run* best);
sshash_status sshash_streaming_best_run_from_file(const sshash_dict* d, const char* filename, int multiline, sshash_read_best_run_fn fn,
                                                  void* ctx, sshash_streaming_report* report);
/* The finish over a COMPLETE CSR of run records (run_offsets[num_reads] records are present): best[r] = the argmax above over
 * runs[run_offsets[r] : run_offsets[r + 1]], 32 zero bytes for an empty range; best is OVERWRITTEN. The _device form takes device
 * pointers and is asynchronous on hip_stream (one lane a record and one 64-bit atomic max per record into 8 bytes of stream-ordered
 * scratch per read, then one lane a read); the other is plain host code over host arrays and needs no dictionary. NULL run_offsets or
 * best with num_reads > 0, or NULL runs where run_offsets[num_reads] > 0 (host form; the device form cannot see it): SSHASH_ERR_ARGUMENT. */
sshash_status sshash_runs_best_device(const sshash_dict* d, int device, const uint64_t* run_offsets, const sshash_streaming_run* runs,
                                      uint64_t num_reads, sshash_streaming_run* best, void* hip_stream);
sshash_status sshash_runs_best(const uint64_t* run_offsets, const sshash_streaming_run* runs, uint64_t num_reads, sshash_streaming_run* best);

/* ---- streaming_query<Dict,canonical>::lookup for EVERY k-mer of every read (include/streaming_query.hpp:56-109),
 *      batched: what the reference returns k-mer by k-mer while it streams a read. Every non-NULL array of `out` has one
 *      entry per BASE of `bases` (total_bases = read_offsets[num_reads] entries): entry read_offsets[r] + j is the result
 *      of the k-mer starting at base j of read r; entries of places where no k-mer starts (the last k-1 bases of a
 *      read, reads shorter than k) are left untouched. A k-mer holding a character other than ACGTacgt gets the
 *      default result the reference returns after its reset() (every u64 field SSHASH_INVALID_U64, orientation +1).
 *      Results equal the point lookups' (the reference asserts exactly that, :107); minimizer_found is not produced
 *      (SSHASH_ERR_ARGUMENT if asked for). `report` (may be NULL; device variant: 6 uint64 counters, accumulated into)
 *      receives the same counters as sshash_streaming_query. ---- */
sshash_status sshash_streaming_lookup_device(const sshash_dict* d, int device, const char* bases, const uint64_t* read_offsets,
                                             uint64_t num_reads, uint64_t total_bases, const sshash_results* out, uint64_t* report,
                                             void* hip_stream);
sshash_status sshash_streaming_lookup(const sshash_dict* d, const char* bases, const uint64_t* read_offsets, uint64_t num_reads,
                                      const sshash_results* out, sshash_streaming_report* report);

/* ---- routing for a minimizer-sharded index: owner shard of the forward
 *      minimizer and of the reverse-complement minimizer of every query (equal for canonical
 *      dictionaries: the smaller-valued minimizer decides). Device pointers, asynchronous. ----------- */
sshash_status sshash_route_packed_device(const sshash_dict* d, int device, const uint64_t* kmers, uint64_t n,
                                         uint32_t num_shards, uint32_t* owner_forward, uint32_t* owner_reverse,
                                         void* hip_stream);

/* The same routing with the bucketing done on the device, two calls on one stream:
 *   1. send == slots == NULL: cursors[s] += number of messages for shard s (one message per query and distinct
 *      owner; `cursors`: num_shards device uint64, zeroed by the caller) -- the send counts of the all-to-all;
 *   2. cursors[s] = index of the first message of shard s (exclusive prefix sum of the counts): message t gets
 *      send[t*W .. t*W+W) = the packed k-mer and slots[t] = the index of its query. Messages of one shard are
 *      contiguous; their order inside the shard is unspecified. n < 2^32, num_shards <= 1024. The second call elects the
 *      owners again and advances the cursors as the first did: afterwards cursors[s] = index behind the last message of
 *      shard s. Words of `send` and `slots` behind the last message are not written.
 * Both calls: SSHASH_ERR_ARGUMENT, before anything is launched, for num_shards outside [1, 1024], n >= 2^32, or only one
 * of send / slots; n == 0 writes nothing.
 * sshash_route_combine_device: out[slots[t]] = replies[t] for every reply != UINT64_MAX (`out` pre-filled with
 * UINT64_MAX by the caller; a reply of UINT64_MAX writes nothing); owners that both find a k-mer return the same id. */
sshash_status sshash_route_bucket_device(const sshash_dict* d, int device, const uint64_t* kmers, uint64_t n,
                                         uint32_t num_shards, int check_reverse_complement, uint64_t* cursors,
                                         uint64_t* send, uint32_t* slots, void* hip_stream);
/* Bucketing for table shards (sshash_to_device_table_shard): the owner of a query is the owner of its table key --
 * strand-symmetric, so exactly ONE message per query. Same two-call protocol as above. */
sshash_status sshash_route_bucket_by_key_device(const sshash_dict* d, int device, const uint64_t* kmers, uint64_t n,
                                                uint32_t num_shards, uint64_t* cursors, uint64_t* send, uint32_t* slots,
                                                void* hip_stream);
sshash_status sshash_route_combine_device(const sshash_dict* d, int device, const uint64_t* replies, const uint32_t* slots,
                                          uint64_t m, uint64_t* out, void* hip_stream);

/* ---- the whole sharded lookup as ONE call (BASELINE.json configs[4]): route -> exchange -> lookup
 *      -> return -> combine against a dictionary partitioned over `num_ranks` GPUs -- minimizer shards
 *      (sshash_build_config.num_shards / shard_id; by_table_key = 0) or table shards (sshash_to_device_table_shard;
 *      by_table_key = 1). Collective: every rank calls it with its own local batch of n packed k-mers (n may be 0) and
 *      receives the n ids, identical to the unpartitioned dictionary's. The one step that needs communication is handed
 *      in as two callbacks (return 0 on success):
 *        counts  all-to-all of ONE uint64 per peer: send[p] goes to rank p, recv[p] comes from rank p (host arrays of
 *                num_ranks entries). The words are opaque to the callback: the library carries the length of its table keys in
 *                their top byte, so that ranks built under different SSHASH_AMD_SK_M refuse to work together (SSHASH_ERR_ARGUMENT
 *                on every rank, after this exchange and before the data exchange) -- in the same exchange on every call, so no rank
 *                ever runs a collective step its peers skip;
 *        data    all-to-all-v of DEVICE buffers: the block for rank p starts after the blocks of the ranks before it,
 *                send_counts[p] / recv_counts[p] elements of elem_bytes each (host arrays); it must be complete, or ordered
 *                on hip_stream, when it returns.
 *      sshash_sharded_lookup_rccl supplies them over an RCCL communicator (grouped ncclSend/ncclRecv: the all-to-all
 *      over xGMI); `nccl_comm` is an ncclComm_t whose rank r holds shard r. RCCL is resolved when first used.
 *      Like any collective, the call completes only if every rank makes it: a rank that fails before the exchange (an argument
 *      error, an allocation failure: it returns its status without having called `counts`) leaves its peers waiting in theirs --
 *      the host application's job control has to take the group down, as it would for a failed ncclAllReduce. ---- */
typedef struct sshash_exchange {
    void* ctx;
    int (*counts)(void* ctx, const uint64_t* send, uint64_t* recv);
    int (*data)(void* ctx, const void* send, const uint64_t* send_counts, void* recv, const uint64_t* recv_counts,
                uint32_t elem_bytes, void* hip_stream);
} sshash_exchange;
sshash_status sshash_sharded_lookup_device(const sshash_dict* d, int device, uint32_t num_ranks, int by_table_key,
                                           const uint64_t* kmers, uint64_t n, int check_reverse_complement, uint64_t* kmer_ids,
                                           const sshash_exchange* exchange, void* hip_stream);
sshash_status sshash_sharded_lookup_rccl(const sshash_dict* d, int device, void* nccl_comm, int by_table_key, const uint64_t* kmers,
                                         uint64_t n, int check_reverse_complement, uint64_t* kmer_ids, void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* SSHASH_AMD_H */
