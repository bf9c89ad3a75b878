// capi.cpp -- the C ABI declared in include/sshash_amd.h (thin shim over engine / index).
#include <condition_variable>
#include <cstdlib>
#include <chrono>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <thread>

#include "../../include/sshash_amd.h"
#include "engine.hpp"
#include "hooks.hpp"
#include "reads.hpp"

using namespace sshash_amd;

struct sshash_dict {
    std::shared_ptr<host_index> idx;
    std::unique_ptr<engine> eng;
};

namespace {

thread_local std::string g_last_error;

sshash_status fail(sshash_status s, std::string const& msg) {
    g_last_error = msg;
    return s;
}

sshash_status classify(std::exception const& e) {
    g_last_error = e.what();
    if (auto const* typed = dynamic_cast<error const*>(&e)) return sshash_status(int(typed->kind));
    return SSHASH_ERR_INTERNAL;
}

template <typename Fn>
sshash_status guarded(Fn&& fn) {
    try {
        test_hooks_refresh();  // (hooks.hpp: the environment is read here, on the caller's thread, never by the library's own threads)
        fn();
        return SSHASH_OK;
    } catch (std::exception const& e) { return classify(e); } catch (...) {
        return fail(SSHASH_ERR_INTERNAL, "unknown exception");
    }
}

build_options to_options(sshash_build_config const* cfg) {
    build_options o;
    if (cfg) {
        if (cfg->k) o.k = cfg->k;
        if (cfg->m) o.m = cfg->m;
        o.seed = cfg->seed;
        o.canonical = cfg->canonical != 0;
        o.num_threads = cfg->num_threads ? cfg->num_threads : std::max(1u, std::thread::hardware_concurrency());
        if (cfg->lambda > 0) o.lambda = cfg->lambda;
        o.verbose = cfg->verbose != 0;
        o.weighted = cfg->weighted != 0;
        o.num_shards = cfg->num_shards ? cfg->num_shards : 1;
        o.shard_id = cfg->shard_id;
    }
    return o;
}

sshash_dict* wrap(std::shared_ptr<host_index> idx) {
    auto* d = new sshash_dict;
    d->idx = std::move(idx);
    d->eng = std::make_unique<engine>(d->idx);
    return d;
}

result_view to_view(sshash_results const* r) {
    result_view v{};
    if (r) {
        v.kmer_id = r->kmer_id;
        v.kmer_id_in_string = r->kmer_id_in_string;
        v.kmer_offset = r->kmer_offset;
        v.string_id = r->string_id;
        v.string_begin = r->string_begin;
        v.string_end = r->string_end;
        v.kmer_orientation = r->kmer_orientation;
        v.minimizer_found = r->minimizer_found;
    }
    return v;
}

bool wants_full(sshash_results const* r) {  // any array besides kmer_id
    bool any = false;
    for_each_field([&](int f, auto* p, uint64_t) { any = any || (f > 0 && p); }, to_view(r));
    return any;
}

/* The optional report of a streaming call: zeroed when the call's arguments have passed (before anything can throw), filled with the
   counters so far by every fill() after that. */
struct report_out {
    sshash_streaming_report* const report;
    explicit report_out(sshash_streaming_report* r) : report(r) {
        if (report) std::memset(report, 0, sizeof(*report));
    }
    void fill(streaming_report const& r) const {
        if (!report) return;
        report->num_kmers = r.num_kmers;
        report->num_positive_kmers = r.num_positive_kmers;
        report->num_negative_kmers = r.num_negative_kmers;
        report->num_invalid_kmers = r.num_invalid_kmers;
        report->num_searches = r.num_searches;
        report->num_extensions = r.num_extensions;
    }
};

/* The query file of a file call, opened (it throws when it cannot be) and handed to `use(read_stream&)` -- every_record: the calls with a
   row per record want the reads shorter than k as well, row i is record i. An extension that is no supported format: the message of
   src/query.cpp:169-171 on stderr and `use` is not called; the call then returns with its zeroed report. */
template <typename Use>
void with_query_file(sshash_dict const* d, const char* filename, int multiline, bool every_record, Use&& use) {
    read_stream in(filename, multiline != 0, d->idx->k, every_record);
    if (!in.supported()) {
        fprintf(stderr, "unsupported query file format\n");
        return;
    }
    use(in);
}

/* The sequential reader of a query file, a batch ahead of whoever uses the batches: `per_batch(read_batch const&)` is called for one
   batch after the other, in file order, on the calling thread. */
template <typename Fn>
void for_each_batch(read_stream& in, Fn&& per_batch) {
    /* The file goes through in batches of ~256 MiB of bases (a FASTQ of hundreds of gigabytes must not be
       materialised): a reader thread decompresses batch i+1 while the devices work on batch i. */
    uint64_t batch_bases = uint64_t(256) << 20;
    batch_bases = test_hook_u64("query_batch_bases", batch_bases, 1, ~uint64_t(0));  // (tests: batch seams inside a small file)
    read_batch slot[2];
    std::mutex mu;
    std::condition_variable cv;
    int filled[2] = {0, 0};  // 0 = free, 1 = holds a batch, 2 = end of file
    std::exception_ptr reader_error;
    bool abandon = false;
    std::thread reader([&] {
        try {
            for (int at = 0;; at ^= 1) {
                {
                    std::unique_lock<std::mutex> lock(mu);
                    cv.wait(lock, [&] { return filled[at] == 0 || abandon; });
                    if (abandon) return;
                }
                const bool more = in.next(slot[at], batch_bases);
                std::lock_guard<std::mutex> lock(mu);
                filled[at] = more ? 1 : 2;
                cv.notify_all();
                if (!more) return;
            }
        } catch (...) {
            std::lock_guard<std::mutex> lock(mu);
            reader_error = std::current_exception();
            filled[0] = filled[1] = 2;
            cv.notify_all();
        }
    });
    struct joiner {
        std::thread& t;
        std::mutex& mu;
        std::condition_variable& cv;
        bool& abandon;
        ~joiner() {
            {
                std::lock_guard<std::mutex> lock(mu);
                abandon = true;
            }
            cv.notify_all();
            t.join();
        }
    } join_reader{reader, mu, cv, abandon};
    double waited = 0, worked = 0;  // SSHASH_AMD_VERBOSE: where the wall clock of the file query went
    uint64_t batches = 0;
    auto now = [] { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    for (int at = 0;; at ^= 1) {
        const double t0 = now();
        {
            std::unique_lock<std::mutex> lock(mu);
            cv.wait(lock, [&] { return filled[at] != 0; });
            if (filled[at] == 2) break;
        }
        const double t1 = now();
        per_batch(slot[at]);
        waited += t1 - t0;
        worked += now() - t1;
        ++batches;
        std::lock_guard<std::mutex> lock(mu);
        filled[at] = 0;
        cv.notify_all();
    }
    if (std::getenv("SSHASH_AMD_VERBOSE"))
        fprintf(stderr, "[sshash_amd] file query: %llu batches; waiting for the reader %.3f s, devices at work %.3f s\n",
                (unsigned long long)batches, waited, worked);
    if (reader_error) std::rethrow_exception(reader_error);
}

/* The file calls with a row per record: one batch of the file after the other through `per_batch(batch, rows)` -- the engine call, which
   fills `row_words` Rows per read and returns the batch's report -- and on to the caller's `fn`, in file order. The report is filled after
   every batch, before `fn` is called: a callback that stops the call leaves the totals so far. */
template <typename Row, typename Fn, typename PerBatch>
void rows_from_file(read_stream& in, uint64_t row_words, Fn fn, void* ctx, report_out const& rep, PerBatch&& per_batch) {
    streaming_report total;
    uint64_t first_read = 0;
    std::vector<Row> rows;
    for_each_batch(in, [&](read_batch const& batch) {
        const uint64_t n = batch.num_reads();
        if (n == 0) return;
        rows.resize(n * row_words);
        rep.fill(total += per_batch(batch, rows.data()));
        const int stop = fn(ctx, first_read, n, rows.data());
        if (stop) throw error(error_kind::argument, "the per-read callback returned " + std::to_string(stop));
        first_read += n;
    });
}

/* The file calls that accumulate over the whole file (cover, depth): a Holder on the devices from the first batch to the last -- every kind
   of file takes the sequential reader --, `per_batch(batch, holder)` the engine call, `into(holder)` the holder's own or_into / add_into
   once the batches are through. */
template <typename Holder, typename PerBatch, typename Into>
void accumulate_from_file(sshash_dict const* d, const char* filename, int multiline, report_out const& rep, PerBatch&& per_batch, Into&& into) {
    with_query_file(d, filename, multiline, false, [&](read_stream& in) {
        const Holder on_devices(*d->eng);
        streaming_report total;
        for_each_batch(in, [&](read_batch const& batch) { total += per_batch(batch, on_devices); });
        into(on_devices);
        rep.fill(total);
    });
}

}  // namespace

extern "C" {

const char* sshash_last_error(void) { return g_last_error.c_str(); }

const char* sshash_build_info(void) {
    static const std::string info = std::string("isa_guard=") + sshash_amd::isa_guard_state() + ";arch=gfx950";
    return info.c_str();
}

void sshash_build_config_default(sshash_build_config* cfg) {
    if (!cfg) return;
    std::memset(cfg, 0, sizeof(*cfg));
    cfg->k = 31;
    cfg->m = 20;
    cfg->seed = 1;
    cfg->num_threads = 1;
    cfg->lambda = 5.0;
    cfg->num_shards = 1;
}

sshash_status sshash_build_from_fasta(const char* filename, const sshash_build_config* cfg, sshash_dict** out) {
    if (!filename || !out) return fail(SSHASH_ERR_ARGUMENT, "null argument");
    *out = nullptr;
    return guarded([&] {
        auto idx = std::make_shared<host_index>();
        build_from_fasta(*idx, filename, to_options(cfg));
        *out = wrap(std::move(idx));
    });
}

sshash_status sshash_build_from_packed(const uint64_t* words, const uint64_t* endpoints, uint64_t num_strings,
                                       const sshash_build_config* cfg, sshash_dict** out) {
    if (!words || !endpoints || !out || num_strings == 0) return fail(SSHASH_ERR_ARGUMENT, "null argument");
    *out = nullptr;
    return guarded([&] {
        std::vector<uint64_t> e(endpoints, endpoints + num_strings + 1);
        std::vector<uint64_t> w(words, words + (2 * e.back() + 63) / 64);
        auto idx = std::make_shared<host_index>();
        build_from_packed(*idx, std::move(w), std::move(e), to_options(cfg));
        *out = wrap(std::move(idx));
    });
}

sshash_status sshash_save(const sshash_dict* d, const char* filename) {
    if (!d || !filename) return fail(SSHASH_ERR_ARGUMENT, "null argument");
    return guarded([&] { save_index(*d->idx, filename); });
}

sshash_status sshash_load(const char* filename, sshash_dict** out) {
    if (!filename || !out) return fail(SSHASH_ERR_ARGUMENT, "null argument");
    *out = nullptr;
    return guarded([&] {
        auto idx = std::make_shared<host_index>();
        load_index(*idx, filename);
        *out = wrap(std::move(idx));
    });
}

void sshash_free(sshash_dict* d) { delete d; }

sshash_status sshash_get_info(const sshash_dict* d, sshash_info* info) {
    if (!d || !info) return fail(SSHASH_ERR_ARGUMENT, "null argument");
    host_index const& x = *d->idx;
    std::memset(info, 0, sizeof(*info));
    std::memcpy(info->version, x.version, 3);
    info->canonical = x.canonical;
    info->k = x.k;
    info->m = x.m;
    info->words_per_kmer = x.words_per_kmer();
    info->num_kmers = x.num_kmers;
    info->num_strings = x.num_strings;
    info->num_bases = x.num_bases;
    info->num_minimizers = x.num_minimizers();
    info->num_bits = x.num_bits();
    info->skew_partitions = x.skew_num_partitions;
    info->weighted = x.weighted() ? 1 : 0;
    info->num_shards = x.num_shards;
    info->shard_id = x.shard_id;
    return SSHASH_OK;
}

sshash_status sshash_bucket_stats(const sshash_dict* d, uint64_t out[64]) {
    if (!d || !out) return fail(SSHASH_ERR_ARGUMENT, "null argument");
    return guarded([&] { bucket_statistics(*d->idx, out); });
}

int sshash_device_count(void) { return visible_device_count(); }

sshash_status sshash_to_device(sshash_dict* d, int device) {
    if (!d) return fail(SSHASH_ERR_ARGUMENT, "null argument");
    return guarded([&] { d->eng->to_device(device); });
}

sshash_status sshash_device_bytes(const sshash_dict* d, int device, uint64_t* bytes) {
    if (!d || !bytes) return fail(SSHASH_ERR_ARGUMENT, "null argument");
    return guarded([&] { *bytes = d->eng->device_bytes(device); });
}

sshash_status sshash_set_read_segments(sshash_dict* d, uint64_t kmers_per_segment, int device_calls) {
    if (!d) return fail(SSHASH_ERR_ARGUMENT, "null argument");
    return guarded([&] { d->eng->set_read_segments(kmers_per_segment, device_calls != 0); });
}

sshash_status sshash_get_read_segments(const sshash_dict* d, uint64_t* kmers_per_segment, int* device_calls, uint64_t* segmented_launches) {
    if (!d) return fail(SSHASH_ERR_ARGUMENT, "null argument");
    if (kmers_per_segment) *kmers_per_segment = d->eng->read_segment_kmers();
    if (device_calls) *device_calls = d->eng->read_segments_device_calls() ? 1 : 0;
    if (segmented_launches) *segmented_launches = d->eng->segmented_launches();
    return SSHASH_OK;
}

sshash_status sshash_device_stats(const sshash_dict* d, int device, uint64_t out[16]) {
    if (!d || !out) return fail(SSHASH_ERR_ARGUMENT, "null argument");
    return guarded([&] { d->eng->device_stats(device, out); });
}

sshash_status sshash_device_table_histogram(const sshash_dict* d, int device, uint64_t out[32]) {
    if (!d || !out) return fail(SSHASH_ERR_ARGUMENT, "null argument");
    return guarded([&] { d->eng->device_table_histogram(device, out); });
}

sshash_status sshash_device_table_export(const sshash_dict* d, int device, uint64_t info[8], void* out, uint64_t capacity_bytes) {
    if (!d || !info) return fail(SSHASH_ERR_ARGUMENT, "null argument");
    return guarded([&] { d->eng->device_table_export(device, info, out, capacity_bytes); });
}

sshash_status sshash_lookup_packed_device(const sshash_dict* d, int device, const uint64_t* kmers, uint64_t n,
                                          int check_rc, const sshash_results* out, void* hip_stream) {
    if (!d || !out || (!kmers && n)) return fail(SSHASH_ERR_ARGUMENT, "null argument");
    return guarded([&] {
        d->eng->lookup_packed_device(device, kmers, n, check_rc != 0, wants_full(out) ? out_mode::full : out_mode::ids,
                                     to_view(out), nullptr, hip_stream);
    });
}

sshash_status sshash_lookup_ascii_device(const sshash_dict* d, int device, const char* kmers, uint64_t n, int check_rc,
                                         const sshash_results* out, void* hip_stream) {
    if (!d || !out || (!kmers && n)) return fail(SSHASH_ERR_ARGUMENT, "null argument");
    return guarded([&] {
        d->eng->lookup_ascii_device(device, kmers, n, check_rc != 0, wants_full(out) ? out_mode::full : out_mode::ids,
                                    to_view(out), nullptr, hip_stream);
    });
}

sshash_status sshash_lookup_packed(const sshash_dict* d, const uint64_t* kmers, uint64_t n, int check_rc,
                                   const sshash_results* out) {
    if (!d || !out || (!kmers && n)) return fail(SSHASH_ERR_ARGUMENT, "null argument");
    return guarded([&] {
        d->eng->lookup_packed_host(kmers, n, check_rc != 0, wants_full(out) ? out_mode::full : out_mode::ids, to_view(out),
                                   nullptr);
    });
}

sshash_status sshash_lookup_ascii(const sshash_dict* d, const char* kmers, uint64_t n, int check_rc,
                                  const sshash_results* out) {
    if (!d || !out || (!kmers && n)) return fail(SSHASH_ERR_ARGUMENT, "null argument");
    return guarded([&] {
        d->eng->lookup_ascii_host(kmers, n, check_rc != 0, wants_full(out) ? out_mode::full : out_mode::ids, to_view(out),
                                  nullptr);
    });
}

sshash_status sshash_neighbours_packed_device(const sshash_dict* d, int device, const uint64_t* kmers, uint64_t n,
                                              int check_rc, const sshash_results* out, void* hip_stream) {
    if (!d || !out || (!kmers && n)) return fail(SSHASH_ERR_ARGUMENT, "null argument");
    return guarded([&] {
        d->eng->neighbours_packed_device(device, kmers, n, check_rc != 0, wants_full(out) ? out_mode::full : out_mode::ids,
                                         to_view(out), hip_stream);
    });
}

sshash_status sshash_neighbours_packed(const sshash_dict* d, const uint64_t* kmers, uint64_t n, int check_rc,
                                       const sshash_results* out) {
    if (!d || !out || (!kmers && n)) return fail(SSHASH_ERR_ARGUMENT, "null argument");
    return guarded([&] {
        d->eng->neighbours_packed_host(kmers, n, check_rc != 0, wants_full(out) ? out_mode::full : out_mode::ids, to_view(out));
    });
}

sshash_status sshash_string_size(const sshash_dict* d, const uint64_t* string_ids, uint64_t n, uint64_t* out_sizes) {
    if (!d || (n && (!string_ids || !out_sizes))) return fail(SSHASH_ERR_ARGUMENT, "null argument");
    return guarded([&] {
        host_index const& x = *d->idx;
        for (uint64_t i = 0; i < n; ++i) {
            if (string_ids[i] >= x.num_strings) throw error(error_kind::argument, "string_id out of range");
            out_sizes[i] = x.endpoints[string_ids[i] + 1] - x.endpoints[string_ids[i]] - x.k + 1;
        }
    });
}

sshash_status sshash_string_offsets(const sshash_dict* d, const uint64_t* string_ids, uint64_t n, uint64_t* out_begin, uint64_t* out_end) {
    if (!d || (n && (!string_ids || !out_begin || !out_end))) return fail(SSHASH_ERR_ARGUMENT, "null argument");
    return guarded([&] {
        host_index const& x = *d->idx;
        for (uint64_t i = 0; i < n; ++i) {
            if (string_ids[i] >= x.num_strings) throw error(error_kind::argument, "string_id out of range");
            out_begin[i] = x.endpoints[string_ids[i]];
            out_end[i] = x.endpoints[string_ids[i] + 1];
        }
    });
}

sshash_status sshash_string_neighbours(const sshash_dict* d, const uint64_t* string_ids, uint64_t n, int check_rc,
                                       const sshash_results* out) {
    if (!d || !out || (!string_ids && n)) return fail(SSHASH_ERR_ARGUMENT, "null argument");
    return guarded([&] {
        d->eng->string_neighbours_host(string_ids, n, check_rc != 0, wants_full(out) ? out_mode::full : out_mode::ids, to_view(out));
    });
}

sshash_status sshash_string_neighbours_device(const sshash_dict* d, int device, const uint64_t* string_ids, uint64_t first_string, uint64_t n,
                                              int check_rc, const sshash_results* out, void* hip_stream) {
    if (!d || !out) return fail(SSHASH_ERR_ARGUMENT, "null argument");
    return guarded([&] {
        d->eng->string_neighbours_device(device, string_ids, first_string, n, check_rc != 0, wants_full(out) ? out_mode::full : out_mode::ids,
                                         to_view(out), hip_stream);
    });
}

static_assert(sizeof(sshash_string_link) == 32, "a link record is 32 bytes: two 16-byte stores on the device");

sshash_status sshash_string_links_device(const sshash_dict* d, int device, uint64_t begin_string, uint64_t end_string, int check_rc,
                                         uint64_t* link_offsets, sshash_string_link* links, uint64_t links_capacity, void* hip_stream) {
    if (!d) return fail(SSHASH_ERR_ARGUMENT, "null argument");
    return guarded([&] { d->eng->string_links_device(device, begin_string, end_string, check_rc != 0, link_offsets, links, links_capacity, hip_stream); });
}

sshash_status sshash_string_links(const sshash_dict* d, uint64_t begin_string, uint64_t end_string, int check_rc, uint64_t* link_offsets,
                                  sshash_string_link* links, uint64_t links_capacity) {
    if (!d) return fail(SSHASH_ERR_ARGUMENT, "null argument");
    return guarded([&] { d->eng->string_links_host(begin_string, end_string, check_rc != 0, link_offsets, links, links_capacity); });
}

sshash_status sshash_kmer_adjacency_device(const sshash_dict* d, int device, uint64_t begin_kmer_id, uint64_t end_kmer_id, int check_rc,
                                           uint8_t* masks, void* hip_stream) {
    if (!d) return fail(SSHASH_ERR_ARGUMENT, "null argument");
    return guarded([&] { d->eng->kmer_adjacency_device(device, begin_kmer_id, end_kmer_id, check_rc != 0, masks, hip_stream); });
}

sshash_status sshash_kmer_adjacency(const sshash_dict* d, uint64_t begin_kmer_id, uint64_t end_kmer_id, int check_rc, uint8_t* masks) {
    if (!d) return fail(SSHASH_ERR_ARGUMENT, "null argument");
    return guarded([&] { d->eng->kmer_adjacency_host(begin_kmer_id, end_kmer_id, check_rc != 0, masks); });
}

sshash_status sshash_is_member_packed_device(const sshash_dict* d, int device, const uint64_t* kmers, uint64_t n,
                                             int check_rc, uint8_t* out, void* hip_stream) {
    if (!d || !out || (!kmers && n)) return fail(SSHASH_ERR_ARGUMENT, "null argument");
    return guarded([&] {
        d->eng->lookup_packed_device(device, kmers, n, check_rc != 0, out_mode::member, result_view{}, out, hip_stream);
    });
}

sshash_status sshash_is_member_packed(const sshash_dict* d, const uint64_t* kmers, uint64_t n, int check_rc, uint8_t* out) {
    if (!d || !out || (!kmers && n)) return fail(SSHASH_ERR_ARGUMENT, "null argument");
    return guarded([&] { d->eng->lookup_packed_host(kmers, n, check_rc != 0, out_mode::member, result_view{}, out); });
}

sshash_status sshash_is_member_ascii(const sshash_dict* d, const char* kmers, uint64_t n, int check_rc, uint8_t* out) {
    if (!d || !out || (!kmers && n)) return fail(SSHASH_ERR_ARGUMENT, "null argument");
    return guarded([&] { d->eng->lookup_ascii_host(kmers, n, check_rc != 0, out_mode::member, result_view{}, out); });
}

sshash_status sshash_weight(const sshash_dict* d, const uint64_t* kmer_ids, uint64_t n, uint64_t* out_weights) {
    if (!d || (n && (!kmer_ids || !out_weights))) return fail(SSHASH_ERR_ARGUMENT, "null argument");
    return guarded([&] {
        for (uint64_t i = 0; i < n; ++i) out_weights[i] = weight_of(*d->idx, kmer_ids[i]);
    });
}

sshash_status sshash_weight_device(const sshash_dict* d, int device, const uint64_t* kmer_ids, uint64_t n,
                                   uint64_t* out_weights, void* hip_stream) {
    if (!d || (n && (!kmer_ids || !out_weights))) return fail(SSHASH_ERR_ARGUMENT, "null argument");
    return guarded([&] { d->eng->weight_device(device, kmer_ids, n, out_weights, hip_stream); });
}

sshash_status sshash_access(const sshash_dict* d, uint64_t kmer_id, char* out_k_chars) {
    if (!d || !out_k_chars) return fail(SSHASH_ERR_ARGUMENT, "null argument");
    return guarded([&] { access_kmer(*d->idx, kmer_id, out_k_chars); });
}

sshash_status sshash_access_packed(const sshash_dict* d, const uint64_t* kmer_ids, uint64_t n, uint64_t* out_words) {
    if (!d || (!kmer_ids && n) || (!out_words && n)) return fail(SSHASH_ERR_ARGUMENT, "null argument");
    return guarded([&] {
        const uint32_t W = d->idx->words_per_kmer();
        const uint32_t nt = std::max(1u, std::min(32u, std::thread::hardware_concurrency()));
        /* an id >= num_kmers throws inside a worker: parallel_ranges hands the first exception back to this thread */
        detail::parallel_ranges(n, n >= 4096 ? nt : 1, [&](uint64_t b, uint64_t e, uint32_t) {
            for (uint64_t i = b; i < e; ++i) access_kmer_packed(*d->idx, kmer_ids[i], out_words + i * W);
        });
    });
}

sshash_status sshash_access_packed_device(const sshash_dict* d, int device, const uint64_t* kmer_ids, uint64_t n,
                                          uint64_t* out_words, void* hip_stream) {
    if (!d || (!kmer_ids && n) || (!out_words && n)) return fail(SSHASH_ERR_ARGUMENT, "null argument");
    return guarded([&] { d->eng->access_packed_device(device, kmer_ids, n, out_words, hip_stream); });
}

sshash_status sshash_iterate_packed(const sshash_dict* d, uint64_t begin_kmer_id, uint64_t end_kmer_id, uint64_t* out_words) {
    if (!d || (!out_words && end_kmer_id > begin_kmer_id)) return fail(SSHASH_ERR_ARGUMENT, "null argument");
    if (begin_kmer_id > end_kmer_id || end_kmer_id > d->idx->num_kmers)
        return fail(SSHASH_ERR_ARGUMENT, "iterate: need begin <= end <= num_kmers");
    return guarded([&] {
        const uint32_t W = d->idx->words_per_kmer();
        const uint64_t n = end_kmer_id - begin_kmer_id;
        const uint32_t nt = std::max(1u, std::min(32u, std::thread::hardware_concurrency()));
        detail::parallel_ranges(n, n > (uint64_t(1) << 16) ? nt : 1, [&](uint64_t b, uint64_t e, uint32_t) {
            iterate_kmers_packed(*d->idx, begin_kmer_id + b, begin_kmer_id + e, out_words + b * W);
        });
    });
}

sshash_status sshash_iterate_packed_device(const sshash_dict* d, int device, uint64_t begin_kmer_id, uint64_t end_kmer_id,
                                           uint64_t* out_words, void* hip_stream) {
    if (!d || (!out_words && end_kmer_id > begin_kmer_id)) return fail(SSHASH_ERR_ARGUMENT, "null argument");
    return guarded([&] { d->eng->iterate_packed_device(device, begin_kmer_id, end_kmer_id, out_words, hip_stream); });
}

sshash_status sshash_check_device(const sshash_dict* d, int device, uint64_t out[8]) {
    if (!d || !out) return fail(SSHASH_ERR_ARGUMENT, "null argument");
    return guarded([&] { d->eng->check_device(device, out); });
}

sshash_status sshash_streaming_query_from_file(const sshash_dict* d, const char* filename, int multiline,
                                               sshash_streaming_report* report) {
    if (!d || !filename || !report) return fail(SSHASH_ERR_ARGUMENT, "null argument");
    const report_out rep(report);
    return guarded([&] {
        with_query_file(d, filename, multiline, false, [&](read_stream& in) {
            /* an uncompressed FASTQ is read and parsed by all the lanes at once (reads.hpp: fastq_pieces); a file that is not four
               lines per record comes back here and takes the sequential reader */
            if (!multiline && fastq_pieces::applicable(filename) && !test_hook_u64("sequential_reader", 0, 0, 1)) {
                streaming_report r;
                if (d->eng->streaming_query_fastq_pieces(filename, r)) {
                    rep.fill(r);
                    return;
                }
            }
            streaming_report total;
            for_each_batch(in, [&](read_batch const& batch) {
                rep.fill(total += d->eng->streaming_query_host(batch.bases.data(), batch.offsets.data(), batch.num_reads()));
            });
        });
    });
}

sshash_status sshash_streaming_query_from_file_per_read(const sshash_dict* d, const char* filename, int multiline,
                                                        sshash_per_read_fn fn, void* ctx, sshash_streaming_report* report) {
    if (!d || !filename || !fn) return fail(SSHASH_ERR_ARGUMENT, "null argument");
    const report_out rep(report);
    return guarded([&] {
        with_query_file(d, filename, multiline, true, [&](read_stream& in) {
            static_assert(sizeof(sshash_streaming_report) == 6 * sizeof(uint64_t), "a row is six words");
            rows_from_file<sshash_streaming_report>(in, 1, fn, ctx, rep, [&](read_batch const& b, sshash_streaming_report* rows) {
                return d->eng->streaming_query_per_read_host(b.bases.data(), b.offsets.data(), b.num_reads(), reinterpret_cast<uint64_t*>(rows));
            });
        });
    });
}

sshash_status sshash_streaming_query(const sshash_dict* d, const char* bases, const uint64_t* read_offsets,
                                     uint64_t num_reads, sshash_streaming_report* report) {
    if (!d || !report || (num_reads && (!bases || !read_offsets))) return fail(SSHASH_ERR_ARGUMENT, "null argument");
    const report_out rep(report);
    return guarded([&] { rep.fill(d->eng->streaming_query_host(bases, read_offsets, num_reads)); });
}

sshash_status sshash_streaming_query_device(const sshash_dict* d, int device, const char* bases,
                                            const uint64_t* read_offsets, uint64_t num_reads, uint64_t total_bases,
                                            uint64_t* report, void* hip_stream) {
    if (!d || !report || (num_reads && (!bases || !read_offsets))) return fail(SSHASH_ERR_ARGUMENT, "null argument");
    return guarded([&] { d->eng->streaming_query_device(device, bases, read_offsets, num_reads, total_bases, report, hip_stream); });
}

sshash_status sshash_streaming_query_per_read_device(const sshash_dict* d, int device, const char* bases,
                                                     const uint64_t* read_offsets, uint64_t num_reads, uint64_t total_bases,
                                                     sshash_streaming_report* per_read, uint64_t* report, void* hip_stream) {
    if (!d || (num_reads && (!bases || !read_offsets || !per_read))) return fail(SSHASH_ERR_ARGUMENT, "null argument");
    return guarded([&] {
        d->eng->streaming_query_per_read_device(device, bases, read_offsets, num_reads, total_bases, reinterpret_cast<uint64_t*>(per_read), report, hip_stream);
    });
}

sshash_status sshash_streaming_query_per_read(const sshash_dict* d, const char* bases, const uint64_t* read_offsets,
                                              uint64_t num_reads, sshash_streaming_report* per_read,
                                              sshash_streaming_report* report) {
    if (!d || (num_reads && (!bases || !read_offsets || !per_read))) return fail(SSHASH_ERR_ARGUMENT, "null argument");
    const report_out rep(report);
    return guarded([&] {
        rep.fill(d->eng->streaming_query_per_read_host(bases, read_offsets, num_reads, reinterpret_cast<uint64_t*>(per_read)));
    });
}

static_assert(sizeof(sshash_streaming_run) == 32, "a run record is 32 bytes: two 16-byte stores on the device");

sshash_status sshash_streaming_runs_device(const sshash_dict* d, int device, const char* bases, const uint64_t* read_offsets,
                                           uint64_t num_reads, uint64_t total_bases, uint64_t* run_offsets,
                                           sshash_streaming_run* runs, uint64_t runs_capacity, uint64_t* report, void* hip_stream) {
    if (!d || (num_reads && (!bases || !read_offsets || !run_offsets)) || (!runs && runs_capacity)) return fail(SSHASH_ERR_ARGUMENT, "null argument");
    return guarded([&] {
        d->eng->streaming_runs_device(device, bases, read_offsets, num_reads, total_bases, run_offsets, runs, runs_capacity, report, hip_stream);
    });
}

sshash_status sshash_streaming_runs(const sshash_dict* d, const char* bases, const uint64_t* read_offsets, uint64_t num_reads,
                                    uint64_t* run_offsets, sshash_streaming_run* runs, uint64_t runs_capacity,
                                    sshash_streaming_report* report) {
    if (!d || (num_reads && (!bases || !read_offsets || !run_offsets)) || (!runs && runs_capacity)) return fail(SSHASH_ERR_ARGUMENT, "null argument");
    const report_out rep(report);
    return guarded([&] {
        rep.fill(d->eng->streaming_runs_host(bases, read_offsets, num_reads, run_offsets, runs, runs_capacity));
    });
}

sshash_status sshash_streaming_runs_from_file(const sshash_dict* d, const char* filename, int multiline, sshash_read_runs_fn fn, void* ctx,
                                              sshash_streaming_report* report) {
    if (!d || !filename || !fn) return fail(SSHASH_ERR_ARGUMENT, "null argument");
    const report_out rep(report);
    return guarded([&] {
        with_query_file(d, filename, multiline, true, [&](read_stream& in) {
            streaming_report total;
            uint64_t first_read = 0;
            std::vector<uint64_t> run_offsets, records;  // (a batch's, local to it: one counting pass sizes the records, the engine hands both back)
            for_each_batch(in, [&](read_batch const& batch) {
                const uint64_t n = batch.num_reads();
                if (n == 0) return;
                rep.fill(total += d->eng->streaming_runs_host(batch.bases.data(), batch.offsets.data(), n, run_offsets, records));
                const int stop = fn(ctx, first_read, n, run_offsets.data(), reinterpret_cast<const sshash_streaming_run*>(records.data()));
                if (stop) throw error(error_kind::argument, "the per-read callback returned " + std::to_string(stop));
                first_read += n;
            });
        });
    });
}

sshash_status sshash_cover_words(const sshash_dict* d, uint64_t* words) {
    if (!d || !words) return fail(SSHASH_ERR_ARGUMENT, "null argument");
    *words = (d->idx->num_kmers + 63) / 64;
    return SSHASH_OK;
}

sshash_status sshash_streaming_cover_device(const sshash_dict* d, int device, const char* bases, const uint64_t* read_offsets,
                                            uint64_t num_reads, uint64_t total_bases, uint64_t* cover, uint64_t* report, void* hip_stream) {
    if (!d || (num_reads && (!bases || !read_offsets || !cover))) return fail(SSHASH_ERR_ARGUMENT, "null argument");
    return guarded([&] { d->eng->streaming_cover_device(device, bases, read_offsets, num_reads, total_bases, cover, report, hip_stream); });
}

sshash_status sshash_streaming_cover(const sshash_dict* d, const char* bases, const uint64_t* read_offsets, uint64_t num_reads,
                                     uint64_t* cover, sshash_streaming_report* report) {
    if (!d || (num_reads && (!bases || !read_offsets || !cover))) return fail(SSHASH_ERR_ARGUMENT, "null argument");
    const report_out rep(report);
    return guarded([&] {
        if (num_reads == 0) return;
        const cover_bitmaps on_devices(*d->eng);
        const streaming_report r = d->eng->streaming_cover_host(bases, read_offsets, num_reads, on_devices);
        on_devices.or_into(cover);
        rep.fill(r);
    });
}

sshash_status sshash_streaming_cover_from_file(const sshash_dict* d, const char* filename, int multiline, uint64_t* cover,
                                               sshash_streaming_report* report) {
    if (!d || !filename || !cover) return fail(SSHASH_ERR_ARGUMENT, "null argument");
    const report_out rep(report);
    return guarded([&] {
        accumulate_from_file<cover_bitmaps>(
            d, filename, multiline, rep,
            [&](read_batch const& b, cover_bitmaps const& bitmaps) { return d->eng->streaming_cover_host(b.bases.data(), b.offsets.data(), b.num_reads(), bitmaps); },
            [&](cover_bitmaps const& bitmaps) { bitmaps.or_into(cover); });
    });
}

sshash_status sshash_cover_string_counts_device(const sshash_dict* d, int device, const uint64_t* cover, uint64_t* counts, uint64_t* total,
                                                void* hip_stream) {
    if (!d || !cover || !counts) return fail(SSHASH_ERR_ARGUMENT, "null argument");
    return guarded([&] { d->eng->cover_string_counts_device(device, cover, counts, total, hip_stream); });
}

sshash_status sshash_cover_string_counts(const sshash_dict* d, const uint64_t* cover, uint64_t* counts, uint64_t* total) {
    if (!d || !cover || !counts) return fail(SSHASH_ERR_ARGUMENT, "null argument");
    return guarded([&] {
        host_index const& x = *d->idx;
        /* set bits among the ids [lo, hi) */
        auto bits_in = [cover](uint64_t lo, uint64_t hi) {
            uint64_t n = 0;
            while (lo < hi) {
                const uint64_t end = std::min(hi, (lo | 63) + 1);  // the part of [lo, hi) inside lo's word
                uint64_t w = cover[lo >> 6] >> (lo & 63);
                if (end - lo < 64) w &= (uint64_t(1) << (end - lo)) - 1;
                n += uint64_t(__builtin_popcountll(w));
                lo = end;
            }
            return n;
        };
        uint64_t all = 0;
        for (uint64_t s = 0; s < x.num_strings; ++s) {  // at_string_id(s): [endpoints[s] - s (k - 1), endpoints[s + 1] - (s + 1)(k - 1))
            counts[s] = bits_in(x.endpoints[s] - s * (x.k - 1), x.endpoints[s + 1] - (s + 1) * (x.k - 1));
            all += counts[s];
        }
        if (total) *total = all;
    });
}

sshash_status sshash_streaming_depth_device(const sshash_dict* d, int device, const char* bases, const uint64_t* read_offsets,
                                            uint64_t num_reads, uint64_t total_bases, uint32_t* deltas, uint64_t* report, void* hip_stream) {
    if (!d || (num_reads && (!bases || !read_offsets || !deltas))) return fail(SSHASH_ERR_ARGUMENT, "null argument");
    return guarded([&] { d->eng->streaming_depth_device(device, bases, read_offsets, num_reads, total_bases, deltas, report, hip_stream); });
}

sshash_status sshash_depth_finish_device(const sshash_dict* d, int device, const uint32_t* deltas, uint32_t* depth, void* hip_stream) {
    if (!d || !deltas || !depth) return fail(SSHASH_ERR_ARGUMENT, "null argument");
    return guarded([&] { d->eng->depth_finish_device(device, deltas, depth, hip_stream); });
}

sshash_status sshash_streaming_depth(const sshash_dict* d, const char* bases, const uint64_t* read_offsets, uint64_t num_reads,
                                     uint32_t* depth, sshash_streaming_report* report) {
    if (!d || (num_reads && (!bases || !read_offsets || !depth))) return fail(SSHASH_ERR_ARGUMENT, "null argument");
    const report_out rep(report);
    return guarded([&] {
        if (num_reads == 0) return;
        const depth_arrays on_devices(*d->eng);
        const streaming_report r = d->eng->streaming_depth_host(bases, read_offsets, num_reads, on_devices);
        on_devices.add_into(depth);
        rep.fill(r);
    });
}

sshash_status sshash_streaming_depth_from_file(const sshash_dict* d, const char* filename, int multiline, uint32_t* depth,
                                               sshash_streaming_report* report) {
    if (!d || !filename || !depth) return fail(SSHASH_ERR_ARGUMENT, "null argument");
    const report_out rep(report);
    return guarded([&] {
        accumulate_from_file<depth_arrays>(
            d, filename, multiline, rep,
            [&](read_batch const& b, depth_arrays const& deltas) { return d->eng->streaming_depth_host(b.bases.data(), b.offsets.data(), b.num_reads(), deltas); },
            [&](depth_arrays const& deltas) { deltas.add_into(depth); });
    });
}

sshash_status sshash_depth_string_sums_device(const sshash_dict* d, int device, const uint32_t* depth, uint64_t* sums, uint64_t* total,
                                              void* hip_stream) {
    if (!d || !depth || !sums) return fail(SSHASH_ERR_ARGUMENT, "null argument");
    return guarded([&] { d->eng->depth_string_sums_device(device, depth, sums, total, hip_stream); });
}

sshash_status sshash_depth_string_sums(const sshash_dict* d, const uint32_t* depth, uint64_t* sums, uint64_t* total) {
    if (!d || !depth || !sums) return fail(SSHASH_ERR_ARGUMENT, "null argument");
    return guarded([&] {
        host_index const& x = *d->idx;
        uint64_t all = 0;
        for (uint64_t s = 0; s < x.num_strings; ++s) {  // the ids of string s, as sshash_cover_string_counts
            const uint64_t lo = x.endpoints[s] - s * (x.k - 1), hi = x.endpoints[s + 1] - (s + 1) * (x.k - 1);
            uint64_t sum = 0;
            for (uint64_t i = lo; i < hi; ++i) sum += depth[i];
            sums[s] = sum;
            all += sum;
        }
        if (total) *total = all;
    });
}

static_assert(sizeof(sshash_read_sum) == 2 * sizeof(uint64_t), "a row of sums is two words");

sshash_status sshash_value_prefix_device(const sshash_dict* d, int device, const uint32_t* values, uint32_t at_least, uint64_t* prefix,
                                         void* hip_stream) {
    if (!d || !values || !prefix) return fail(SSHASH_ERR_ARGUMENT, "null argument");
    return guarded([&] { d->eng->value_prefix_device(device, values, at_least, prefix, hip_stream); });
}

sshash_status sshash_streaming_sums_device(const sshash_dict* d, int device, const char* bases, const uint64_t* read_offsets,
                                           uint64_t num_reads, uint64_t total_bases, const uint64_t* prefix, sshash_read_sum* sums,
                                           uint64_t* report, void* hip_stream) {
    if (!d || (num_reads && (!bases || !read_offsets || !prefix || !sums))) return fail(SSHASH_ERR_ARGUMENT, "null argument");
    return guarded([&] {
        d->eng->streaming_sums_device(device, bases, read_offsets, num_reads, total_bases, prefix, reinterpret_cast<uint64_t*>(sums), report, hip_stream);
    });
}

sshash_status sshash_streaming_sums(const sshash_dict* d, const char* bases, const uint64_t* read_offsets, uint64_t num_reads,
                                    const uint32_t* values, uint32_t at_least, sshash_read_sum* sums, sshash_streaming_report* report) {
    if (!d || (num_reads && (!bases || !read_offsets || !values || !sums))) return fail(SSHASH_ERR_ARGUMENT, "null argument");
    const report_out rep(report);
    return guarded([&] {
        if (num_reads == 0) return;
        const value_prefixes on_devices(*d->eng, values, at_least);
        rep.fill(d->eng->streaming_sums_host(bases, read_offsets, num_reads, on_devices, reinterpret_cast<uint64_t*>(sums)));
    });
}

sshash_status sshash_streaming_sums_from_file(const sshash_dict* d, const char* filename, int multiline, const uint32_t* values,
                                              uint32_t at_least, sshash_read_sums_fn fn, void* ctx, sshash_streaming_report* report) {
    if (!d || !filename || !values || !fn) return fail(SSHASH_ERR_ARGUMENT, "null argument");
    const report_out rep(report);
    return guarded([&] {
        with_query_file(d, filename, multiline, true, [&](read_stream& in) {
            const value_prefixes on_devices(*d->eng, values, at_least);  // (the prefix stays on the devices from the first batch to the last)
            rows_from_file<sshash_read_sum>(in, 1, fn, ctx, rep, [&](read_batch const& b, sshash_read_sum* rows) {
                return d->eng->streaming_sums_host(b.bases.data(), b.offsets.data(), b.num_reads(), on_devices, reinterpret_cast<uint64_t*>(rows));
            });
        });
    });
}

static_assert(sizeof(sshash_read_class) == 4 * sizeof(uint32_t), "a read's class is four words");
static_assert(SSHASH_MAX_CLASSES == engine::MAX_CLASSES, "one cap");

static bool classes_in_range(uint32_t num_classes) { return num_classes >= 1 && num_classes <= SSHASH_MAX_CLASSES; }

sshash_status sshash_streaming_classes_device(const sshash_dict* d, int device, const char* bases, const uint64_t* read_offsets,
                                              uint64_t num_reads, uint64_t total_bases, const uint32_t* labels, uint32_t num_classes,
                                              uint32_t* rows, uint64_t* report, void* hip_stream) {
    if (!d || (num_reads && (!bases || !read_offsets || !labels || !rows))) return fail(SSHASH_ERR_ARGUMENT, "null argument");
    if (!classes_in_range(num_classes)) return fail(SSHASH_ERR_ARGUMENT, "num_classes must be 1 .. SSHASH_MAX_CLASSES");
    return guarded([&] {
        d->eng->streaming_classes_device(device, bases, read_offsets, num_reads, total_bases, labels, num_classes, rows, report, hip_stream);
    });
}

sshash_status sshash_streaming_classes(const sshash_dict* d, const char* bases, const uint64_t* read_offsets, uint64_t num_reads,
                                       const uint32_t* labels, uint32_t num_classes, uint32_t* rows, sshash_streaming_report* report) {
    if (!d || (num_reads && (!bases || !read_offsets || !labels || !rows))) return fail(SSHASH_ERR_ARGUMENT, "null argument");
    if (!classes_in_range(num_classes)) return fail(SSHASH_ERR_ARGUMENT, "num_classes must be 1 .. SSHASH_MAX_CLASSES");
    const report_out rep(report);
    return guarded([&] {
        if (num_reads == 0) return;
        const class_labels_on_devices on_devices(*d->eng, labels);
        rep.fill(d->eng->streaming_classes_host(bases, read_offsets, num_reads, on_devices, num_classes, rows));
    });
}

sshash_status sshash_streaming_classes_from_file(const sshash_dict* d, const char* filename, int multiline, const uint32_t* labels,
                                                 uint32_t num_classes, sshash_read_classes_fn fn, void* ctx, sshash_streaming_report* report) {
    if (!d || !filename || !labels || !fn) return fail(SSHASH_ERR_ARGUMENT, "null argument");
    if (!classes_in_range(num_classes)) return fail(SSHASH_ERR_ARGUMENT, "num_classes must be 1 .. SSHASH_MAX_CLASSES");
    const report_out rep(report);
    return guarded([&] {
        with_query_file(d, filename, multiline, true, [&](read_stream& in) {
            const class_labels_on_devices on_devices(*d->eng, labels);  // (the labels stay on the devices from the first batch to the last)
            rows_from_file<uint32_t>(in, num_classes, fn, ctx, rep, [&](read_batch const& b, uint32_t* rows) {
                return d->eng->streaming_classes_host(b.bases.data(), b.offsets.data(), b.num_reads(), on_devices, num_classes, rows);
            });
        });
    });
}

sshash_status sshash_class_best_device(const sshash_dict* d, int device, const uint32_t* rows, uint64_t num_reads, uint32_t num_classes,
                                       sshash_read_class* best, void* hip_stream) {
    if (!d || (num_reads && (!rows || !best))) return fail(SSHASH_ERR_ARGUMENT, "null argument");
    if (!classes_in_range(num_classes)) return fail(SSHASH_ERR_ARGUMENT, "num_classes must be 1 .. SSHASH_MAX_CLASSES");
    return guarded([&] { d->eng->class_best_device(device, rows, num_reads, num_classes, reinterpret_cast<uint32_t*>(best), hip_stream); });
}

sshash_status sshash_class_best(const uint32_t* rows, uint64_t num_reads, uint32_t num_classes, sshash_read_class* best) {
    if (num_reads && (!rows || !best)) return fail(SSHASH_ERR_ARGUMENT, "null argument");
    if (!classes_in_range(num_classes)) return fail(SSHASH_ERR_ARGUMENT, "num_classes must be 1 .. SSHASH_MAX_CLASSES");
    return guarded([&] {
        for (uint64_t r = 0; r < num_reads; ++r) {
            const uint32_t* const row = rows + r * num_classes;
            sshash_read_class out{SSHASH_NO_CLASS, 0, 0, 0};
            for (uint32_t c = 0; c < num_classes; ++c) {  // (ascending, and only a LARGER count takes the lead: among equals the smallest class)
                const uint32_t v = row[c];
                out.total += v;
                if (v > out.best) {
                    out.second = out.best;
                    out.best = v;
                    out.best_class = c;
                } else if (v > out.second) {
                    out.second = v;
                }
            }
            best[r] = out;
        }
    });
}

sshash_status sshash_class_totals_device(const sshash_dict* d, int device, const uint32_t* rows, uint64_t num_reads, uint32_t num_classes,
                                         uint64_t* totals, void* hip_stream) {
    if (!d || !totals || (num_reads && !rows)) return fail(SSHASH_ERR_ARGUMENT, "null argument");
    if (!classes_in_range(num_classes)) return fail(SSHASH_ERR_ARGUMENT, "num_classes must be 1 .. SSHASH_MAX_CLASSES");
    return guarded([&] { d->eng->class_totals_device(device, rows, num_reads, num_classes, totals, hip_stream); });
}

sshash_status sshash_class_totals(const uint32_t* rows, uint64_t num_reads, uint32_t num_classes, uint64_t* totals) {
    if (!totals || (num_reads && !rows)) return fail(SSHASH_ERR_ARGUMENT, "null argument");
    if (!classes_in_range(num_classes)) return fail(SSHASH_ERR_ARGUMENT, "num_classes must be 1 .. SSHASH_MAX_CLASSES");
    return guarded([&] {
        std::fill(totals, totals + num_classes, uint64_t(0));
        for (uint64_t r = 0; r < num_reads; ++r)
            for (uint32_t c = 0; c < num_classes; ++c) totals[c] += rows[r * num_classes + c];
    });
}

/* ---- anchors: per read, its longest run (a sshash_streaming_run of 32 bytes: the static_assert stands with sshash_streaming_runs_device) ---- */
sshash_status sshash_streaming_best_run_device(const sshash_dict* d, int device, const char* bases, const uint64_t* read_offsets,
                                               uint64_t num_reads, uint64_t total_bases, sshash_streaming_run* best, uint64_t* report,
                                               void* hip_stream) {
    if (!d || (num_reads && (!bases || !read_offsets || !best))) return fail(SSHASH_ERR_ARGUMENT, "null argument");
    return guarded([&] { d->eng->streaming_best_run_device(device, bases, read_offsets, num_reads, total_bases, best, report, hip_stream); });
}

sshash_status sshash_streaming_best_run(const sshash_dict* d, const char* bases, const uint64_t* read_offsets, uint64_t num_reads,
                                        sshash_streaming_run* best, sshash_streaming_report* report) {
    if (!d || (num_reads && (!bases || !read_offsets || !best))) return fail(SSHASH_ERR_ARGUMENT, "null argument");
    const report_out rep(report);
    return guarded([&] {
        if (num_reads == 0) return;
        rep.fill(d->eng->streaming_best_run_host(bases, read_offsets, num_reads, best));
    });
}

sshash_status sshash_streaming_best_run_from_file(const sshash_dict* d, const char* filename, int multiline, sshash_read_best_run_fn fn,
                                                  void* ctx, sshash_streaming_report* report) {
    if (!d || !filename || !fn) return fail(SSHASH_ERR_ARGUMENT, "null argument");
    const report_out rep(report);
    return guarded([&] {
        d->eng->best_run_ready();  // (no replica, a minimizer shard: said before the file is opened)
        with_query_file(d, filename, multiline, true, [&](read_stream& in) {
            rows_from_file<sshash_streaming_run>(in, 1, fn, ctx, rep, [&](read_batch const& b, sshash_streaming_run* best) {
                return d->eng->streaming_best_run_host(b.bases.data(), b.offsets.data(), b.num_reads(), best);
            });
        });
    });
}

sshash_status sshash_runs_best_device(const sshash_dict* d, int device, const uint64_t* run_offsets, const sshash_streaming_run* runs,
                                      uint64_t num_reads, sshash_streaming_run* best, void* hip_stream) {
    if (!d || (num_reads && (!run_offsets || !best))) return fail(SSHASH_ERR_ARGUMENT, "null argument");
    return guarded([&] { d->eng->runs_best_device(device, run_offsets, runs, num_reads, best, hip_stream); });
}

sshash_status sshash_runs_best(const uint64_t* run_offsets, const sshash_streaming_run* runs, uint64_t num_reads, sshash_streaming_run* best) {
    if (num_reads && (!run_offsets || !best)) return fail(SSHASH_ERR_ARGUMENT, "null argument");
    if (num_reads && !runs && run_offsets[num_reads] > run_offsets[0]) return fail(SSHASH_ERR_ARGUMENT, "null argument");
    return guarded([&] {
        for (uint64_t r = 0; r < num_reads; ++r) {
            sshash_streaming_run out;
            std::memset(&out, 0, sizeof(out));
            uint32_t longest = 0;
            for (uint64_t i = run_offsets[r]; i < run_offsets[r + 1]; ++i) {  // (in read order, and only a LONGER run takes the lead: among equals the first)
                const uint32_t length = runs[i].num_kmers & ~SSHASH_RUN_BACKWARD;
                if (length > longest) {
                    longest = length;
                    out = runs[i];
                }
            }
            best[r] = out;
        }
    });
}

sshash_status sshash_streaming_lookup_device(const sshash_dict* d, int device, const char* bases, const uint64_t* read_offsets,
                                             uint64_t num_reads, uint64_t total_bases, const sshash_results* out, uint64_t* report,
                                             void* hip_stream) {
    if (!d || !out || (num_reads && (!bases || !read_offsets))) return fail(SSHASH_ERR_ARGUMENT, "null argument");
    return guarded([&] { d->eng->streaming_lookup_device(device, bases, read_offsets, num_reads, total_bases, to_view(out), report, hip_stream); });
}

sshash_status sshash_streaming_lookup(const sshash_dict* d, const char* bases, const uint64_t* read_offsets, uint64_t num_reads,
                                      const sshash_results* out, sshash_streaming_report* report) {
    if (!d || !out || (num_reads && (!bases || !read_offsets))) return fail(SSHASH_ERR_ARGUMENT, "null argument");
    const report_out rep(report);
    return guarded([&] {
        rep.fill(d->eng->streaming_lookup_host(bases, read_offsets, num_reads, to_view(out)));
    });
}

sshash_status sshash_route_packed_device(const sshash_dict* d, int device, const uint64_t* kmers, uint64_t n,
                                         uint32_t num_shards, uint32_t* owner_forward, uint32_t* owner_reverse,
                                         void* hip_stream) {
    if (!d || (n && (!kmers || !owner_forward || !owner_reverse)) || num_shards == 0) return fail(SSHASH_ERR_ARGUMENT, "null argument");
    return guarded([&] { d->eng->route_packed_device(device, kmers, n, num_shards, owner_forward, owner_reverse, hip_stream); });
}

sshash_status sshash_route_bucket_device(const sshash_dict* d, int device, const uint64_t* kmers, uint64_t n,
                                         uint32_t num_shards, int check_rc, uint64_t* cursors, uint64_t* send,
                                         uint32_t* slots, void* hip_stream) {
    if (!d || (n && !kmers) || !cursors) return fail(SSHASH_ERR_ARGUMENT, "null argument");
    return guarded([&] { d->eng->route_bucket_device(device, kmers, n, num_shards, check_rc != 0, false, cursors, send, slots, hip_stream); });
}

sshash_status sshash_route_bucket_by_key_device(const sshash_dict* d, int device, const uint64_t* kmers, uint64_t n,
                                                uint32_t num_shards, uint64_t* cursors, uint64_t* send, uint32_t* slots,
                                                void* hip_stream) {
    if (!d || (n && !kmers) || !cursors) return fail(SSHASH_ERR_ARGUMENT, "null argument");
    return guarded([&] { d->eng->route_bucket_device(device, kmers, n, num_shards, true, true, cursors, send, slots, hip_stream); });
}

sshash_status sshash_to_device_table_shard(sshash_dict* d, int device, uint32_t num_table_shards, uint32_t table_shard_id) {
    if (!d) return fail(SSHASH_ERR_ARGUMENT, "null argument");
    return guarded([&] { d->eng->to_device(device, num_table_shards, table_shard_id); });
}

sshash_status sshash_route_combine_device(const sshash_dict* d, int device, const uint64_t* replies, const uint32_t* slots,
                                          uint64_t m, uint64_t* out, void* hip_stream) {
    if (!d || (m && (!replies || !slots || !out))) return fail(SSHASH_ERR_ARGUMENT, "null argument");
    return guarded([&] { d->eng->route_combine_device(device, replies, slots, m, out, hip_stream); });
}

sshash_status sshash_sharded_lookup_device(const sshash_dict* d, int device, uint32_t num_ranks, int by_table_key,
                                           const uint64_t* kmers, uint64_t n, int check_rc, uint64_t* kmer_ids,
                                           const sshash_exchange* exchange, void* hip_stream) {
    if (!d || !exchange || (n && (!kmers || !kmer_ids))) return fail(SSHASH_ERR_ARGUMENT, "null argument");
    return guarded([&] {
        exchange_ops x{exchange->ctx, exchange->counts, exchange->data};
        d->eng->sharded_lookup_device(device, num_ranks, by_table_key != 0, kmers, n, check_rc != 0, kmer_ids, x, hip_stream);
    });
}

sshash_status sshash_sharded_lookup_rccl(const sshash_dict* d, int device, void* nccl_comm, int by_table_key, const uint64_t* kmers,
                                         uint64_t n, int check_rc, uint64_t* kmer_ids, void* hip_stream) {
    if (!d || !nccl_comm || (n && (!kmers || !kmer_ids))) return fail(SSHASH_ERR_ARGUMENT, "null argument");
    return guarded([&] { d->eng->sharded_lookup_rccl(device, nccl_comm, by_table_key != 0, kmers, n, check_rc != 0, kmer_ids, hip_stream); });
}

}  // extern "C"
