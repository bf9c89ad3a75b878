// replica.hpp -- one dictionary replica resident in the HBM of one device (internal header).
#pragma once

#include <algorithm>
#include <atomic>

#include <cstdio>
#include <cstdlib>

#include <hip/hip_runtime.h>

#include <functional>
#include <mutex>
#include <stdexcept>
#include <string>
#include <unordered_map>
#include <vector>

#include "lookup_device.hpp"
#include "mphf_build.hpp"

namespace sshash_amd {

inline void hip_check(hipError_t e, char const* what) {
    if (e != hipSuccess) throw error(error_kind::hip, std::string("HIP error in ") + what + ": " + hipGetErrorString(e));
}
#define HIP_CHECK(x) ::sshash_amd::hip_check((x), #x)

struct device_guard {
    int prev = 0;
    int target;
    explicit device_guard(int dev) : target(dev) {
        HIP_CHECK(hipGetDevice(&prev));
        if (prev != dev) HIP_CHECK(hipSetDevice(dev));
    }
    ~device_guard() {
        if (prev != target) (void)hipSetDevice(prev);
    }
};

/* one pipeline of the host-buffer entry points: stream + pinned staging block + device block (engine.hip) */
struct host_lane {
    hipStream_t stream = nullptr;
    void* pinned = nullptr;
    void* device = nullptr;
    size_t capacity = 0;
};

/* a device block kept for one stream (stream_cache): free_block() before it grows, release() when the stream gives it up */
struct stream_block {
    void* block = nullptr;
    size_t bytes = 0;
    void free_block() {
        if (block) HIP_CHECK(hipFree(block));  // (synchronises: nothing in flight still uses it)
        block = nullptr;
        bytes = 0;
    }
    void release() {
        if (block) (void)hipFree(block);
        block = nullptr;
        bytes = 0;
    }
};

/* Device blocks keyed by stream. Work on one stream is ordered, so its block is reused without synchronisation; a block only
   grows (hipFree of the old block synchronises implicitly). Once more than MAX_STREAMS streams or MAX_BYTES bytes would be
   held, the least recently used blocks other than the one being grown go first. Slot: a stream_block, or one with more to
   wait for before its block is freed, or more to release. */
template <typename Slot, size_t MAX_STREAMS, size_t MAX_BYTES>
class stream_cache {
public:
    /* the slot of `stream`, its block at least `bytes` (grown with 1/headroom to spare) */
    Slot& get(void* stream, size_t bytes, size_t headroom) {
        std::lock_guard<std::mutex> lock(m_mutex);
        auto it = m_slots.try_emplace(stream).first;
        it->second.last_use = ++m_clock;
        Slot& slot = it->second.slot;
        if (slot.bytes >= bytes) return slot;
        slot.free_block();
        const size_t want = bytes + bytes / headroom + 4096;
        size_t held = want;
        for (auto const& kv : m_slots) held += kv.second.slot.bytes;
        while (m_slots.size() > 1 && (m_slots.size() > MAX_STREAMS || held > MAX_BYTES)) {
            auto oldest = m_slots.end();
            for (auto jt = m_slots.begin(); jt != m_slots.end(); ++jt)
                if (jt != it && (oldest == m_slots.end() || jt->second.last_use < oldest->second.last_use)) oldest = jt;
            held -= oldest->second.slot.bytes;
            oldest->second.slot.release();
            m_slots.erase(oldest);
        }
        HIP_CHECK(hipMalloc(&slot.block, want));
        slot.bytes = want;
        return slot;
    }
    void release(void* stream) {
        std::lock_guard<std::mutex> lock(m_mutex);
        auto it = m_slots.find(stream);
        if (it == m_slots.end()) return;
        it->second.slot.release();
        m_slots.erase(it);
    }
    void clear() {
        std::lock_guard<std::mutex> lock(m_mutex);
        for (auto& kv : m_slots) kv.second.slot.release();
        m_slots.clear();
    }

private:
    struct entry {
        Slot slot;
        uint64_t last_use = 0;
    };
    std::mutex m_mutex;
    std::unordered_map<void*, entry> m_slots;
    uint64_t m_clock = 0;
};

struct device_replica {
    int device = -1;
    uint64_t bytes = 0;
    uint64_t bytes_still_to_come = 0;  // during the upload: what follows the super-k-mer table (its budget test counts it in)
    dict_view view{};
    skew_part_dev* d_skew = nullptr;
    uint64_t directory_overflowed = 0;  // sectors carrying the overflow flag
    uint64_t directory_entries = 0;     // keys resident in the directory
    uint64_t sk_keys = 0, sk_heavy_keys = 0, sk_heavy_kmers = 0, sk_unplaced = 0, sk_slots_used = 0, sk_bytes = 0;  // super-k-mer table
    uint32_t sk_absent_reason = 1;  // SK_ABSENT_* (0 = the table is there)
    /* keys of the table by number of occurrences (bins SK_HIST_BINS: 1, 2, 3, 4, 5-8, 9-16, 17-64, 65-1024, > 1024):
       [0..9) keys per bin, [9..18) occurrences (= super-k-mers) per bin; [18] super-k-mers, [19] slots asked for */
    uint64_t sk_histogram[20] = {0};
    std::vector<void*> allocations;
    /* Stream-ordered scratch of the batched calls (streaming lookup, sharded lookup, neighbours) comes out of a memory pool of
       this replica's own, which keeps what it has used (a pool hands everything back to the driver at the next
       synchronisation by default: 13 vs 190-260 ms per 3 x 10^8-base streaming lookup). Round 2 raised the threshold of the
       DEVICE'S DEFAULT pool instead -- a process-wide side effect on the embedding application, whose own hipMallocAsync
       blocks were then never returned either. */
    hipMemPool_t scratch_pool = nullptr;
    void create_scratch_pool() {
        hipMemPoolProps props{};
        props.allocType = hipMemAllocationTypePinned;
        props.handleTypes = hipMemHandleTypeNone;
        props.location.type = hipMemLocationTypeDevice;
        props.location.id = device;
        if (hipMemPoolCreate(&scratch_pool, &props) != hipSuccess) {
            scratch_pool = nullptr;  // (fall back to the default pool with its default behaviour)
            (void)hipGetLastError();
            /* not silently: the default pool hands its memory back at every synchronisation -- 190-260 ms instead of 13 per batched
               streaming call (HISTORY.md) */
            if (std::getenv("SSHASH_AMD_VERBOSE"))
                fprintf(stderr, "[sshash_amd] device %d: no private memory pool (hipMemPoolCreate failed): stream-ordered scratch comes out of the default pool\n", device);
            return;
        }
        uint64_t keep = ~uint64_t(0);
        (void)hipMemPoolSetAttribute(scratch_pool, hipMemPoolAttrReleaseThreshold, &keep);
    }
    void* stream_alloc(size_t bytes, hipStream_t s) const {
        void* p = nullptr;
        if (scratch_pool) HIP_CHECK(hipMallocFromPoolAsync(&p, bytes ? bytes : 8, scratch_pool, s));
        else HIP_CHECK(hipMallocAsync(&p, bytes ? bytes : 8, s));
        return p;
    }

    /* held while one launch sequence (queue reset, first / resume / deferred pass; the streaming runs) is enqueued: two host
       threads that share a stream (the null stream, typically) must not interleave their sequences, which share that stream's
       scratch below */
    mutable std::mutex launch_mutex;
    /* Per-stream scratch (stream_cache) for the resume and deferred queues of the multi-pass lookup (engine.hip). At most 16
       streams keep a block: an application that makes a stream per request must not keep a gigabyte of queues per stream it
       ever used. */
    struct stream_scratch : stream_block {
        /* the tail passes (resume, deferred) of one launch piece run on `aux` while the caller's stream already runs the
           first pass of the next piece (engine.hip: launch): one auxiliary stream and two event pairs per caller stream */
        hipStream_t aux = nullptr;
        hipEvent_t first_done[2] = {nullptr, nullptr};
        hipEvent_t tail_done[2] = {nullptr, nullptr};
        void free_block() {
            if (aux) HIP_CHECK(hipStreamSynchronize(aux));  // a tail pass of an earlier call may still read the block
            stream_block::free_block();
        }
        void release() {
            if (aux) (void)hipStreamSynchronize(aux);
            for (int i = 0; i < 2; ++i) {
                if (first_done[i]) (void)hipEventDestroy(first_done[i]);
                if (tail_done[i]) (void)hipEventDestroy(tail_done[i]);
                first_done[i] = tail_done[i] = nullptr;
            }
            if (aux) (void)hipStreamDestroy(aux);
            aux = nullptr;
            stream_block::release();
        }
    };
    mutable stream_cache<stream_scratch, 16, ~size_t(0)> queue_scratch;
    /* Per-stream scratch of the streaming query (streaming.hip: the 2-bit packed copy of a call's reads and their validity bits).
       Round 5 took it from the pool above and gave it back at every call -- two stream-ordered allocations of ~0.4 GB each per call
       of 3 x 10^9 bases, on the host side of a step that the device then waits for (profiles/r06/). Kept per stream instead, for
       at most 64 streams (the file query runs up to 32 lanes, each on its own stream) and 8 GiB. */
    mutable stream_cache<stream_block, 64, size_t(8) << 30> read_scratch;
    /* (the caller holds launch_mutex: the slot, its aux stream and its events are used outside the cache's own lock) */
    stream_scratch& scratch_for(void* stream, size_t bytes, bool with_aux_stream) const {
        stream_scratch& slot = queue_scratch.get(stream, bytes, 4);
        if (with_aux_stream && !slot.aux) {
            HIP_CHECK(hipStreamCreateWithFlags(&slot.aux, hipStreamNonBlocking));
            for (int i = 0; i < 2; ++i) {
                HIP_CHECK(hipEventCreateWithFlags(&slot.first_done[i], hipEventDisableTiming));
                HIP_CHECK(hipEventCreateWithFlags(&slot.tail_done[i], hipEventDisableTiming));
            }
        }
        return slot;
    }
    void* read_scratch_for(void* stream, size_t bytes) const { return read_scratch.get(stream, bytes, 8).block; }

    /* Hand back the scratch of a stream that its owner is about to destroy (the work on it must be complete): a call that makes a
       stream of its own for its duration (own_stream) leaves no block behind. */
    void release_stream_scratch(void* stream) const {
        queue_scratch.release(stream);
        read_scratch.release(stream);
    }

    /* pooled lanes of the host-buffer path */
    mutable std::mutex lanes_mutex;
    mutable std::vector<host_lane*> idle_lanes;
    host_lane* acquire_lane(size_t bytes) const;
    void release_lane(host_lane* lane) const;

    template <typename T>
    T* put(std::vector<T> const& v) {
        T* d = nullptr;
        const size_t n = (v.empty() ? 1 : v.size()) * sizeof(T);
        HIP_CHECK(hipMalloc(&d, n));
        allocations.push_back(d);
        if (!v.empty()) HIP_CHECK(hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
        bytes += n;
        return d;
    }
    mphf_view put_mphf(mphf_host const& f) {
        mphf_view v = f.view();
        v.parts = put(f.parts);
        v.pilots = put(f.pilots);
        v.free_slots = put(f.free_slots);
        return v;
    }
    device_replica() = default;
    device_replica(device_replica const&) = delete;
    device_replica& operator=(device_replica const&) = delete;
    ~device_replica() {
        if (device < 0) return;
        int prev = 0;
        if (hipGetDevice(&prev) != hipSuccess) return;
        (void)hipSetDevice(device);
        for (void* p : allocations) (void)hipFree(p);
        if (scratch_pool) {
            (void)hipDeviceSynchronize();  // (stream-ordered frees of this pool must have run)
            (void)hipMemPoolDestroy(scratch_pool);
        }
        queue_scratch.clear();
        read_scratch.clear();
        for (host_lane* lane : idle_lanes) {
            if (lane->pinned) (void)hipHostFree(lane->pinned);
            if (lane->device) (void)hipFree(lane->device);
            if (lane->stream) (void)hipStreamDestroy(lane->stream);
            delete lane;
        }
        (void)hipSetDevice(prev);
    }
};

/* A stream that a call makes for its own duration (engine::check_device, engine::streaming_lookup_host): on every way out it is
   drained, the scratch the replica keyed by it is handed back and it is destroyed. */
struct own_stream {
    device_replica const* rep;
    hipStream_t s = nullptr;
    explicit own_stream(device_replica const* r) : rep(r) { HIP_CHECK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking)); }
    own_stream(own_stream const&) = delete;
    own_stream& operator=(own_stream const&) = delete;
    ~own_stream() {
        (void)hipStreamSynchronize(s);
        rep->release_stream_scratch(s);
        (void)hipStreamDestroy(s);
    }
};

/* Device buffers freed on every way out of their scope: hipMalloc'ed and freed with hipFree, or -- given a replica and a stream --
   stream-ordered out of the replica's pool and freed with hipFreeAsync on that stream. */
class device_buffers {
public:
    device_buffers() = default;
    device_buffers(device_replica const* rep, hipStream_t s) : m_rep(rep), m_stream(s) {}
    device_buffers(device_buffers const&) = delete;
    device_buffers& operator=(device_buffers const&) = delete;
    ~device_buffers() {
        for (void* p : m_owned) free_one(p);
    }
    template <typename T>
    T* alloc(uint64_t n) {
        const size_t bytes = std::max<uint64_t>(n * sizeof(T), 8);
        void* p = nullptr;
        if (m_rep) p = m_rep->stream_alloc(bytes, m_stream);
        else HIP_CHECK(hipMalloc(&p, bytes));
        m_owned.push_back(p);
        return static_cast<T*>(p);
    }
    /* free one before the others */
    void release(void const* p) {
        for (void*& q : m_owned)
            if (q == p) {
                free_one(q);
                q = nullptr;
            }
    }
    /* hand a hipMalloc'ed buffer over to the replica, which frees it with the rest of its HBM */
    void keep(void const* p, device_replica& rep) {
        for (void*& q : m_owned)
            if (q == p) {
                rep.allocations.push_back(q);
                q = nullptr;
            }
    }

private:
    void free_one(void* p) const {
        if (!p) return;
        if (m_rep) (void)hipFreeAsync(p, m_stream);
        else (void)hipFree(p);
    }
    device_replica const* m_rep = nullptr;
    hipStream_t m_stream = nullptr;
    std::vector<void*> m_owned;
};

class engine;

/* data[i] = data[0] + .. + data[i - 1] for i < n, 64-bit words in place on `s` (streaming.hip: the scan of the runs' CSR); its tile
   sums are allocated and freed by the call, stream-ordered, from the replica's pool */
void exclusive_scan_words(device_replica const* rep, uint64_t* data, uint64_t n, hipStream_t s);

/* the devices holding a replica (engine::devices), or the error that there are none */
std::vector<int> resident_devices(engine const& eng);

/* Runs the lanes of a host-buffer entry point (engine.hip): lane i calls fn(i, devices[i], lane) with devices[i] current and a
   pooled lane of that device's replica of at least `bytes` -- on the calling thread when there is one lane, else on a thread
   each. Once every lane has finished, the caller's device is restored and the first exception (in lane order) rethrown;
   `failed`, when given, is set as soon as a lane throws. */
void run_lanes(engine const& eng, std::vector<int> const& devices, size_t bytes, std::function<void(size_t, int, host_lane&)> const& fn,
               std::atomic<bool>* failed = nullptr);

}  // namespace sshash_amd
