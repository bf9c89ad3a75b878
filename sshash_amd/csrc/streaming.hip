// streaming.hip -- batched streaming query (gfx950 only).
//
// Reference: streaming_query<Dict,canonical>::lookup / seed (include/streaming_query.hpp:56-109,
// 144-197) driven per read by src/query.cpp:78-108. The state machine is sequential inside a
// read and independent across reads, so reads are the parallel dimension (long reads are cut into segments first): a lane owns a read and
// handles its EVENTS -- a seed (one point lookup, through the super-k-mer table when the replica has
// one), or the run of extensions behind a hit, measured as a longest common prefix of the read and
// the strings, 32 bases a step (streaming_run_kernel below). With the granule layout the reference's
// `remaining_string_bases` counter is implicit: a string-start mark at the next base is exactly
// remaining == 0. The negative short-cut (:150-157) becomes "the k-mers behind a miss that elect the
// same table key, and cannot be in that key's slot either, are negative too" -- the same k-mers are
// negative either way, so the counters are unchanged.
// Output: the six counters of streaming_query_report (include/util.hpp:21-36), for the batch or -- the kernel's PER_READ form -- for every
// read on its own, or -- its run forms -- one record per run (a search and the extensions behind it: where the read hits) in CSR layout;
// per-k-mer results: the position-parallel pipeline further down.
#include <hip/hip_runtime.h>
#include <sys/stat.h>

#include <algorithm>
#include <atomic>
#include <cstring>
#include <exception>
#include <stdexcept>
#include <thread>

#include "engine.hpp"
#include "hooks.hpp"
#include "reads.hpp"
#include "replica.hpp"
#include "segments.hpp"

namespace sshash_amd {

namespace {

template <int W, bool CANON>
__device__ __forceinline__ hit_t seed_lookup(dict_view const& d, skew_part_dev const* __restrict__ skew,
                                             kmer_w<W> const& x, kmer_w<W> const& x_rc, minimizer_t mf, minimizer_t mr) {
    if constexpr (CANON) {  // include/streaming_query.hpp:159-169
        if (mf.value < mr.value) return probe_canonical<W, true>(d, skew, x, x_rc, mf);
        if (mr.value < mf.value) return probe_canonical<W, true>(d, skew, x, x_rc, mr);
        hit_t h = probe_canonical<W, true>(d, skew, x, x_rc, mf);
        if (!h.found) h = probe_canonical<W, true>(d, skew, x, x_rc, mr);
        return h;
    } else {  // :170-180
        hit_t h = probe_regular<W, true>(d, skew, x, mf);
        if (!h.found) {
            const bool mf_found = h.minimizer_found;
            h = probe_regular<W, true>(d, skew, x_rc, mr);
            h.orientation = -1;
            h.minimizer_found = h.minimizer_found || mf_found;
        }
        return h;
    }
}

__device__ __forceinline__ uint64_t wave_sum(uint64_t v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}

/* The continuation rule of a run (include/sshash_amd.h, "WHERE a read hits"), on the results of two neighbouring k-mers of a read: the
   second, a positive k-mer, continues the run of the first iff that one is positive, lies in the same string and its id moved by its
   orientation. The one statement of it: the classification, the run marks and the seams of a segmented launch all ask here. */
__device__ __forceinline__ bool continues_run(uint64_t id_before, uint64_t sid_before, int ori_before, uint64_t id, uint64_t sid) {
    return id_before != INVALID_U64 && sid_before == sid && id == id_before + uint64_t(int64_t(ori_before));
}

/* The counters of a workgroup (of 256) reach `report` with ONE set of atomics: the six counters share a cache line, and a set
   per wave -- 2 x 10^5 atomics on one line for 3 x 10^8 bases -- serialises at ~90 atomics/us (HISTORY.md). Called by
   every lane of the workgroup. */
__device__ __forceinline__ void block_report(uint64_t c_kmers, uint64_t c_invalid, uint64_t c_negative, uint64_t c_searches,
                                             uint64_t c_extensions, uint64_t* __restrict__ report) {
    __shared__ uint64_t partial[4][5];
    c_kmers = wave_sum(c_kmers);
    c_invalid = wave_sum(c_invalid);
    c_negative = wave_sum(c_negative);
    c_searches = wave_sum(c_searches);
    c_extensions = wave_sum(c_extensions);
    if ((threadIdx.x & 63) == 0) {
        uint64_t* mine = partial[threadIdx.x >> 6];
        mine[0] = c_kmers;
        mine[1] = c_invalid;
        mine[2] = c_negative;
        mine[3] = c_searches;
        mine[4] = c_extensions;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    uint64_t t[5];
    for (int j = 0; j < 5; ++j) t[j] = partial[0][j] + partial[1][j] + partial[2][j] + partial[3][j];
    if (t[0] == 0) return;
    atomicAdd(reinterpret_cast<unsigned long long*>(report + 0), (unsigned long long)t[0]);
    atomicAdd(reinterpret_cast<unsigned long long*>(report + 1), (unsigned long long)(t[3] + t[4]));
    atomicAdd(reinterpret_cast<unsigned long long*>(report + 2), (unsigned long long)t[2]);
    atomicAdd(reinterpret_cast<unsigned long long*>(report + 3), (unsigned long long)t[1]);
    atomicAdd(reinterpret_cast<unsigned long long*>(report + 4), (unsigned long long)t[3]);
    atomicAdd(reinterpret_cast<unsigned long long*>(report + 5), (unsigned long long)t[4]);
}

/* ==== the run-based streaming kernel (round 5) =====================================================================
   The per-base walk of rounds 1-4 (one read a lane, the lanes in step along their reads, k-mer and table key rolled base by base: HISTORY.md)
   spent its instructions where nothing is decided: 61 % of the k-mers of a high-hit read extend the
   run of the k-mer before them, and it rolled the k-mer, its reverse complement and two election candidates for every one of them,
   64 reads in step (397 vector instructions per base and wave; 48 G k-mers/s on that set, 104 on random reads, 37 on config C4's). A run is a longest common prefix: once a seed has put the read at
   offset `off` of the strings in orientation `o`, the next k-mers are extensions for as long as the read's NEXT BASE equals the
   strings' next base in that direction and no string starts there -- streaming_query.hpp:86-100 compares whole k-mers
   (`expected == kmer or expected == kmer_rc`), but given the k-mer before matched the strings' k-mer before, the two k-mers share
   k - 1 bases and differ or agree in the one new base; the other alternative of the reference's test can then only hold when the
   new bases agree as well:
       forward   F' = F[1:] + s, x' = x[1:] + r, F = x.   F' = rc(x') means y + s = comp(r) + rc(y) for y = x[1:]:  y[0] = comp(r),
                 y[i] = comp(y[k-2-(i-1)]) ..., s = comp(y[0]) = r.
       backward  F' = s + F[:-1], F = rc(x), rc(x') = comp(r) + F[:-1].   F' = x' means s + z = rc(z) + r for z = F[:-1]:
                 r = z[k-2], s = comp(z[k-2]) = comp(r).
   So the length of a run is min(longest common prefix of the read's tail and the strings -- 32 bases a step: XOR of two packed
   words and a count of trailing zeros --, bases left in the string, valid bases left in the read), and nothing per base is left.

   What remains are the SEEDS (the negative k-mers, and one search per run): 0.29 per base on the high-hit set, 0.41 on config
   C4's. The kernel is a loop over EVENTS, not over bases: in every turn every lane of a wave handles the next event of its own
   read -- a seed at its own position, or the extension that follows a hit -- so the lanes of a wave are no longer in step along
   their reads, and a lane that is done with its read takes the next one of its wave's share at once (the wave hands them out in
   order: a ballot and a prefix count, no atomics). The reads are packed to two bits a base (and a validity bit a base) by a pass
   of their own first: a seed cuts its k-mer out of two or three words, and the invalid k-mers around an `N` are counted and
   skipped with one subtraction (streaming_query.hpp:59-65: a k-mer is invalid iff one of its k characters is). */

/* pass 1: lane t packs bases [8t, 8t + 8): 16 bits of codes ((c >> 1) & 3, include/kmer.hpp:118; base i of a 32-base word in bits
   2i, 2i + 1) and 8 validity bits (A C G T a c g t, include/kmer.hpp:209-219) */
__global__ void __launch_bounds__(256)
stream_pack_kernel(const char* __restrict__ bases, const uint64_t total_bases, uint16_t* __restrict__ packed, uint8_t* __restrict__ okay) {
    const uint64_t t = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    const uint64_t at = 8 * t;
    if (at >= total_bases) return;
    uint64_t v = 0;
    if (at + 8 <= total_bases && ((reinterpret_cast<uintptr_t>(bases) + at) & 7) == 0) {
        v = *reinterpret_cast<const uint64_t*>(bases + at);
    } else {
        for (uint32_t b = 0; b < 8 && at + b < total_bases; ++b) v |= uint64_t(uint8_t(bases[at + b])) << (8 * b);
    }
    uint64_t two = (v >> 1) & 0x0303030303030303ULL;
    two = (two | (two >> 6)) & 0x000F000F000F000FULL;
    two = (two | (two >> 12)) & 0x000000FF000000FFULL;
    two = two | (two >> 24);
    const uint64_t u = v & 0xDFDFDFDFDFDFDFDFULL;  // fold the case
    auto nonzero = [](uint64_t z) { return ((z & 0x7F7F7F7F7F7F7F7FULL) + 0x7F7F7F7F7F7F7F7FULL) | z; };  // bit 7 of every byte that is not zero
    uint64_t ok = ~(nonzero(u ^ 0x4141414141414141ULL) & nonzero(u ^ 0x4343434343434343ULL) & nonzero(u ^ 0x4747474747474747ULL) &
                    nonzero(u ^ 0x5454545454545454ULL)) & 0x8080808080808080ULL;
    ok >>= 7;
    ok |= ok >> 7;
    ok |= ok >> 14;
    ok |= ok >> 28;
    packed[t] = uint16_t(two);
    okay[t] = uint8_t(ok);
}

/* first invalid base in [from, end), or `end` */
__device__ __forceinline__ uint64_t first_invalid_base(const uint64_t* __restrict__ okay, uint64_t from, uint64_t end) {
    uint64_t p = from;
    while (p < end) {
        const uint64_t bad = ~okay[p >> 6] >> (p & 63u);
        if (bad) {
            p += uint64_t(__builtin_ctzll(bad));
            break;
        }
        p = (p | 63u) + 1;
    }
    return p < end ? p : end;
}

/* first valid base in [from, end), or `end` */
__device__ __forceinline__ uint64_t first_valid_base(const uint64_t* __restrict__ okay, uint64_t from, uint64_t end) {
    uint64_t p = from;
    while (p < end) {
        const uint64_t good = okay[p >> 6] >> (p & 63u);
        if (good) {
            p += uint64_t(__builtin_ctzll(good));
            break;
        }
        p = (p | 63u) + 1;
    }
    return p < end ? p : end;
}

/* the 32 bases of the packed reads starting at base p */
__device__ __forceinline__ uint64_t read_bases32(const uint64_t* __restrict__ packed, uint64_t p) {
    const uint64_t i = p >> 5;
    return funnel_shr(packed[i], packed[i + 1], 2 * (uint32_t(p) & 31u));
}

/* the 32 bases of the strings starting at base p; mark bit j (0 .. 32): a string starts at base p + j */
template <int W>
__device__ __forceinline__ void string_bases32(dict_view const& d, uint64_t p, uint64_t& bases, uint64_t& marks) {
    const uint32_t rel = uint32_t(p) & 31u;
    if constexpr (W == 1) {
        const uint4* A = reinterpret_cast<const uint4*>(d.granules) + 2 * (p >> 5);
        const uint4 q0 = A[0], q1 = A[1];
        bases = funnel_shr(uint64_t(q0.x) | (uint64_t(q0.y) << 32), uint64_t(q0.z) | (uint64_t(q0.w) << 32), 2 * rel);
        marks = (uint64_t(q1.x) | (uint64_t(q1.y) << 32)) >> rel;
    } else {
        const uint4* G = reinterpret_cast<const uint4*>(d.granules) + (p >> 5);
        const uint4 g0 = G[0], g1 = G[1];
        bases = funnel_shr(uint64_t(g0.z) | (uint64_t(g0.w) << 32), uint64_t(g1.z) | (uint64_t(g1.w) << 32), 2 * rel);
        marks = (uint64_t(g0.y) | (uint64_t(g1.y) << 32)) >> rel;
    }
}

/* Length of the run behind a hit: the read's k-mer that ends at base `b` - 1 lies at offset `off` of the strings (orientation
   `ori`); at most `room` k-mers follow it inside the read's valid bases. Returns how many of them are extensions. */
/* One step of a run's measurement: the 32 bases of the strings that come next in the run's direction and the marks that stop it,
   next to the read's 32 bases from base b + run. Forward, the t-th extension gains the strings' base off + k - 1 + t and leaves its
   string iff a string starts there. Backward it gains the base off - t, complemented, and leaves its string iff a string starts at
   off - t + 1 (streaming_query.hpp:92: remaining_string_bases = kmer_id_in_string going backward): a step takes the `have` bases below
   `top` = off - run. Loads only: what they bring is looked at by run_step_length. */
struct run_step_t {
    uint64_t s, marks, read;
    uint32_t have;  // backward: how many bases lie below `top` (32, fewer at the very start of the strings; 0: none)
};

template <int W>
__device__ __forceinline__ run_step_t run_step_load(dict_view const& d, const uint64_t* __restrict__ packed, uint64_t off, bool forward,
                                                    uint64_t b, uint64_t run) {
    run_step_t t;
    const uint64_t top = off - run;
    t.have = forward || top >= 32 ? 32u : uint32_t(top);
    string_bases32<W>(d, forward ? off + d.k + run : top - t.have, t.s, t.marks);
    t.read = read_bases32(packed, b + run);
    return t;
}

/* how many of the (at most 32) extensions of a step hold: the strings' bases along the run -- backward: the `have` bases below `top`,
   the last of them moved to place 31, reversed and complemented: place i = comp(S[top - 1 - i]) -- against the read's, up to the first
   mark that stops the run -- bit 31 - i of `gate` stops extension i; backward the mark of base top - i: marks bit (have - i) */
__device__ __forceinline__ uint32_t run_step_length(run_step_t const& t, bool forward) {
    const uint64_t along = forward ? t.s : revcomp_word(t.s << ((2 * (32 - t.have)) & 63u));  // (have = 0: a shift by 64 is not one; the step is min(., have) = 0 whatever this gives)
    const uint64_t diff = along ^ t.read;
    const uint32_t same = diff ? uint32_t(__builtin_ctzll(diff)) >> 1 : 32u;
    const uint32_t gate = forward ? uint32_t(__brev(uint32_t(t.marks))) : uint32_t((t.marks >> 1) << (32 - t.have));
    const uint32_t inside = gate ? uint32_t(__builtin_clz(gate)) : 32u;
    const uint32_t step = same < inside ? same : inside;
    return step < t.have ? step : t.have;
}

/* Length of the run behind a hit: the read's k-mer that ends at base `b` - 1 lies at offset `off` of the strings (orientation `ori`);
   at most `room` k-mers follow it inside the read's valid bases; `first`: the first step's loads, asked for by the caller early in
   its turn so that they travel while the turn's bucket lines do. Returns how many of the following k-mers are extensions. */
template <int W>
__device__ __forceinline__ uint64_t extend_run(dict_view const& d, const uint64_t* __restrict__ packed, uint64_t off, int ori, uint64_t b,
                                               uint64_t room, run_step_t t) {
    const bool forward = ori > 0;
    uint64_t run = 0;
    for (;;) {
        uint64_t step = run_step_length(t, forward);
        if (step > room - run) step = room - run;
        run += step;
        if (step < 32 || run >= room) break;
        t = run_step_load<W>(d, packed, off, forward, b, run);
    }
    return run;
}

/* (the per-read form of the kernel below) the lane's counters into its read's row: stored, or -- `partial`: the row already holds a part
   of the read's counts -- added to what went there before; the counters start again at zero */
__device__ __forceinline__ void row_flush(uint64_t* __restrict__ row, bool partial, uint32_t& c_invalid, uint32_t& c_negative, uint32_t& c_searches,
                                          uint32_t& c_extensions) {
    const uint64_t s = c_searches, e = c_extensions;
    if (partial) {
        row[1] += s + e;
        row[2] += c_negative;
        row[3] += c_invalid;
        row[4] += s;
        row[5] += e;
    } else {
        row[1] = s + e;
        row[2] = c_negative;
        row[3] = c_invalid;
        row[4] = s;
        row[5] = e;
    }
    c_invalid = c_negative = c_searches = c_extensions = 0;
}

/* (five waves a SIMD: 96 registers. Round 5's steps there, same-box: k <= 31 four -> five waves 110 -> 126 G k-mers/s; k <= 63, once 32-bit
   counters and a run measurement without early loads had made room, 138 -> 147 with 20 bytes of scratch. Compiled for six: 14 / 31 % slower,
   profiles/r05/streaming_run_kernel_waves_per_simd_ab.txt.) */
#ifndef SSHASH_STREAM_WAVES
#define SSHASH_STREAM_WAVES 5
#endif
/* PER_READ: one streaming_query_report PER READ instead of one for the batch -- `report` is then the array of ROWS, six words a read
   in the order of the batch's report (num_kmers, positive, negative, invalid, searches, extensions), row r for read r. The lane that
   takes read r owns row r until it takes its next read, and every counter it bumps in between belongs to that read: the row is
   written by that lane alone, with plain stores, no atomics. num_kmers is stored at the hand-out, the other five when the read is
   done (the lane's 32-bit counters are then exactly the read's). The two ways a count leaves the lane's counters early -- the move-out
   every `move_out_every` turns, and a run or a stretch of invalid k-mers of 2^15 and more -- put it into the row early instead, and
   mark the row (ROW_PARTIAL): what follows is ADDED to such a row (a load, an add, a store -- a dependent round trip that the common
   read never pays). A read shorter than k gets its six zeros at the hand-out and is never anybody's. No batch totals here: they are
   the column sums of the rows (stream_rows_sum_kernel). */
/* MODE (what leaves the kernel besides, or instead of, the batch's six counters):
     STREAM_TOTALS       the six counters of the batch;
     STREAM_ROWS         PER_READ, above;
     STREAM_RUN_COUNTS   the six counters of the batch as STREAM_TOTALS, and for every read the number of its RUNS -- a run is a search
                         and the extensions behind it, so a read has as many as it has searches -- at sink.run_offsets[r] (one plain
                         store when the read is done: a count per read that never leaves the lane early, in a register of its own);
     STREAM_RUN_RECORDS  one sshash_streaming_run per run (include/sshash_amd.h), no counters: the lane that takes read r starts its
                         cursor at sink.run_offsets[r] -- the counts of a STREAM_RUN_COUNTS launch over the same reads, scanned -- and
                         stores the record of every hit where its run has been measured (top of the turn after the hit; a hit that
                         nothing can follow: where it is found), two 16-byte stores, nothing at or beyond sink.capacity and nothing at
                         or beyond run_offsets[r + 1]. The hit's string travels across the turn in one more register.
     STREAM_COVER        the six counters of the batch as STREAM_TOTALS, and WHICH k-mers of the dictionary the reads hold: where the record form
                         stores a run's record this one marks the run's range of k-mer ids in the bitmap at sink.records (cover_mark: bit
                         i & 63 of word i >> 6 for k-mer id i) -- the hit's string travels across the turn as there (kmer_id = off - sid * (k - 1)).
                         One launch: no count per read, no cursor, no run_offsets, and sink.capacity means nothing.
     STREAM_DEPTH        the six counters of the batch as STREAM_TOTALS, and HOW OFTEN the reads hold each k-mer of the dictionary, as a difference
                         array: where the cover form marks a run's range of ids [lo, hi) this one adds +1 to word lo and -1 to word hi of the
                         32-bit deltas at sink.records (depth_mark_run; hi = num_kmers: no word, nothing added) -- one or two atomics a run,
                         whatever its length; the inclusive prefix sum of the deltas (inclusive_scan_u32) is the depth. One launch, as the cover.
     STREAM_SUMS         the six counters of the batch as STREAM_TOTALS, and PER READ the sum of a value per k-mer over the read's positive
                         k-mers, and their number: over the 64-bit exclusive prefix sums P of the values at sink.values_prefix a run of ids
                         [lo, hi) is worth P[hi] - P[lo], two loads whatever its length. Where the depth form adds its +1 / -1 this one adds
                         that difference and the run's length to the two words of the read's row at sink.records (sums_add: two 64-bit
                         atomics without return into rows the caller zeroed). The lane keeps the index of its row, one register, counted
                         from the row of its wave's first read (sink.read_of: the read of every segment, for reads cut into segments,
                         whose lanes then share rows -- addition commutes). One launch, as the depth.
     STREAM_CLASSES      the six counters of the batch as STREAM_TOTALS, and PER READ its positive k-mers BY CLASS OF STRING: a run lies in
                         one string, so it is worth its length in one column -- the label of its string (sink.labels: one 32-bit word
                         per string id) -- of its read's row of sink.num_classes 32-bit words at sink.records; a label at or above
                         that count is no class and adds nothing. The sums form with another add (classes_add: ONE 32-bit atomic without
                         return into rows the caller zeroed, one 4-byte load a run whatever its length); the row's index is kept as
                         there, sink.read_of included. One launch.
     STREAM_BEST_RUN     the six counters of the batch as STREAM_TOTALS, and PER READ its LONGEST RUN (among equals the first in read
                         order) as one sshash_streaming_run at sink.records, record r for read r, into records the caller zeroed: the
                         lane owns its read, keeps the length of the longest run it has stored for it in one register (best_len, zero
                         when it takes a read) and, where a run is measured, stores the run's record over the read's -- the record
                         form's two 16-byte stores (run_record_write), plain, no atomics -- when the run is LONGER; runs come in the
                         order of their place in the read, so the first of equals stays. The hit's string travels across the turn as
                         in the record form, the read's index as in the counting form. Never over segments: a longest run is not
                         additive. One launch.
     STREAM_RUN_RECORDS_SEGMENTS  the record form over a segment table ("the run RECORDS over segments" below): the lane that takes
                         segment g starts its cursor at sink.run_offsets[g] -- here E[g], the final index of the first record that
                         STARTS in the segment --; the first run of a segment whose seam is joined is the tail of a record that a
                         segment before it stores: not stored, its length to cont[g] for the merge; every other run is a record,
                         its read_pos counted from the begin of the READ (sink.read_of, and the reads' offsets in the word of
                         sink.values_prefix). A form of its own, not a branch of the record form: that one's code stays what it was. */
enum : int {
    STREAM_TOTALS = 0, STREAM_ROWS = 1, STREAM_RUN_COUNTS = 2, STREAM_RUN_RECORDS = 3, STREAM_COVER = 4, STREAM_DEPTH = 5, STREAM_SUMS = 6,
    STREAM_CLASSES = 7, STREAM_BEST_RUN = 8, STREAM_RUN_RECORDS_SEGMENTS = 9
};

/* the record (sshash_streaming_run, 32 bytes) of the run of `n` k-mers of read `r` whose first (in read order) starts at base `at` of the
   packed reads and lies at offset `off` of the strings, in string `sid`, to place `index` of `records`: two 16-byte stores, one 8-byte
   load of the string's begin. The one statement of what a record holds: the record form and the best-run form both store through it. */
__device__ __forceinline__ void run_record_write(dict_view const& d, void* records, uint64_t index, const uint64_t* __restrict__ begins, uint64_t r, uint64_t at,
                                                 uint64_t off, uint32_t sid, int ori, uint64_t n) {
    const uint64_t kmer_id = off - uint64_t(sid) * (d.k - 1), in_string = off - d.endpoints[sid];  // (store_result, lookup_device.hpp)
    const uint32_t read_pos = uint32_t(at - begins[r]), length = uint32_t(n) | (ori > 0 ? 0u : 0x80000000u);
    uint4* const rec = static_cast<uint4*>(records) + 2 * index;
    rec[0] = make_uint4(uint32_t(kmer_id), uint32_t(kmer_id >> 32), sid, 0u);
    rec[1] = make_uint4(uint32_t(in_string), uint32_t(in_string >> 32), read_pos, length);
}

/* that record to place `cursor` of the records, unless that is past what the read or the caller has room for */
__device__ __forceinline__ void run_record_store(dict_view const& d, run_sink const& sink, const uint64_t* __restrict__ begins, uint64_t r,
                                                 uint64_t cursor, uint64_t at, uint64_t off, uint32_t sid, int ori, uint64_t n) {
    if (cursor >= sink.capacity || cursor >= sink.run_offsets[r + 1]) return;
    run_record_write(d, sink.records, cursor, begins, r, at, off, sid, ori, n);
}

/* (the record form over segments) where the lanes find what lies behind E in the scratch (segments.hpp: segment_runs_scratch), from E
   and the number of entries alone: the sink is as large as it was */
__device__ __forceinline__ uint32_t* seg_runs_cont(run_sink const& sink, uint64_t bound) { return reinterpret_cast<uint32_t*>(sink.run_offsets + bound + 1); }
__device__ __forceinline__ const uint8_t* seg_runs_joined(run_sink const& sink, uint64_t bound) {
    return reinterpret_cast<const uint8_t*>(sink.run_offsets + bound + 1 + segment_runs_cont_words(bound));
}

/* (the record form over segments) the run of segment `g` to place `cursor`, under the guards of run_record_store -- the caller's room, and
   the place where the records that start in the next segment begin --, its position counted from the begin of its read */
__device__ __forceinline__ void seg_record_store(dict_view const& d, run_sink const& sink, uint64_t g, uint64_t cursor, uint64_t at, uint64_t off,
                                                 uint32_t sid, int ori, uint64_t n) {
    if (cursor >= sink.capacity || cursor >= sink.run_offsets[g + 1]) return;
    run_record_write(d, sink.records, cursor, sink.values_prefix /* the reads' offsets */, sink.read_of[g], at, off, sid, ori, n);
}

/* (the best-run form) the same run over the record of its read, record `r` of sink.records, when it is longer than the longest stored for
   that read so far, whose length the lane keeps in `best_len`: strictly longer, so of equals the first in read order stays */
__device__ __forceinline__ void best_run_store(dict_view const& d, run_sink const& sink, const uint64_t* __restrict__ begins, uint64_t r,
                                               uint32_t& best_len, uint64_t at, uint64_t off, uint32_t sid, int ori, uint64_t n) {
    if (n <= best_len) return;
    best_len = uint32_t(n);  // (a read has fewer than 2^31 bases: the precondition of the run records)
    run_record_write(d, sink.records, r, begins, r, at, off, sid, ori, n);
}

/* the k-mer ids [lo, hi), hi > lo, into the bitmap: an atomic OR (nothing comes back: the lane does not wait for it) for the first and the
   last word -- other runs may end in them --, a plain store for the words in between: whoever else touches such a word ORs into it or
   stores the same all-ones, and all-ones is what every order of those leaves behind. Ids at or above num_kmers are in no run. */
__device__ __forceinline__ void cover_mark(uint64_t* __restrict__ cover, uint64_t lo, uint64_t hi) {
    const uint64_t w0 = lo >> 6, w1 = (hi - 1) >> 6;
    const unsigned long long first = ~0ULL << (lo & 63u), last = ~0ULL >> (63u - (uint32_t(hi - 1) & 63u));
    unsigned long long* const words = reinterpret_cast<unsigned long long*>(cover);
    if (w0 == w1) {
        (void)__hip_atomic_fetch_or(words + w0, first & last, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return;
    }
    (void)__hip_atomic_fetch_or(words + w0, first, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    for (uint64_t w = w0 + 1; w < w1; ++w) words[w] = ~0ULL;
    (void)__hip_atomic_fetch_or(words + w1, last, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

/* the run of `n` k-mers whose first (in read order) lies at offset `off` of the strings, in string `sid`: forward its ids go up from that
   k-mer's, backward down (run_record_store: the same run as a record) */
__device__ __forceinline__ void cover_mark_run(dict_view const& d, run_sink const& sink, uint64_t off, uint32_t sid, int ori, uint64_t n) {
    const uint64_t kmer_id = off - uint64_t(sid) * (d.k - 1);
    const uint64_t lo = ori > 0 ? kmer_id : kmer_id + 1 - n;
    cover_mark(static_cast<uint64_t*>(sink.records), lo, lo + n);
}

/* the same run into the deltas of a depth array (num_kmers words of 32 bits, arithmetic modulo 2^32): +1 where its ids begin, -1 behind
   them unless that is behind the array. Nothing comes back: the lane does not wait for either. */
__device__ __forceinline__ void depth_mark_run(dict_view const& d, run_sink const& sink, uint64_t off, uint32_t sid, int ori, uint64_t n) {
    const uint64_t kmer_id = off - uint64_t(sid) * (d.k - 1);
    const uint64_t lo = ori > 0 ? kmer_id : kmer_id + 1 - n, hi = lo + n;
    uint32_t* const deltas = static_cast<uint32_t*>(sink.records);
    (void)__hip_atomic_fetch_add(deltas + lo, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (hi < d.num_kmers) (void)__hip_atomic_fetch_add(deltas + hi, ~0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

/* the same run into the row of its read (two words of 64 bits, arithmetic modulo 2^64): what the values of its ids [lo, hi) sum to --
   P[hi] - P[lo] -- and its length. The `anchor` is the one of the two words that does not depend on the run's length, P[lo] forward and
   P[hi] backward: asked for before the run is measured. Nothing comes back from the adds: the lane does not wait for either. */
__device__ __forceinline__ uint64_t sums_run_anchor(dict_view const& d, run_sink const& sink, uint64_t off, uint32_t sid, int ori) {
    const uint64_t kmer_id = off - uint64_t(sid) * (d.k - 1);
    return sink.values_prefix[ori > 0 ? kmer_id : kmer_id + 1];
}
/* the other of the two: P[hi] forward, P[lo] backward, known once the run is measured */
__device__ __forceinline__ uint64_t sums_run_far(dict_view const& d, run_sink const& sink, uint64_t off, uint32_t sid, int ori, uint64_t n) {
    const uint64_t kmer_id = off - uint64_t(sid) * (d.k - 1);
    return sink.values_prefix[ori > 0 ? kmer_id + n : kmer_id + 1 - n];  // (at most num_kmers: P holds num_kmers + 1 words)
}
/* `above` - `below` (P[hi] - P[lo]) and the run's length n into the row */
__device__ __forceinline__ void sums_add(run_sink const& sink, uint64_t row, uint64_t above, uint64_t below, uint64_t n) {
    const uint64_t sum = above - below;
    unsigned long long* const words = static_cast<unsigned long long*>(sink.records) + 2 * row;
    if (sum) (void)__hip_atomic_fetch_add(words, (unsigned long long)sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    (void)__hip_atomic_fetch_add(words + 1, (unsigned long long)n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

/* the classes form's sink (engine.hpp: run_sink): rows at `records`, their width in `num_classes`, the labels at `labels` */
inline run_sink class_sink(uint32_t const* labels, uint32_t classes, uint32_t* rows) {
    run_sink sink{nullptr, rows, 0, nullptr, nullptr};
    sink.num_classes = classes;
    sink.labels = labels;
    return sink;
}

/* the same run into the column of its string's class (rows of sink.num_classes words of 32 bits, arithmetic modulo 2^32): its length,
   whatever its ids are. A label at or above the number of classes is no class: nothing is added. Nothing comes back from the add. */
__device__ __forceinline__ void classes_add(run_sink const& sink, uint64_t row, uint32_t label, uint64_t n) {
    const uint32_t classes = uint32_t(sink.num_classes);
    if (label >= classes) return;
    uint32_t* const word = static_cast<uint32_t*>(sink.records) + row * classes + label;
    (void)__hip_atomic_fetch_add(word, uint32_t(n), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

/* The reads are given by a begin and an end pointer: read r spans the bases [begins[r], ends[r]) of the packed copy. For whole reads the two
   are `offsets` and `offsets + 1` -- the two words the kernel has always loaded --; for long reads cut into segments they are the two
   arrays of the segment table, and a "read" of the kernel is a segment ("long reads: SEGMENTS" below). */
template <int W, bool CANON, bool SK, int MODE>
__global__ void __launch_bounds__(256, SSHASH_STREAM_WAVES)
streaming_run_kernel(const dict_view d, const skew_part_dev* __restrict__ skew, const uint64_t* __restrict__ packed,
                     const uint64_t* __restrict__ okay, const uint64_t* __restrict__ begins, const uint64_t* __restrict__ ends, const uint64_t n_reads,
                     const uint64_t reads_per_wave, const uint32_t move_out_every, uint64_t* __restrict__ report, const run_sink sink) {
    constexpr bool SEG_RECORDS = MODE == STREAM_RUN_RECORDS_SEGMENTS;  // (RECORDS as well: what the two forms share says RECORDS)
    constexpr bool PER_READ = MODE == STREAM_ROWS, COUNT_RUNS = MODE == STREAM_RUN_COUNTS, RECORDS = MODE == STREAM_RUN_RECORDS || SEG_RECORDS, COVER = MODE == STREAM_COVER,
                   DEPTH = MODE == STREAM_DEPTH, SUMS = MODE == STREAM_SUMS, CLASSES = MODE == STREAM_CLASSES, BEST_RUN = MODE == STREAM_BEST_RUN;
    constexpr bool ROW_INDEX = SUMS || CLASSES;  // the lane keeps the index of its read's row, counted from row_first
    /* (SUMS) when a measured run's two words of P are added to its row: at the end of the turn -- by then the seed's own loads have been
       waited for, and these with them -- or where the run is measured, which makes the wave wait for them there. Late costs seven
       registers across the turn. Measured, 2 x 10^7 reads of 150 bases with the table: at k <= 31 late 15.85 ms against 16.56, at
       k <= 63, where the kernel spills as it is (72 bytes of scratch; late: 92), 13.76 against 12.58. */
    constexpr bool LATE_SUMS = SUMS && W == 1;
    /* (CLASSES) added where the run is measured, at every W. What made the late add pay for the sums at k <= 31 is absent here: there
       the second word of P depends on the run's length, is asked for behind the run's own loads and has to be waited for before the
       add. The label depends on the hit alone: it is asked for before the run is measured (as sums_run_anchor), the loads of a wave
       come back in the order they were issued, so it is there when the run's last load is, and the add -- which returns nothing --
       waits for no load of its own. A late add would carry the label, the length and the row (three registers) across the turn in
       a kernel that is at its 96 with the table, to save a wait that does not exist. No late variant was built; measured as it is,
       same reads, 4 classes: 14.94 ms at k <= 31 beside the sums form's 15.85 (late), 12.19 at k <= 63 beside its 12.36 (early). */
    __shared__ uint4 stage[SK ? 4 * 256 : 1];  // a wave's 64 bucket lines on their way from the quads that fetch them to the lanes that own them
    uint4* const wave_stage = stage + (SK ? (threadIdx.x >> 6) * 256 : 0);
    /* the counters are 32 bits wide in the lanes (six registers fewer than five 64-bit ones: with them the k <= 63 kernel fits five waves a
       SIMD); every 2^16 turns -- long before one could wrap -- the wave moves them into 64-bit totals of its own in LDS */
    __shared__ unsigned long long moved_out[4][5];
    uint32_t c_invalid = 0, c_negative = 0, c_searches = 0, c_extensions = 0;  // (the k-mers of a read go straight to the wave's total)
    const uint32_t k = d.k;
    const uint32_t lane = threadIdx.x & 63u;
    unsigned long long* const wave_moved_out = moved_out[threadIdx.x >> 6];
    if constexpr (!PER_READ && !RECORDS) {
        if (lane < 5) wave_moved_out[lane] = 0;
    }
    /* this wave's share of the reads, handed out in order to whichever lane is done with its read */
    const uint64_t wave = uint64_t(blockIdx.x) * (blockDim.x >> 6) + (threadIdx.x >> 6);
    uint64_t next = wave * reads_per_wave, last = next + reads_per_wave;
    if (next > n_reads) next = n_reads;
    if (last > n_reads) last = n_reads;
    uint64_t cur = 0, rd_end = 0, inv = 0;  // the k-mer to settle starts at base cur of the read that ends at rd_end; inv: first invalid base >= cur
    bool pending = false;                   // the k-mer before cur was found at `off`, orientation `ori`: the run behind it is to be measured
    uint64_t off = 0;
    int ori = 1;
    bool neg_unknown_mini = false;          // (no table) streaming_query.hpp:150-157
    uint64_t prev_f = 0, prev_r = 0;
    /* a seed whose probe has to go on past its key's first bucket is WALKING: its k-mer, its key and where the walk stands are kept
       from turn to turn. `where`: the choice of the sequence it is on | flags | the choice of the key's sequence to come back to */
    constexpr uint32_t WALK_CHOICE = 7u, WALK_COMPACT = 8u, WALK_VISITED = 16u, WALK_BACK_SHIFT = 8u, WALK_NO_RETURN = 7u;
    constexpr uint32_t WALK_LASTS_SHIFT = 16u, WALK_LASTS = 63u;  // what the slots met so far allow (min over the walk; 63: anything)
    /* A HEAVY key remembered (round 6). The k-mers of a heavy key are entered under keys of their own, and a seed learns that from the key's
       marker: one bucket for the marker, another -- a turn later -- on the k-mer's own sequence. Over a substitution inside a repeat every one
       of the k (negative) k-mers paid both, and none stands for its neighbours: on the high-hit set a fifth of all lane-turns were such
       second turns (profiles/r06/streaming_lane_occupancy_per_turn.txt). The k-mers that FOLLOW along the read and elect the same key
       occurrence (sk_key_persists) would walk the same buckets of the key's sequence up to the same marker; if none of those buckets holds
       an inline slot with the key's fingerprint (WALK_INLINE: then nothing in them can answer any k-mer of this key) they may start where
       that walk ended: on their own sequence, with the same choice of the key's sequence to come back to. Fields of `where` that outlive
       the seed: how many following k-mers may still do so, and that choice. */
    constexpr uint32_t WALK_INLINE = 32u, WALK_HEAVY_BACK_SHIFT = 11u, WALK_HEAVY_SHIFT = 24u, WALK_HEAVY = 63u, WALK_HEAVY_PENDING = 1u << 30;
    constexpr uint32_t WALK_HEAVY_FIELDS = (7u << WALK_HEAVY_BACK_SHIFT) | (WALK_HEAVY << WALK_HEAVY_SHIFT) | WALK_HEAVY_PENDING;
    bool walking = false;
    kmer_w<W> x = kmer_zero<W>(), x_rc = kmer_zero<W>();
    sk_key_t kk{};
    uint64_t on = 0, on_a = 0;
    uint32_t where = 0;
    uint32_t turns = 0;
    /* (PER_READ) the read this lane is on, counted from the wave's first -- one register: a wave's share is far below 2^31 reads --, and
       whether its row already holds a part of its counts */
    constexpr uint32_t ROW_NONE = ~0u, ROW_PARTIAL = 1u << 31;
    uint32_t my_row = ROW_NONE;
    /* (the run forms) the runs of the lane's read so far; where its next record goes; the string of the hit whose run is to be measured */
    uint32_t n_runs = 0, hit_sid = 0;
    uint64_t cursor = 0;
    uint32_t best_len = 0;  // (BEST_RUN) the length of the longest run stored for the lane's read so far
    bool seam_open = false;  // (SEG_RECORDS) the lane's segment begins inside a run, and that run -- its first -- is still to come
    const uint64_t wave_first = wave * reads_per_wave;
    /* (SUMS) the row of the wave's first read: the read itself, or -- segments -- the read of that segment (an empty entry of the table,
       behind the last segment: then so are all of the wave's, and none of them has a k-mer to add) */
    uint64_t row_first = wave_first;
    uint64_t late_anchor = 0, late_far = 0, late_n = 0;  // (SUMS) a measured run whose two words of P are on their way: sums_add at the end of the turn
    uint32_t late_row = 0;
    bool late_forward = true;
    if constexpr (ROW_INDEX) {
        if (sink.read_of) row_first = wave_first < n_reads ? sink.read_of[wave_first] : 0;
    }
    uint64_t* const wave_rows = report + wave * reads_per_wave * 6;  // (PER_READ) the row of the wave's first read
#ifdef SSHASH_STREAM_STATS
    /* (a debug build, tools/jobs/r06_stream_stats.sh: what the lanes of a wave do per turn -- wave-level sums in scalar registers, out
       through report[6 ..]; the caller's report has 16 entries then) */
    unsigned long long st_turns = 0, st_fresh = 0, st_walk = 0, st_ext = 0, st_slot1 = 0, st_inv = 0, st_idle = 0, st_full = 0, st_short = 0;
    uint64_t st_kept_lane = 0;
#define STAT(var, pred) var += (unsigned long long)__popcll(__ballot(pred))
#else
#define STAT(var, pred) (void)0
#endif
    for (;;) {
#ifdef SSHASH_STREAM_STATS
        ++st_turns;
#endif
        if (++turns >= move_out_every) {  // (scalar; a turn adds less than 2^15 to a lane's counter -- a longer run of extensions or of invalid k-mers goes to the wave's 64-bit totals at once --, so 2^16 turns stay below 2^31)
            turns = 0;
            if constexpr (PER_READ) {
                if (my_row != ROW_NONE) {
                    row_flush(wave_rows + uint64_t(my_row & ~ROW_PARTIAL) * 6, (my_row & ROW_PARTIAL) != 0, c_invalid, c_negative, c_searches, c_extensions);
                    my_row |= ROW_PARTIAL;
                }
            } else if constexpr (!RECORDS) {
                const uint64_t i = wave_sum(c_invalid), n = wave_sum(c_negative), f = wave_sum(c_searches), e = wave_sum(c_extensions);
                if (lane == 0) {
                    wave_moved_out[0] += i;
                    wave_moved_out[1] += n;
                    wave_moved_out[2] += f;
                    wave_moved_out[3] += e;
                }
                c_invalid = c_negative = c_searches = c_extensions = 0;
            }
        }
        /* -- the run behind the hit of the turn before, THEN this turn's seed (round 6): the lane measures its run and goes straight on to
              whatever lies behind it in the same turn -- the negative over the substitution that ended the run, as a rule; the NEXT READ when
              the run reached the end of this one (which is why the run comes before the reads are handed out). Until round 5 a lane did one
              or the other in a turn (the run's first loads travelled beside the seeds' bucket lines: one wait for both), and a hit -- run --
              miss cycle took a turn more than it has events (that order, as a build of this file, is the "run after seed" column of
              profiles/r06/streaming_*_ab.txt). (`pending` is only set when the k-mer behind the hit lies inside the read's
              valid bases: no test of its own here.) -- */
        STAT(st_ext, pending);
        if (pending) {
            const uint64_t b = cur + k - 1, valid_end = inv < rd_end ? inv : rd_end;
            uint64_t anchor = 0;
            if constexpr (SUMS) anchor = sums_run_anchor(d, sink, off, hit_sid, ori);  // (on its way while the run is measured)
            uint32_t label = 0;
            if constexpr (CLASSES) label = sink.labels[hit_sid];  // (likewise)
            const uint64_t run = extend_run<W>(d, packed, off, ori, b, valid_end - b, run_step_load<W>(d, packed, off, ori > 0, b, 0));
            if constexpr (CLASSES) classes_add(sink, row_first + my_row, label, run + 1);
            if constexpr (COVER) cover_mark_run(d, sink, off, hit_sid, ori, run + 1);
            if constexpr (DEPTH) depth_mark_run(d, sink, off, hit_sid, ori, run + 1);
            if constexpr (SUMS && !LATE_SUMS) {
                const uint64_t far = sums_run_far(d, sink, off, hit_sid, ori, run + 1);
                sums_add(sink, row_first + my_row, ori > 0 ? far : anchor, ori > 0 ? anchor : far, run + 1);
            }
            if constexpr (LATE_SUMS) {
                /* asked for here, added at the end of the turn (or of the kernel). The row goes along: the lane may take its next read in between. */
                late_far = sums_run_far(d, sink, off, hit_sid, ori, run + 1);  // (neither word is looked at here, not even to tell which is which)
                late_anchor = anchor;
                late_forward = ori > 0;
                late_n = run + 1;
                late_row = my_row;
            }
            if constexpr (BEST_RUN) best_run_store(d, sink, begins, wave_first + my_row, best_len, cur - 1, off, hit_sid, ori, run + 1);  // (beside the counting below, not instead of it)
            if constexpr (SEG_RECORDS) {
                if (seam_open) {  // (the tail of a record stored by a segment before: its length for the merge, no record, no place taken)
                    seg_runs_cont(sink, n_reads)[wave_first + my_row] = uint32_t(run + 1);
                    seam_open = false;
                } else {
                    seg_record_store(d, sink, wave_first + my_row, cursor, cur - 1, off, hit_sid, ori, run + 1);
                    ++cursor;
                }
            } else if constexpr (RECORDS) {  // (the hit lies a base before cur)
                run_record_store(d, sink, begins, wave_first + my_row, cursor, cur - 1, off, hit_sid, ori, run + 1);
                ++cursor;
            } else if (run >> 15) {  // (past what the lane's 32-bit counter may take in one turn: 2^16 turns lie between two move-outs)
                if constexpr (PER_READ) {  // (into the row at once, behind what the lane has counted for it so far)
                    uint64_t* const row = wave_rows + uint64_t(my_row & ~ROW_PARTIAL) * 6;
                    row_flush(row, (my_row & ROW_PARTIAL) != 0, c_invalid, c_negative, c_searches, c_extensions);
                    my_row |= ROW_PARTIAL;
                    row[1] += run;
                    row[5] += run;
                } else {
                    atomicAdd(wave_moved_out + 3, (unsigned long long)run);
                }
            } else {
                c_extensions += uint32_t(run);
            }
            cur += run;
            if (run) where &= ~WALK_HEAVY_FIELDS;  // (the k-mer behind a run elects a key of its own)
        }
        pending = false;
        /* -- the reads: whoever has none left takes the next of the wave's share -- */
        const bool want = !walking && cur + k > rd_end;
        const uint64_t wants = __ballot(want);
        if constexpr (PER_READ) {
            if (want && my_row != ROW_NONE) {  // (not walking, no k-mer left, the run behind the last hit measured above: the read is done)
                row_flush(wave_rows + uint64_t(my_row & ~ROW_PARTIAL) * 6, (my_row & ROW_PARTIAL) != 0, c_invalid, c_negative, c_searches, c_extensions);
                my_row = ROW_NONE;
            }
        }
        if constexpr (COUNT_RUNS) {
            if (want && my_row != ROW_NONE) {  // (the read is done, as above: its count)
                sink.run_offsets[wave_first + my_row] = n_runs;
                n_runs = 0;
                my_row = ROW_NONE;
            }
        }
        if (wants != 0 && next < last) {
            const uint64_t rank = uint64_t(__popcll(wants & ((uint64_t(1) << lane) - 1)));
            if (want && rank < last - next) {
                const uint64_t r = next + rank;
                cur = begins[r];
                rd_end = ends[r];
                if constexpr (PER_READ) {
                    uint64_t* const row = report + r * 6;
                    const uint64_t kmers = rd_end - cur >= k ? rd_end - cur - k + 1 : 0;
                    row[0] = kmers;
                    if (kmers) {
                        my_row = uint32_t(r - wave * reads_per_wave);
                    } else {  // (nothing will ever be counted for it: the whole row now)
                        row[1] = row[2] = row[3] = row[4] = row[5] = 0;
                    }
                } else if constexpr (COUNT_RUNS) {
                    if (rd_end - cur >= k) {
                        atomicAdd(wave_moved_out + 4, (unsigned long long)(rd_end - cur - k + 1));
                        my_row = uint32_t(r - wave_first);
                    } else {  // (no k-mer, no run)
                        sink.run_offsets[r] = 0;
                    }
                } else if constexpr (RECORDS) {
                    my_row = uint32_t(r - wave_first);
                    cursor = sink.run_offsets[r];
                    if constexpr (SEG_RECORDS) {  // (every entry of the table: an empty one is joined to nothing)
                        seam_open = seg_runs_joined(sink, n_reads)[r] != 0;
                        seg_runs_cont(sink, n_reads)[r] = 0;  // (a joined segment's first run stores its length over this, the same lane, later)
                    }
                } else if constexpr (BEST_RUN) {
                    if (rd_end - cur >= k) {  // (a read without a k-mer has no run: its record keeps the caller's zeros)
                        atomicAdd(wave_moved_out + 4, (unsigned long long)(rd_end - cur - k + 1));
                        my_row = uint32_t(r - wave_first);
                        best_len = 0;
                    }
                } else if constexpr (ROW_INDEX) {
                    if (rd_end - cur >= k) {  // (a read without a k-mer adds nothing: its row keeps the caller's zeros)
                        atomicAdd(wave_moved_out + 4, (unsigned long long)(rd_end - cur - k + 1));
                        my_row = uint32_t((sink.read_of ? sink.read_of[r] : r) - row_first);
                    }
                } else {
                    if (rd_end - cur >= k) atomicAdd(wave_moved_out + 4, (unsigned long long)(rd_end - cur - k + 1));
                }
                inv = first_invalid_base(okay, cur, rd_end);
                neg_unknown_mini = false;
                where = 0;
            }
            const uint64_t taken = uint64_t(__popcll(wants));
            next = taken < last - next ? next + taken : last;
        }
        bool live = cur + k <= rd_end;
        if (next >= last && __ballot(live) == 0) break;
        /* -- the k-mers over an invalid base: all invalid (streaming_query.hpp:59-65), counted and skipped -- a whole RUN of invalid
              bases a step: every k-mer that starts at or before the run's last base holds one of them (those from `cur` on reach
              `inv`: cur + k > inv). (Round 5 advanced one invalid base per iteration, each with a dependent load, the other 63 lanes
              waiting: a read with a long run of N was a cliff) -- */
        uint32_t c_invalid_turn = 0;
        STAT(st_inv, live && cur + k > inv);
        while (live && cur + k > inv) {
            const uint64_t nv = first_valid_base(okay, inv + 1, rd_end);  // the run of invalid bases is [inv, nv)
            const uint64_t last_over_it = nv - 1 < rd_end - k ? nv - 1 : rd_end - k;
            const uint64_t over = last_over_it - cur + 1;
            /* (a turn may add 2^15 - 1 to a lane's 32-bit counter and no more -- 2^16 turns lie between two move-outs --; this loop
               can cross a whole read in one turn, so what it adds is bounded by the loop's own sum, kept here) */
            if ((over + c_invalid_turn) >> 15) {
                if constexpr (PER_READ) {
                    uint64_t* const row = wave_rows + uint64_t(my_row & ~ROW_PARTIAL) * 6;
                    row_flush(row, (my_row & ROW_PARTIAL) != 0, c_invalid, c_negative, c_searches, c_extensions);
                    my_row |= ROW_PARTIAL;
                    row[3] += over;
                } else if constexpr (!RECORDS) {
                    atomicAdd(wave_moved_out + 0, (unsigned long long)over);
                }
            } else {
                c_invalid_turn += uint32_t(over);
            }
            cur = nv;
            inv = first_invalid_base(okay, nv, rd_end);
            neg_unknown_mini = false;
            where = 0;
            live = cur + k <= rd_end;
        }
        c_invalid += c_invalid_turn;
        const uint64_t valid_end = inv < rd_end ? inv : rd_end;
        /* -- seed() at cur (streaming_query.hpp:144-197): the k-mer, its key, its key's first bucket; a lane in the middle of a walk
              (its key's first bucket was not the end of it) keeps its k-mer and comes with the walk's next bucket instead -- */
        uint64_t ahead_f = 0, ahead_r = 0;
        bool table = false;
        STAT(st_fresh, live && !walking);
        STAT(st_walk, live && walking);
        STAT(st_idle, !live);
        if (live && !walking) {
            const uint64_t i = cur >> 5;
            const uint32_t sh = 2 * (uint32_t(cur) & 31u);
            const uint64_t w0 = packed[i], w1 = packed[i + 1];
            x.w[0] = funnel_shr(w0, w1, sh);
            if constexpr (W == 2) x.w[1] = funnel_shr(w1, packed[i + 2], sh);
            x = kmer_take_chars<W>(x, k);
            x_rc = kmer_revcomp<W>(x, k);
            if constexpr (SK) {
                /* what sk_key_persists looks at, asked for together with the k-mer's own words: one wait for all of the read this turn needs */
                const uint32_t sm = d.sk.m, hashed = sm < 12 ? sm : 12;
                ahead_f = read_bases32(packed, cur + k - sm + 1);
                ahead_r = read_bases32(packed, cur + k + 1 - hashed);
                const uint32_t heavy_left = (where >> WALK_HEAVY_SHIFT) & WALK_HEAVY;
                STAT(st_short, heavy_left != 0);
                if (heavy_left) {
                    /* the k-mer before this one met its key's marker, and this one elects the same occurrence -- one base further along its
                       strand --: straight to its own sequence */
                    kk.pos = kk.rc ? kk.pos + 1 : kk.pos - 1;
                    table = true;
                    on = sk_kmer_key<W>(x, x_rc);
                    const uint32_t back = (where >> WALK_HEAVY_BACK_SHIFT) & 7u;
                    where = WALK_VISITED | WALK_COMPACT | (back << WALK_BACK_SHIFT) | (back << WALK_HEAVY_BACK_SHIFT) | ((heavy_left - 1) << WALK_HEAVY_SHIFT);
                } else {
                    kk = sk_key<W>(x, x_rc, k, sm);
                    table = sk_usable(d, kk);
                    on = kk.key;
                    where = (WALK_NO_RETURN << WALK_BACK_SHIFT) | (WALK_LASTS << WALK_LASTS_SHIFT);  // choice 0 of the key's own sequence, nothing to come back to
                }
                on_a = sk_hash_a(on);
            }
        }
        if constexpr (SK) {
            if (live && walking && (!(where & WALK_VISITED) || (where & WALK_HEAVY_PENDING))) {  // (a walk along the key's own sequence may end in a miss that stands for more than itself; one behind a heavy key's marker ends with a look at how long the key lasts)
                const uint32_t sm = d.sk.m, hashed = sm < 12 ? sm : 12;
                ahead_f = read_bases32(packed, cur + k - sm + 1);
                ahead_r = read_bases32(packed, cur + k + 1 - hashed);
            }
        }
        bool settled = false, found = false;
        if constexpr (SK) {
            /* ONE bucket a turn for every lane that is at a seed: the key's first, or the next of a walk -- fetched by the wave together
               (sk_stage_lines: the four lanes of a quad read one line with one instruction, ONE address translation a line; a lane
               reading its own line in four pieces asks for four, and at 70 G translation misses a second chip-wide that bounded the
               first version of this kernel) and examined out of LDS. A walk that goes on does so in the lane's next turn: no lane
               waits inside a turn for another lane's second bucket (what the walk cost as a loop inside the turn: 27 % of the kernel,
               profiles/r05/streaming_ablation_what_each_part_costs.txt). */
            const bool need = table || walking;
            const uint32_t c = where & WALK_CHOICE;
            const bool compact = (where & WALK_COMPACT) != 0;  // on the k-mer's own sequence: the k-mers' region, compact entries
            uint32_t bucket = 0;
            if (need) bucket = compact ? d.sk.num_buckets + sk_choice_of(on, on_a, c, d.sk.kmer_buckets) : sk_choice_of(on, on_a, c, d.sk.num_buckets);
            sk_stage_lines<W, true>(d, bucket, 0u, need, wave_stage, compact);  // (all 64 lanes, whatever their event)
            if (need) {
                const uint4* mine = wave_stage + (lane & 3u) * 64 + (lane >> 2) * 4;
                sk_query_t<W> Q = sk_make_query<W>(x, x_rc, kk, uint32_t(on_a) & 0xFFFFFFu);
                fast_t r = fast_unsettled(false);
                sk_bucket_flags flags;
                flags.go_on = 0;
                flags.second_used = false;
                bool marker = false, seen = false, inline_seen = false;
                uint32_t lasts = 0xFFFFu;
                if (!compact) {
                    sk_examine_slot_tracking<W, true, true>(d, Q, c, [mine](uint32_t i) { return mine[i]; }, r, seen, marker, flags, lasts, inline_seen);
                    STAT(st_slot1, r.outcome == FAST_MISS && flags.second_used);
                    if (r.outcome == FAST_MISS && flags.second_used) {
                        if constexpr (W == 1) {
                            sk_examine_slot_tracking<W, false, true>(d, Q, c, [mine](uint32_t i) { return mine[2 + i]; }, r, seen, marker, flags, lasts, inline_seen);
                        } else {  // slot 1 lives in the bucket's second line, and only the lanes whose key's fingerprint is there get here
                            const uint4* B1 = reinterpret_cast<const uint4*>(d.sk.slots) + (SK_BUCKET_SLOTS * 2 * W) * uint64_t(bucket) + 2 * W;
                            sk_examine_slot_tracking<W, false, true>(d, Q, c, [B1](uint32_t i) { return B1[i]; }, r, seen, marker, flags, lasts, inline_seen);
                        }
                    }
                } else if constexpr (W == 1) {
                    const uint32_t* words = reinterpret_cast<const uint32_t*>(mine);
                    sk_examine_kmer_line(Q, c, [words](uint32_t i) { return words[i]; }, r, flags);
                } else {
                    sk_examine_kmer_entry<true>(Q, c, [mine](uint32_t i) { return mine[i]; }, r, flags);
                    sk_examine_kmer_entry<false>(Q, c, [mine](uint32_t i) { return mine[2 + i]; }, r, flags);
                }
                /* what the slots of the key's sequence have allowed so far, this bucket's included (the buckets of the KEY's sequence are
                   the key's alone: which of them a walk sees does not depend on the k-mer) */
                {
                    const uint32_t before = (where >> WALK_LASTS_SHIFT) & WALK_LASTS;
                    lasts = lasts < before ? lasts : before;
                    where = (where & ~(WALK_LASTS << WALK_LASTS_SHIFT)) | (lasts << WALK_LASTS_SHIFT) | (inline_seen ? WALK_INLINE : 0u);
                }
                /* where the walk goes from here (lookup_device.hpp: sk_walk_step) */
                const bool go_on = flags.go_on != 0;
                bool more = false, defer = false;
                if (r.outcome == FAST_MISS) {
                    if (marker && !(where & WALK_VISITED)) {  // the key is heavy: its k-mers are entered under keys of their own
                        const uint32_t back = go_on ? c + 1 : WALK_NO_RETURN;
                        where = WALK_VISITED | WALK_COMPACT | (back << WALK_BACK_SHIFT) |
                                ((where & WALK_INLINE) ? 0u : (WALK_HEAVY_PENDING | (back << WALK_HEAVY_BACK_SHIFT)));  // (nothing inline on the way: the k-mers behind may skip it)
                        on = sk_kmer_key<W>(x, x_rc);
                        on_a = sk_hash_a(on);
                        more = true;
                    } else if (go_on) {
                        defer = c + 1 >= SK_CHOICES;  // a key (or k-mer) that found no slot: the complete path
                        where = (where & ~WALK_CHOICE) | (c + 1);
                        more = !defer;
                    } else if (compact && ((where >> WALK_BACK_SHIFT) & WALK_CHOICE) != WALK_NO_RETURN) {
                        /* the k-mer is not under its own key (the marker may have been another key's with an equal fingerprint): what is
                           left is the rest of the key's sequence */
                        const uint32_t back = (where >> WALK_BACK_SHIFT) & WALK_CHOICE;
                        defer = back >= SK_CHOICES;
                        where = WALK_VISITED | back | (WALK_NO_RETURN << WALK_BACK_SHIFT) | (where & WALK_HEAVY_FIELDS);
                        on = kk.key;
                        on_a = sk_hash_a(on);
                        more = !defer;
                    }
                }
                walking = more;
                if (!more && !defer) {
                    settled = true;
                    found = r.outcome == FAST_HIT;
                    off = r.kmer_offset;
                    ori = r.orientation;
                    if constexpr (RECORDS || COVER || DEPTH || SUMS || CLASSES || BEST_RUN) hit_sid = r.string_id;
                    const bool stands = !found && !(where & WALK_VISITED);
                    if (stands || (where & WALK_HEAVY_PENDING)) {
                        /* a miss that stands for the k-mers behind this one: those that elect the same key occurrence (sk_key_persists)
                           and still hold the base that keeps the read and the key's slots apart (`lasts`, over every bucket of the key's
                           sequence the walk has seen; no slot with the key: all of them) are negative as well -- counted, not looked at.
                           (A walk that met its key's marker went on along the K-MER's own sequence: its miss stands for itself.) */
                        uint64_t keep = sk_key_persists<W>(kk, k, d.sk.m, ahead_f, ahead_r);
                        keep = keep < valid_end - (cur + k) ? keep : valid_end - (cur + k);
                        if (stands) {
                            keep = keep < lasts ? keep : lasts;
                            c_negative += keep;
                            cur += keep;
#ifdef SSHASH_STREAM_STATS
                            st_kept_lane += keep;
#endif
                        } else {  // (a heavy key's first k-mer, settled on its own sequence -- found or not: that many k-mers behind it share the key)
                            where = (where & ~(WALK_HEAVY_PENDING | (WALK_HEAVY << WALK_HEAVY_SHIFT))) | (uint32_t(keep) << WALK_HEAVY_SHIFT);
                        }
                    }
                }
            }
        }
        const bool finishing = live && !walking;  // (a walking lane's seed is settled in a later turn)
        STAT(st_full, finishing && !settled);
        if (finishing && !settled) {
            /* no table, or a tie / an unplaced key / another shard's key: the complete seed() */
            const minimizer_t mf = compute_minimizer<W>(x, k, d.m, d.hash_magic);
            const minimizer_t mr = compute_minimizer<W>(x_rc, k, d.m, d.hash_magic);
            if (!SK && neg_unknown_mini && mf.value == prev_f && mr.value == prev_r) {  // :150-157
                found = false;
            } else {
                prev_f = mf.value;
                prev_r = mr.value;
                const hit_t h = seed_lookup<W, CANON>(d, skew, x, x_rc, mf, mr);
                found = h.found;
                off = h.kmer_offset;
                ori = h.orientation;
                if constexpr (RECORDS || COVER || DEPTH || SUMS || CLASSES || BEST_RUN) hit_sid = h.string_id;
                neg_unknown_mini = !SK && !h.found && !h.minimizer_found;
            }
        }
        if (finishing) {
            if (found) {
                ++c_searches;
                neg_unknown_mini = false;
                pending = cur + 1 + k <= valid_end;  // (otherwise nothing can extend it)
                if constexpr (COUNT_RUNS) ++n_runs;
                if constexpr (SEG_RECORDS) {
                    if (!pending) {  // a run of one
                        if (seam_open) {
                            seg_runs_cont(sink, n_reads)[wave_first + my_row] = 1;
                            seam_open = false;
                        } else {
                            seg_record_store(d, sink, wave_first + my_row, cursor, cur, off, hit_sid, ori, 1);
                            ++cursor;
                        }
                    }
                } else if constexpr (RECORDS) {
                    if (!pending) {  // a run of one
                        run_record_store(d, sink, begins, wave_first + my_row, cursor, cur, off, hit_sid, ori, 1);
                        ++cursor;
                    }
                }
                if constexpr (COVER) {
                    if (!pending) cover_mark_run(d, sink, off, hit_sid, ori, 1);  // a run of one
                }
                if constexpr (DEPTH) {
                    if (!pending) depth_mark_run(d, sink, off, hit_sid, ori, 1);
                }
                if constexpr (SUMS) {
                    if (!pending) {  // a run of one: P[id + 1] - P[id]
                        const uint64_t kmer_id = off - uint64_t(hit_sid) * (k - 1);
                        sums_add(sink, row_first + my_row, sink.values_prefix[kmer_id + 1], sink.values_prefix[kmer_id], 1);
                    }
                }
                if constexpr (CLASSES) {
                    if (!pending) classes_add(sink, row_first + my_row, sink.labels[hit_sid], 1);  // a run of one
                }
                if constexpr (BEST_RUN) {
                    if (!pending) best_run_store(d, sink, begins, wave_first + my_row, best_len, cur, off, hit_sid, ori, 1);  // a run of one: the read's best only when it has none yet
                }
            } else {
                ++c_negative;
            }
            ++cur;
        }
        if constexpr (LATE_SUMS) {
            if (late_n) {
                sums_add(sink, row_first + late_row, late_forward ? late_far : late_anchor, late_forward ? late_anchor : late_far, late_n);
                late_n = 0;
            }
        }
    }
    if constexpr (LATE_SUMS) {  // (the turn that measured the last run of all left the loop before its end)
        if (late_n) sums_add(sink, row_first + late_row, late_forward ? late_far : late_anchor, late_forward ? late_anchor : late_far, late_n);
    }
#ifdef SSHASH_STREAM_STATS
    const unsigned long long st_neg_kept = wave_sum(st_kept_lane);
    if (lane == 0 && MODE == STREAM_TOTALS) {  // (the statistics are the six-counter kernel's: `report` is rows otherwise)
        unsigned long long* st = reinterpret_cast<unsigned long long*>(report) + 6;
        atomicAdd(st + 0, st_turns); atomicAdd(st + 1, st_fresh); atomicAdd(st + 2, st_walk); atomicAdd(st + 3, st_ext); atomicAdd(st + 4, st_slot1);
        atomicAdd(st + 5, st_inv); atomicAdd(st + 6, st_idle); atomicAdd(st + 7, st_full); atomicAdd(st + 8, st_neg_kept); atomicAdd(st + 9, st_short);
    }
#endif
    if constexpr (PER_READ) {
        if (my_row != ROW_NONE) row_flush(wave_rows + uint64_t(my_row & ~ROW_PARTIAL) * 6, (my_row & ROW_PARTIAL) != 0, c_invalid, c_negative, c_searches, c_extensions);  // (no lane gets here with a read: whoever is not live has handed its row in above)
    } else if constexpr (!RECORDS) {
        if constexpr (COUNT_RUNS) {
            if (my_row != ROW_NONE) sink.run_offsets[wave_first + my_row] = n_runs;  // (as the rows: nobody gets here with a read)
        }
        const bool first = lane == 0;  // (what the wave moved out is added once)
        block_report(first ? wave_moved_out[4] : 0, uint64_t(c_invalid) + (first ? wave_moved_out[0] : 0), uint64_t(c_negative) + (first ? wave_moved_out[1] : 0),
                     uint64_t(c_searches) + (first ? wave_moved_out[2] : 0), uint64_t(c_extensions) + (first ? wave_moved_out[3] : 0), report);
    }
}

/* the batch's six counters out of the rows of its reads: column sums, accumulated into `report` (one set of atomics a workgroup) */
__global__ void __launch_bounds__(256)
stream_rows_sum_kernel(const uint64_t* __restrict__ rows, const uint64_t n_reads, uint64_t* __restrict__ report) {
    uint64_t c_kmers = 0, c_invalid = 0, c_negative = 0, c_searches = 0, c_extensions = 0;
    const uint64_t stride = uint64_t(gridDim.x) * blockDim.x;
    for (uint64_t r = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x; r < n_reads; r += stride) {
        const uint64_t* row = rows + 6 * r;
        c_kmers += row[0];
        c_negative += row[2];
        c_invalid += row[3];
        c_searches += row[4];
        c_extensions += row[5];
    }
    block_report(c_kmers, c_invalid, c_negative, c_searches, c_extensions, report);
}

/* ---- an exclusive prefix sum over 64-bit words, in place (counts per read -> run_offsets; head marks -> ranks): tiles of 4096 words, three
        launches -- the tiles' sums, their scan by one workgroup, the tiles again with their sums in front. Two reads and a write a word. ---- */
constexpr uint32_t SCAN_PER_LANE = 16, SCAN_TILE = 256 * SCAN_PER_LANE;
inline uint64_t scan_tiles(uint64_t n) { return (n + SCAN_TILE - 1) / SCAN_TILE; }

/* (a workgroup of 256) what the lanes before this one hold together; `total`: what all hold */
template <class T>  // uint64_t; uint32_t for the depth's deltas (modulo 2^32)
__device__ __forceinline__ T block_exclusive_scan(T v, T& total) {
    __shared__ T wave_total[4];
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    T inc = v;
    for (uint32_t o = 1; o < 64; o <<= 1) {
        const T t = __shfl_up(inc, o, 64);
        if (lane >= o) inc += t;
    }
    __syncthreads();  // (called in a loop: the totals of the call before have been read)
    if (lane == 63) wave_total[w] = inc;
    __syncthreads();
    T before = 0;
    total = 0;
    for (uint32_t j = 0; j < 4; ++j) {
        if (j < w) before += wave_total[j];
        total += wave_total[j];
    }
    return before + inc - v;
}

__global__ void __launch_bounds__(256)
scan_tile_sums_kernel(const uint64_t* __restrict__ data, const uint64_t n, uint64_t* __restrict__ sums) {
    const uint64_t base = uint64_t(blockIdx.x) * SCAN_TILE + threadIdx.x * SCAN_PER_LANE;
    uint64_t v = 0;
    for (uint32_t j = 0; j < SCAN_PER_LANE; ++j)
        if (base + j < n) v += data[base + j];
    uint64_t total;
    block_exclusive_scan(v, total);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

__global__ void __launch_bounds__(256)
scan_sums_kernel(uint64_t* __restrict__ sums, const uint64_t tiles) {  // one workgroup
    uint64_t carry = 0;
    for (uint64_t at = 0; at < tiles; at += 256) {
        const uint64_t i = at + threadIdx.x;
        const uint64_t v = i < tiles ? sums[i] : 0;
        uint64_t total;
        const uint64_t before = block_exclusive_scan(v, total);
        if (i < tiles) sums[i] = carry + before;
        carry += total;
    }
}

__global__ void __launch_bounds__(256)
scan_apply_kernel(uint64_t* __restrict__ data, const uint64_t n, const uint64_t* __restrict__ sums) {
    const uint64_t base = uint64_t(blockIdx.x) * SCAN_TILE + threadIdx.x * SCAN_PER_LANE;
    uint64_t e[SCAN_PER_LANE], v = 0;
#pragma unroll
    for (uint32_t j = 0; j < SCAN_PER_LANE; ++j) {
        e[j] = base + j < n ? data[base + j] : 0;
        v += e[j];
    }
    uint64_t total;
    uint64_t at = sums[blockIdx.x] + block_exclusive_scan(v, total);
#pragma unroll
    for (uint32_t j = 0; j < SCAN_PER_LANE; ++j) {
        if (base + j < n) data[base + j] = at;
        at += e[j];
    }
}

/* data[i] = data[0] + .. + data[i - 1] for i < n; `sums`: scan_tiles(n) words of scratch */
void exclusive_scan_u64(uint64_t* data, uint64_t n, uint64_t* sums, hipStream_t s) {
    if (n == 0) return;
    const uint64_t tiles = scan_tiles(n);
    hipLaunchKernelGGL(scan_tile_sums_kernel, dim3(uint32_t(tiles)), dim3(256), 0, s, data, n, sums);
    hipLaunchKernelGGL(scan_sums_kernel, dim3(1), dim3(256), 0, s, sums, tiles);
    hipLaunchKernelGGL(scan_apply_kernel, dim3(uint32_t(tiles)), dim3(256), 0, s, data, n, sums);
    HIP_CHECK(hipGetLastError());
}

/* ---- the depth out of its deltas: out[i] = in[0] + .. + in[i] modulo 2^32, the same three launches over words of 32 bits -- tile sums,
        one workgroup over the sums (as many rounds of 256 as there are), apply; no workgroup waits for another. A lane holds 16
        consecutive words, 64 bytes: four 16-byte loads and stores where the arrays are 16-byte aligned and the lane's words all lie
        below n, word by word otherwise. out == in is allowed: a tile's words are all read (by the lanes that write them, in the apply
        launch; by the sums launch before it) before one of them is written. ---- */
__device__ __forceinline__ uint32_t scan_load16_u32(const uint32_t* __restrict__ in, uint64_t base, uint64_t n, bool aligned, uint32_t (&e)[SCAN_PER_LANE]) {
    static_assert(SCAN_PER_LANE == 16, "four 16-byte pieces a lane");
    uint32_t v = 0;
    if (aligned && base + SCAN_PER_LANE <= n) {
        const uint4* const q = reinterpret_cast<const uint4*>(in + base);
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) {
            const uint4 x = q[j];
            e[4 * j] = x.x, e[4 * j + 1] = x.y, e[4 * j + 2] = x.z, e[4 * j + 3] = x.w;
        }
    } else {
#pragma unroll
        for (uint32_t j = 0; j < SCAN_PER_LANE; ++j) e[j] = base + j < n ? in[base + j] : 0u;
    }
#pragma unroll
    for (uint32_t j = 0; j < SCAN_PER_LANE; ++j) v += e[j];
    return v;
}

__global__ void __launch_bounds__(256)
scan_tile_sums_u32_kernel(const uint32_t* in, const uint64_t n, uint32_t* __restrict__ sums) {
    const uint64_t base = uint64_t(blockIdx.x) * SCAN_TILE + threadIdx.x * SCAN_PER_LANE;
    uint32_t e[SCAN_PER_LANE], total;
    block_exclusive_scan(scan_load16_u32(in, base, n, (reinterpret_cast<uintptr_t>(in) & 15u) == 0, e), total);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

__global__ void __launch_bounds__(256)
scan_sums_u32_kernel(uint32_t* __restrict__ sums, const uint64_t tiles) {  // one workgroup; sums[t] becomes what the tiles before t hold
    uint32_t carry = 0;
    for (uint64_t at = 0; at < tiles; at += 256) {
        const uint64_t i = at + threadIdx.x;
        const uint32_t v = i < tiles ? sums[i] : 0u;
        uint32_t total;
        const uint32_t before = block_exclusive_scan(v, total);
        if (i < tiles) sums[i] = carry + before;
        carry += total;
    }
}

__global__ void __launch_bounds__(256)
scan_apply_inclusive_u32_kernel(const uint32_t* in, uint32_t* out, const uint64_t n, const uint32_t* __restrict__ sums) {  // (in and out may be one array)
    const uint64_t base = uint64_t(blockIdx.x) * SCAN_TILE + threadIdx.x * SCAN_PER_LANE;
    const bool aligned = ((reinterpret_cast<uintptr_t>(in) | reinterpret_cast<uintptr_t>(out)) & 15u) == 0;
    uint32_t e[SCAN_PER_LANE], total;
    const uint32_t v = scan_load16_u32(in, base, n, aligned, e);
    uint32_t at = sums[blockIdx.x] + block_exclusive_scan(v, total);
#pragma unroll
    for (uint32_t j = 0; j < SCAN_PER_LANE; ++j) e[j] = at += e[j];
    if (aligned && base + SCAN_PER_LANE <= n) {
        uint4* const q = reinterpret_cast<uint4*>(out + base);
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) q[j] = make_uint4(e[4 * j], e[4 * j + 1], e[4 * j + 2], e[4 * j + 3]);
    } else {
#pragma unroll
        for (uint32_t j = 0; j < SCAN_PER_LANE; ++j)
            if (base + j < n) out[base + j] = e[j];
    }
}

/* out[i] = in[0] + .. + in[i] modulo 2^32 for i < n; `sums`: scan_tiles(n) words of 32 bits of scratch */
void inclusive_scan_u32(uint32_t const* in, uint32_t* out, uint64_t n, uint32_t* sums, hipStream_t s) {
    if (n == 0) return;
    const uint64_t tiles = scan_tiles(n);
    if (tiles >> 31) throw error(error_kind::argument, "too many k-mers for one scan");
    hipLaunchKernelGGL(scan_tile_sums_u32_kernel, dim3(uint32_t(tiles)), dim3(256), 0, s, in, n, sums);
    hipLaunchKernelGGL(scan_sums_u32_kernel, dim3(1), dim3(256), 0, s, sums, tiles);
    hipLaunchKernelGGL(scan_apply_inclusive_u32_kernel, dim3(uint32_t(tiles)), dim3(256), 0, s, in, out, n, sums);
    HIP_CHECK(hipGetLastError());
}

/* ---- the values of the sums form as 64-bit words, ready for exclusive_scan_u64: wide[i] = values[i], or -- at_least >= 1 -- whether
        values[i] >= at_least; word n (the scan turns it into the total) zero ---- */
__global__ void __launch_bounds__(256)
values_widen_kernel(const uint32_t* __restrict__ values, const uint64_t n, const uint32_t at_least, uint64_t* __restrict__ wide) {
    const uint64_t i = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i > n) return;
    uint64_t v = 0;
    if (i < n) {
        const uint32_t x = values[i];
        v = at_least ? uint64_t(x >= at_least) : uint64_t(x);
    }
    wide[i] = v;
}

/* ==== long reads: SEGMENTS ==========================================================================================================
   One lane walks one read, so a batch of few long reads is few lanes, and its time is that of its longest read. A k-mer is positive,
   negative or invalid whatever lies around it; only whether a positive k-mer is a search or an extension depends on the k-mer before
   it. So a read of K k-mers is cut into ceil(K / S) SEGMENTS of S k-mers (segments.hpp: neighbours overlap by k - 1 bases of the packed
   copy, nothing is copied), the run kernel takes the segments for reads -- it is handed a begin and an end pointer, the offsets and the
   offsets behind them for whole reads, the two arrays of the segment table here --, and the one thing that differs is put right
   afterwards: a segment's first k-mer, when positive, was counted as a search; in the whole read it is an extension iff it continues
   the run of the k-mer before it (continues_run) -- the SEAM is then JOINED. The seam kernel looks both k-mers up, one lane a seam, and
   moves one count from searches to extensions for every joined seam. The cover is the same either way (OR), and so are the depth's
   deltas: adjacent runs [lo, mid) and [mid, hi) leave what [lo, hi) leaves, the +1 and the -1 at mid cancel. The sums likewise: P[mid]
   cancels, and the segments of a read add into the read's row (sink.read_of).
   The table is built on the stream: the segments of every read, their exclusive scan (the index of every read's first segment), and
   one lane per ENTRY that finds its read by bisection over those -- no lane's work grows with a read's length. The host sizes the table
   from a bound (segment_bound); the entries past the true count are empty segments, which the run kernel takes for reads shorter than k. */
__global__ void __launch_bounds__(256)
stream_segment_counts_kernel(const uint64_t* __restrict__ offsets, const uint64_t n_reads, const uint32_t k, const uint64_t S, uint64_t* __restrict__ counts) {
    const uint64_t r = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (r > n_reads) return;
    counts[r] = r < n_reads ? segments_of_read(read_kmers(offsets[r + 1] - offsets[r], k), S) : 0;  // (the last: scanned into the number of segments)
}

constexpr uint64_t SEG_NO_READ = ~uint64_t(0);  // seg_read of an entry past the last segment

__global__ void __launch_bounds__(256)
stream_segment_fill_kernel(const uint64_t* __restrict__ offsets, const uint64_t n_reads, const uint64_t* __restrict__ first /* n_reads + 1 */, const uint32_t k,
                           const uint64_t S, const uint64_t bound, uint64_t* __restrict__ seg_begin, uint64_t* __restrict__ seg_end, uint64_t* __restrict__ seg_read) {
    const uint64_t g = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (g >= bound) return;
    if (g >= first[n_reads]) {  // an empty segment
        seg_begin[g] = seg_end[g] = 0;
        seg_read[g] = SEG_NO_READ;
        return;
    }
    uint64_t lo = 0, hi = n_reads - 1;  // my read: the largest r with first[r] <= g (every read has a segment: `first` goes strictly up)
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo + 1) / 2;
        if (first[mid] <= g) lo = mid;
        else hi = mid - 1;
    }
    const uint64_t begin = offsets[lo], end = offsets[lo + 1], at = begin + (g - first[lo]) * S;
    seg_begin[g] = at;
    seg_end[g] = end - at > S + k - 1 ? at + S + k - 1 : end;
    seg_read[g] = lo;
}

/* the complete seed() of the k-mer that starts at base p of the packed reads, as the run kernel does it for a lane without a table */
template <int W, bool CANON>
__device__ __forceinline__ hit_t seed_at(dict_view const& d, skew_part_dev const* __restrict__ skew, const uint64_t* __restrict__ packed, uint64_t p) {
    const uint64_t i = p >> 5;
    const uint32_t sh = 2 * (uint32_t(p) & 31u);
    kmer_w<W> x = kmer_zero<W>();
    x.w[0] = funnel_shr(packed[i], packed[i + 1], sh);
    if constexpr (W == 2) x.w[1] = funnel_shr(packed[i + 1], packed[i + 2], sh);
    x = kmer_take_chars<W>(x, d.k);
    const kmer_w<W> x_rc = kmer_revcomp<W>(x, d.k);
    return seed_lookup<W, CANON>(d, skew, x, x_rc, compute_minimizer<W>(x, d.k, d.m, d.hash_magic), compute_minimizer<W>(x_rc, d.k, d.m, d.hash_magic));
}

/* One lane a seam: entry g > 0 of the table whose read is that of entry g - 1 begins at a seam, base p = seg_begin[g]; the k-mers
   that start at p - 1 and at p both lie in the read (segment g holds a k-mer, and p - 1 is a base of segment g - 1). joined[g]
   (`joined` may be null) = both are valid and positive and the second continues the run of the first. With `report`: its searches
   minus, its extensions plus the joined seams (modulo 2^64; the run kernel's own counts may arrive before or after), one pair of
   atomics a workgroup. */
template <int W, bool CANON>
__global__ void __launch_bounds__(256)
stream_seams_kernel(const dict_view d, const skew_part_dev* __restrict__ skew, const uint64_t* __restrict__ packed, const uint64_t* __restrict__ okay,
                    const uint64_t* __restrict__ seg_begin, const uint64_t* __restrict__ seg_read, const uint64_t* __restrict__ n_segments, const uint64_t bound,
                    uint8_t* __restrict__ joined, uint64_t* __restrict__ report) {
    __shared__ uint64_t wave_joined[4];
    const uint64_t g = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    bool join = false;
    if (g > 0 && g < bound && g < *n_segments && seg_read[g] == seg_read[g - 1]) {
        const uint64_t p = seg_begin[g];
        if (first_invalid_base(okay, p - 1, p + d.k) == p + d.k) {
            const hit_t before = seed_at<W, CANON>(d, skew, packed, p - 1);
            if (before.found) {
                const hit_t here = seed_at<W, CANON>(d, skew, packed, p);
                const uint64_t k1 = d.k - 1;  // (kmer_id = offset - string * (k - 1): run_record_store)
                join = here.found && continues_run(before.kmer_offset - uint64_t(before.string_id) * k1, before.string_id, before.orientation,
                                                   here.kmer_offset - uint64_t(here.string_id) * k1, here.string_id);
            }
        }
    }
    if (joined && g < bound) joined[g] = join ? 1 : 0;
    if (!report) return;  // (uniform)
    const uint64_t in_wave = wave_sum(join ? 1 : 0);
    if ((threadIdx.x & 63u) == 0) wave_joined[threadIdx.x >> 6] = in_wave;
    __syncthreads();
    if (threadIdx.x != 0) return;
    const unsigned long long J = wave_joined[0] + wave_joined[1] + wave_joined[2] + wave_joined[3];
    if (J == 0) return;
    atomicAdd(reinterpret_cast<unsigned long long*>(report + 4), 0ULL - J);
    atomicAdd(reinterpret_cast<unsigned long long*>(report + 5), J);
}

/* The rows of the segments into the rows of their reads (zeroed by the caller): one lane a segment, its joined seam moved from its
   searches to its extensions. The segments of a read are neighbours, thousands of them for a chromosome: the lanes of a wave first sum
   over their stretches of equal read (a segmented sum, five steps of doubling: after the step of width o a lane holds its own and the
   next 2 o - 1 of its stretch), and a stretch's first lane adds what is not zero -- at most one atomic per wave, read and counter. */
__global__ void __launch_bounds__(256)
stream_segment_rows_kernel(const uint64_t* __restrict__ seg_rows, const uint64_t* __restrict__ seg_read, const uint8_t* __restrict__ joined,
                           const uint64_t* __restrict__ n_segments, const uint64_t bound, uint64_t* __restrict__ rows) {
    const uint64_t g = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u;
    const bool has = g < bound && g < *n_segments;
    const uint64_t read = has ? seg_read[g] : SEG_NO_READ;
    uint64_t v[6] = {0, 0, 0, 0, 0, 0};
    if (has) {
#pragma unroll
        for (uint32_t c = 0; c < 6; ++c) v[c] = seg_rows[6 * g + c];
        const uint64_t j = joined[g];
        v[4] -= j;
        v[5] += j;
    }
    if (__ballot(has) == 0) return;  // (uniform)
    const uint64_t read_before = __shfl_up(read, 1, 64);
    for (uint32_t o = 1; o < 64; o <<= 1) {
        const bool same = __shfl_down(read, o, 64) == read && lane + o < 64;
#pragma unroll
        for (uint32_t c = 0; c < 6; ++c) {
            const uint64_t further = __shfl_down(v[c], o, 64);
            if (same) v[c] += further;
        }
    }
    if (!has || (lane > 0 && read_before == read)) return;
    unsigned long long* const row = reinterpret_cast<unsigned long long*>(rows + 6 * read);
#pragma unroll
    for (uint32_t c = 0; c < 6; ++c)
        if (v[c]) atomicAdd(row + c, (unsigned long long)v[c]);
}

/* ---- the run RECORDS over segments: a merge that moves no record ----
   A run that goes on over a seam arrives from the run kernel as the last run of one segment and the first of the next. joined[g] says
   exactly that of the seam in front of segment g, so the first run of such a segment is no record of its own, and of the c[g] runs the
   counting form finds in segment g, c'[g] = c[g] - joined[g] are records that START there. Their exclusive scan E puts every record at
   its final place -- reads in order, a read's segments in order, a segment's runs in order: the canonical layout --, and the CSR offsets
   of the reads are E at their first segments. The record form over segments stores every run that starts in its segment at E[g] and
   on, and hands the length of a joined first run to cont[g]; the merge adds that to the length of record E[g] - 1: the last record that
   starts before segment g, which is the run that the seam continues -- also through a chain of segments that lie wholly inside one run,
   because those start no record (c' = 0) and so share one E. The length's bit 31, the strand, is safe: the lengths of one run add up to
   fewer than 2^31 k-mers (the precondition on a read's length). The record's store and the adds are in different launches of one
   stream, and integer adds commute: the bytes are those of the uncut call. ---- */
__global__ void __launch_bounds__(256)
stream_segment_run_starts_kernel(uint64_t* __restrict__ counts /* bound + 1 */, const uint8_t* __restrict__ joined, const uint64_t* __restrict__ n_segments,
                                 const uint64_t bound) {
    const uint64_t g = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (g > bound) return;
    uint64_t starts = 0;
    if (g < bound && g < *n_segments) {
        const uint64_t c = counts[g], j = joined[g];
        starts = c > j ? c - j : 0;  // (a joined segment has a run: its first k-mer is positive)
    }
    counts[g] = starts;  // (the entries behind the last segment, and the word the scan turns into the total: zero)
}

/* the reads' CSR offsets out of E: read r's records begin where those of its first segment do; word n_reads -- first[n_reads] is the
   number of segments -- the number of records */
__global__ void __launch_bounds__(256)
stream_segment_run_offsets_kernel(const uint64_t* __restrict__ E, const uint64_t* __restrict__ first /* n_reads + 1 */, const uint64_t n_reads,
                                  uint64_t* __restrict__ run_offsets) {
    const uint64_t r = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (r <= n_reads) run_offsets[r] = E[first[r]];
}

/* one lane a segment: the length of a joined first run to the record it continues, unless the caller has no room for that record */
__global__ void __launch_bounds__(256)
stream_segment_run_merge_kernel(const uint64_t* __restrict__ E, const uint8_t* __restrict__ joined, const uint32_t* __restrict__ cont,
                                const uint64_t* __restrict__ n_segments, const uint64_t bound, void* records, const uint64_t capacity) {
    const uint64_t g = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (g >= bound || g >= *n_segments || !joined[g]) return;
    const uint64_t at = E[g];
    if (at == 0 || at - 1 >= capacity) return;  // (at > 0: the run that is continued started before this segment)
    uint32_t* const length = static_cast<uint32_t*>(records) + 8 * (at - 1) + RUN_RECORD_LENGTH_WORD;
    (void)__hip_atomic_fetch_add(length, cont[g], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

template <int W, bool CANON>
void launch_seams(device_replica const* rep, dict_view const& d, hipStream_t s, uint64_t const* packed, uint64_t const* okay, uint64_t const* seg_begin,
                  uint64_t const* seg_read, uint64_t const* n_segments, uint64_t bound, uint8_t* joined, uint64_t* report) {
    hipLaunchKernelGGL((stream_seams_kernel<W, CANON>), dim3(uint32_t((bound + 255) / 256)), dim3(256), 0, s, d, rep->d_skew, packed, okay, seg_begin, seg_read,
                       n_segments, bound, joined, report);
    HIP_CHECK(hipGetLastError());
}

/* The one place that launches the run kernel: (k > 31, canonical, skew table) -> <W, CANON, SK>, in the form MODE. */
template <int MODE>
using run_form = std::integral_constant<int, MODE>;  // (a form as a value: launch_streaming_runs names it where it launches)
template <int MODE>
void launch_run_kernel(device_replica const* rep, dict_view const& d, dim3 grid, dim3 block, hipStream_t s, uint64_t const* packed, uint64_t const* okay,
                       uint64_t const* begins, uint64_t const* ends, uint64_t n_reads, uint64_t reads_per_wave, uint32_t move_out_every, uint64_t* report,
                       run_sink const& sink) {
    auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, grid, block, 0, s, d, rep->d_skew, packed, okay, begins, ends, n_reads, reads_per_wave, move_out_every, report, sink);
        HIP_CHECK(hipGetLastError());
    };
    const bool wide = d.k > 31, canon = d.canonical, sk = d.sk.enabled;
    if (!wide && !canon && !sk) launch(streaming_run_kernel<1, false, false, MODE>);
    else if (!wide && !canon) launch(streaming_run_kernel<1, false, true, MODE>);
    else if (!wide && !sk) launch(streaming_run_kernel<1, true, false, MODE>);
    else if (!wide) launch(streaming_run_kernel<1, true, true, MODE>);
    else if (!canon && !sk) launch(streaming_run_kernel<2, false, false, MODE>);
    else if (!canon) launch(streaming_run_kernel<2, false, true, MODE>);
    else if (!sk) launch(streaming_run_kernel<2, true, false, MODE>);
    else launch(streaming_run_kernel<2, true, true, MODE>);
}

/* `run_phases` (with `sink`): RUNS_COUNT -- sink.run_offsets becomes the CSR offsets of the reads' runs (the counting form of the kernel, then
   the scan; `report` as without, may be null) --, RUNS_WRITE -- the records, for run_offsets that hold those offsets --, or both; or
   RUNS_COVER alone -- the cover form, ONE launch: the runs' k-mer ids marked in the bitmap at sink.records, `report` as without, may be null --;
   or RUNS_DEPTH alone -- the depth form, ONE launch: the runs' +1 / -1 added to the 32-bit deltas at sink.records, `report` as with the cover --;
   or RUNS_SUMS alone -- the sums form: the reads' rows at sink.records (n_reads x 2 words) zeroed, then ONE launch that adds every run's
   sum out of sink.values_prefix and its length to its read's row, `report` as with the cover --;
   or RUNS_CLASSES alone -- the classes form, a sink made by class_sink: the reads' rows at sink.records (n_reads x sink.num_classes words of
   32 bits) zeroed, then ONE launch that adds every run's length to the column of its string's label, `report` as with the cover --;
   or RUNS_BEST_RUN alone -- the best-run form: the reads' records at sink.records (n_reads x 32 bytes) zeroed, then ONE launch in which
   every lane stores its read's longest run, `report` as with the cover; never segmented. */
enum : int { RUNS_COUNT = 1, RUNS_WRITE = 2, RUNS_COVER = 4, RUNS_DEPTH = 8, RUNS_SUMS = 16, RUNS_CLASSES = 32, RUNS_BEST_RUN = 64 };
void launch_streaming_runs(device_replica const* rep, char const* bases, uint64_t const* offsets, uint64_t n_reads, uint64_t total_bases, uint64_t* report,
                           hipStream_t s, uint64_t* rows = nullptr /* per read: n_reads x 6 words; `report` may then be null */,
                           run_sink sink = run_sink{nullptr, nullptr, 0}, int run_phases = 0,
                           uint64_t S = 0 /* the reads cut into segments of S k-mers (totals, rows, run records, cover, depth, sums, classes; never the best run) */) {
    dict_view const& d = rep->view;
    const bool segmented = S != 0;
    if (segmented && (run_phases & RUNS_BEST_RUN)) throw error(error_kind::internal, "the best run is not segmented");
    const bool segmented_records = segmented && (run_phases & (RUNS_COUNT | RUNS_WRITE)) != 0;
    segment_layout L{};
    segment_runs_layout R{};
    if (segmented) {
        L = segment_scratch(n_reads, total_bases, S, SCAN_TILE, rows != nullptr);
        if (L.words == 0 || (L.bound + 255) / 256 >> 31) throw error(error_kind::argument, "too many segments for one call");
        if (segmented_records) {
            R = segment_runs_scratch(L.bound, SCAN_TILE);
            if (R.words == 0) throw error(error_kind::argument, "too many segments for one call");
        }
    }
    /* two bits and a validity bit a base, in words of 32 and 64 bases; three words of slack behind the last base (a seed and a
       run read up to two words past their first) */
    const uint64_t packed_bytes = ((total_bases + 31) / 32 + 3) * 8, okay_bytes = ((total_bases + 63) / 64 + 2) * 8;
    /* (scratch the replica keeps for this stream, replica.hpp; two host threads that share a stream must not interleave their
       launch sequences, which share it) */
    const uint64_t runs_bytes = run_phases ? (scan_tiles(n_reads + 1) + 6) * 8 : 0;  // (the scan's tile sums; six counters nobody asked for)
    uint64_t* const caller_report = report;
    std::lock_guard<std::mutex> sequence(rep->launch_mutex);
    uint64_t* packed = static_cast<uint64_t*>(rep->read_scratch_for(s, packed_bytes + okay_bytes + runs_bytes + (L.words + R.words) * 8));
    uint64_t* okay = packed + packed_bytes / 8;
    uint64_t* scan_sums = okay + okay_bytes / 8;
    uint64_t* const seg = scan_sums + runs_bytes / 8;  // (segmented) the table, the segments' rows, the seam flags: segments.hpp
    uint64_t* const seg_runs = seg + L.words;           // (the run records over segments) segments.hpp: segment_runs_scratch
    if (total_bases) {
        const uint64_t lanes = (total_bases + 7) / 8;
        hipLaunchKernelGGL(stream_pack_kernel, dim3(uint32_t((lanes + 255) / 256)), dim3(256), 0, s, bases, total_bases,
                           reinterpret_cast<uint16_t*>(packed), reinterpret_cast<uint8_t*>(okay));
    }
    /* what the lanes take for reads: the reads, or their segments -- every entry of the table, the empty ones behind the last included */
    uint64_t const *begins = offsets, *ends = offsets + 1;
    const uint64_t n_whole_reads = n_reads;
    if (segmented) {
        hipLaunchKernelGGL(stream_segment_counts_kernel, dim3(uint32_t((n_reads + 256) / 256)), dim3(256), 0, s, offsets, n_reads, d.k, S, seg + L.first);
        exclusive_scan_u64(seg + L.first, n_reads + 1, seg + L.sums, s);
        hipLaunchKernelGGL(stream_segment_fill_kernel, dim3(uint32_t((L.bound + 255) / 256)), dim3(256), 0, s, offsets, n_reads, seg + L.first, d.k, S, L.bound,
                           seg + L.begin, seg + L.end, seg + L.read);
        HIP_CHECK(hipGetLastError());
        begins = seg + L.begin;
        ends = seg + L.end;
        n_reads = L.bound;
    }
    /* (segmented, and somebody wants searches and extensions apart: the joined seams; `joined`: the flags, for the rows) */
    auto seams = [&](uint8_t* joined, uint64_t* into) {
        uint64_t const* n_segments = seg + L.first + n_whole_reads;
        if (d.k <= 31 && !d.canonical) launch_seams<1, false>(rep, d, s, packed, okay, begins, seg + L.read, n_segments, L.bound, joined, into);
        else if (d.k <= 31) launch_seams<1, true>(rep, d, s, packed, okay, begins, seg + L.read, n_segments, L.bound, joined, into);
        else if (!d.canonical) launch_seams<2, false>(rep, d, s, packed, okay, begins, seg + L.read, n_segments, L.bound, joined, into);
        else launch_seams<2, true>(rep, d, s, packed, okay, begins, seg + L.read, n_segments, L.bound, joined, into);
    };
    /* waves: as many as the chip holds at once -- a lane that finishes its read takes the next of its wave's share, and the longer the
       share, the better the lanes of a wave even out --, fewer for a small call (a piece of a query file: some 10^4 reads, many calls
       side by side on their own streams), down to two reads a lane */
    const uint64_t max_waves = uint64_t(256) * 4 * SSHASH_STREAM_WAVES;  // (what the chip holds of this kernel: 256 CUs, four SIMDs each, SSHASH_STREAM_WAVES waves a SIMD)
    uint64_t waves = std::min<uint64_t>(max_waves, std::max<uint64_t>(1, n_reads / (64 * 2)));
    waves = (waves + 3) / 4 * 4;
    const uint64_t reads_per_wave = (n_reads + waves - 1) / waves;
    const dim3 grid(uint32_t(waves / 4)), block(256);
    const uint32_t move_out_every = uint32_t(test_hook_u64("stream_move_out_every", uint64_t(1) << 16, 1, uint64_t(1) << 16));
    /* the cover, the depth and the counting form count the batch as they go: where nobody asked for the six counters they go into the scratch */
    auto totals = [&]() {
        if (report) return report;
        uint64_t* spare = scan_sums + scan_tiles(n_whole_reads + 1);
        HIP_CHECK(hipMemsetAsync(spare, 0, 6 * sizeof(uint64_t), s));
        return spare;
    };
    /* the row, counting, record and sums forms keep a lane's read as a 31-bit index into its wave's share -- not the cover and totals forms */
    if ((rows || (run_phases & (RUNS_COUNT | RUNS_WRITE | RUNS_SUMS | RUNS_CLASSES | RUNS_BEST_RUN))) && reads_per_wave >> 31) throw error(error_kind::argument, "too many reads for one call");
    /* the launch line of every form: what differs is the form, where the six counters (or the rows) go, and the sink */
    auto run = [&](auto form, uint64_t* into) {
        launch_run_kernel<decltype(form)::value>(rep, d, grid, block, s, packed, okay, begins, ends, n_reads, reads_per_wave, move_out_every, into, sink);
    };
    const int one_launch = run_phases & (RUNS_COVER | RUNS_DEPTH | RUNS_SUMS | RUNS_CLASSES | RUNS_BEST_RUN);
    if (one_launch) {
        /* the forms with a row per read add to it, or leave it alone (the best run of a read without a hit, or without a k-mer: num_kmers == 0 is
           "no run"): zeroed first. Over segments their lanes look their read up. (A run that spans a seam arrives as [lo, mid) and [mid, hi):
           the sums' P[mid] cancels, the lengths add up, in the same column of the classes -- the seams are for the counters alone.) */
        const uint64_t row_bytes = one_launch == RUNS_SUMS ? 2 * sizeof(uint64_t) : one_launch == RUNS_CLASSES ? sink.num_classes * sizeof(uint32_t) : one_launch == RUNS_BEST_RUN ? 32 : 0;
        if (row_bytes) HIP_CHECK(hipMemsetAsync(sink.records, 0, n_whole_reads * row_bytes, s));
        if (segmented && (one_launch & (RUNS_SUMS | RUNS_CLASSES))) sink.read_of = seg + L.read;
        if (one_launch == RUNS_COVER) run(run_form<STREAM_COVER>{}, totals());
        else if (one_launch == RUNS_DEPTH) run(run_form<STREAM_DEPTH>{}, totals());
        else if (one_launch == RUNS_SUMS) run(run_form<STREAM_SUMS>{}, totals());
        else if (one_launch == RUNS_CLASSES) run(run_form<STREAM_CLASSES>{}, totals());
        else run(run_form<STREAM_BEST_RUN>{}, totals());
        if (segmented && caller_report) seams(nullptr, caller_report);  // (nobody reads the six counters: no seam is looked at; the best run is never segmented)
    } else if (segmented_records) {
        /* ("the run RECORDS over segments" above) Either phase needs the segments' counts, the seams and E: a call that only writes makes
           them again -- the scratch is this call's alone only while it holds the launch mutex, so nothing is kept from the counting call. */
        uint64_t* const E = seg_runs + R.counts;
        uint8_t* const joined = reinterpret_cast<uint8_t*>(seg_runs + R.joined);
        uint64_t const* const n_segments = seg + L.first + n_whole_reads;
        const uint32_t entry_blocks = uint32_t((L.bound + 256) / 256);  // (bound + 1 lanes)
        const run_sink counting{E, nullptr, 0};
        launch_run_kernel<STREAM_RUN_COUNTS>(rep, d, grid, block, s, packed, okay, begins, ends, n_reads, reads_per_wave, move_out_every, totals(), counting);
        seams(joined, (run_phases & RUNS_COUNT) ? caller_report : nullptr);
        hipLaunchKernelGGL(stream_segment_run_starts_kernel, dim3(entry_blocks), dim3(256), 0, s, E, joined, n_segments, L.bound);
        HIP_CHECK(hipGetLastError());
        exclusive_scan_u64(E, L.bound + 1, seg_runs + R.sums, s);
        if (run_phases & RUNS_COUNT) {
            hipLaunchKernelGGL(stream_segment_run_offsets_kernel, dim3(uint32_t((n_whole_reads + 256) / 256)), dim3(256), 0, s, E, seg + L.first, n_whole_reads,
                               sink.run_offsets);
            HIP_CHECK(hipGetLastError());
        }
        if (run_phases & RUNS_WRITE) {
            const run_sink writing{E, sink.records, sink.capacity, offsets /* the reads' begins, in the word of values_prefix */, seg + L.read};
            launch_run_kernel<STREAM_RUN_RECORDS_SEGMENTS>(rep, d, grid, block, s, packed, okay, begins, ends, n_reads, reads_per_wave, move_out_every, nullptr, writing);
            hipLaunchKernelGGL(stream_segment_run_merge_kernel, dim3(uint32_t((L.bound + 255) / 256)), dim3(256), 0, s, E, joined,
                               reinterpret_cast<uint32_t const*>(seg_runs + R.cont), n_segments, L.bound, sink.records, sink.capacity);
            HIP_CHECK(hipGetLastError());
        }
    } else if (run_phases) {
        if (run_phases & RUNS_COUNT) {
            run(run_form<STREAM_RUN_COUNTS>{}, totals());
            HIP_CHECK(hipMemsetAsync(sink.run_offsets + n_reads, 0, sizeof(uint64_t), s));
            exclusive_scan_u64(sink.run_offsets, n_reads + 1, scan_sums, s);
        }
        if (run_phases & RUNS_WRITE) run(run_form<STREAM_RUN_RECORDS>{}, nullptr);
    } else if (rows) {
        if (segmented) {  // a row per segment in the scratch, then the reads' rows out of those and the seams
            uint8_t* const joined = reinterpret_cast<uint8_t*>(seg + L.joined);
            run(run_form<STREAM_ROWS>{}, seg + L.rows);
            seams(joined, nullptr);
            HIP_CHECK(hipMemsetAsync(rows, 0, n_whole_reads * 6 * sizeof(uint64_t), s));
            hipLaunchKernelGGL(stream_segment_rows_kernel, dim3(uint32_t((L.bound + 255) / 256)), dim3(256), 0, s, seg + L.rows, seg + L.read, joined,
                               seg + L.first + n_whole_reads, L.bound, rows);
            HIP_CHECK(hipGetLastError());
        } else {
            run(run_form<STREAM_ROWS>{}, rows);
        }
        if (report) {
            const uint32_t blocks = uint32_t(std::min<uint64_t>((n_whole_reads + 255) / 256, 1024));
            hipLaunchKernelGGL(stream_rows_sum_kernel, dim3(blocks), dim3(256), 0, s, rows, n_whole_reads, report);
            HIP_CHECK(hipGetLastError());
        }
    } else {
        run(run_form<STREAM_TOTALS>{}, report);
        if (segmented && report) seams(nullptr, report);
    }
}

/* The packing pass covers bases [0, read_offsets[n_reads]): a caller that does not say how many that is (total_bases = 0: the C ABI's
   device entry points) costs the launch one 8-byte read-back on its stream. */
uint64_t resolve_total_bases(uint64_t const* d_read_offsets, uint64_t n_reads, uint64_t total_bases, hipStream_t s) {
    if (n_reads && total_bases == 0) {
        HIP_CHECK(hipMemcpyAsync(&total_bases, d_read_offsets + n_reads, sizeof(uint64_t), hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
    }
    return total_bases;
}

/* The writing pass of streaming_runs_host for one piece, behind its counting call (streaming_runs_device without room for a record, from
   which the piece's records were sized): the records, for sink.run_offsets that hold the offsets of these very reads. `S`: what the
   counting call cut the reads into (0: whole reads). The counting call is what counts as a segmented launch. */
void streaming_runs_write(engine const& eng, int device, char const* d_bases, uint64_t const* d_read_offsets, uint64_t n_reads, uint64_t total_bases,
                          run_sink const& sink, hipStream_t s, uint64_t S) {
    if (n_reads == 0 || total_bases == 0) return;  // no read, or empty reads only: no run
    device_guard guard(device);
    launch_streaming_runs(eng.replica(device), d_bases, d_read_offsets, n_reads, total_bases, nullptr, s, nullptr, sink, RUNS_WRITE, S);
}

}  // namespace

/* What the device entry points of the run kernel share behind their own argument checks: the device made current, the number of bases
   resolved, and -- empty reads only -- `d_rows` (nullable: the call keeps nothing per read) zeroed, `row_bytes` a read, and nothing
   launched; else `launch` (void(hipStream_t, uint64_t total_bases, uint64_t S)) with the segments the call takes. */
template <class Launch>
void engine::run_kernel_call(int device, uint64_t const* d_read_offsets, uint64_t n_reads, uint64_t total_bases, void* stream, uint64_t segment_kmers,
                             void* d_rows, uint64_t row_bytes, Launch const& launch) const {
    device_guard guard(device);
    hipStream_t s = hipStream_t(stream);
    total_bases = resolve_total_bases(d_read_offsets, n_reads, total_bases, s);
    if (total_bases == 0) {  // empty reads only: no k-mer, their rows are zero
        if (d_rows) HIP_CHECK(hipMemsetAsync(d_rows, 0, n_reads * row_bytes, s));
        return;
    }
    const uint64_t S = segments_for(segment_kmers);
    launch(s, total_bases, S);
    if (S) ++m_segmented_launches;  // (counted once the launches are made: a call that threw is none)
}

void engine::streaming_query_device(int device, char const* d_bases, uint64_t const* d_read_offsets, uint64_t n_reads,
                                    uint64_t total_bases, uint64_t* d_report, void* stream, uint64_t segment_kmers) const {
    device_replica const* rep = replica(device);
    if (n_reads == 0) return;
    run_kernel_call(device, d_read_offsets, n_reads, total_bases, stream, segment_kmers, nullptr, 0, [&](hipStream_t s, uint64_t nb, uint64_t S) {
        launch_streaming_runs(rep, d_bases, d_read_offsets, n_reads, nb, d_report, s, nullptr, run_sink{nullptr, nullptr, 0}, 0, S);
    });
}

/* The setting of sshash_set_read_segments (engine.hpp). */
void engine::set_read_segments(uint64_t kmers_per_segment, bool device_calls) {
    if (!segment_setting_valid(kmers_per_segment)) throw error(error_kind::argument, "kmers_per_segment is neither 0, SSHASH_SEGMENTS_OFF nor in 1 .. 2^30");
    m_segment_kmers = kmers_per_segment ? kmers_per_segment : SEGMENT_KMERS_DEFAULT;
    m_segment_device_calls = device_calls;
}

/* What a host call cuts its long reads into: the setting, except on a minimizer shard -- its run kernel follows a run through k-mers
   it does not own, which a seed at a seam would miss: a shard never segments. 0: no segments. */
uint64_t engine::host_segments() const {
    const uint64_t S = m_segment_kmers;
    return S == SEGMENTS_OFF || m_idx->num_shards > 1 ? 0 : S;
}

/* What a device entry point launches with: what its caller inside the library says (0, or the S of a piece that holds a long read;
   SEGMENTS_OFF is 0 as well), or -- SEGMENTS_AS_SET, the C ABI -- the setting where it was made for the device calls as well. */
uint64_t engine::segments_for(uint64_t asked) const {
    if (asked == SEGMENTS_AS_SET) return m_segment_device_calls ? host_segments() : 0;
    return asked == SEGMENTS_OFF ? 0 : asked;
}

/* One report per read, by the run kernel whatever the reads' lengths (one lane a read, or -- segment_kmers -- one lane a segment).
   Every row is written: also when no base is there to look at. */
void engine::streaming_query_per_read_device(int device, char const* d_bases, uint64_t const* d_read_offsets, uint64_t n_reads,
                                             uint64_t total_bases, uint64_t* d_rows, uint64_t* d_report, void* stream, uint64_t segment_kmers) const {
    device_replica const* rep = replica(device);
    if (n_reads == 0) return;
    if (!d_rows) throw error(error_kind::argument, "per-read output pointer is null");
    run_kernel_call(device, d_read_offsets, n_reads, total_bases, stream, segment_kmers, d_rows, 6 * sizeof(uint64_t), [&](hipStream_t s, uint64_t nb, uint64_t S) {
        launch_streaming_runs(rep, d_bases, d_read_offsets, n_reads, nb, d_report, s, d_rows, run_sink{nullptr, nullptr, 0}, 0, S);
    });
}

/* The runs of every read (sshash_streaming_runs_device): count -> scan -> write, always the run kernel -- one lane a read, or
   (segment_kmers) one lane a segment and the merge of the runs that span seams behind it: the same offsets, the same bytes. */
void engine::streaming_runs_device(int device, char const* d_bases, uint64_t const* d_read_offsets, uint64_t n_reads, uint64_t total_bases,
                                   uint64_t* d_run_offsets, void* d_runs, uint64_t runs_capacity, uint64_t* d_report, void* stream,
                                   uint64_t segment_kmers) const {
    device_replica const* rep = replica(device);  // (not resident: that error first)
    if (n_reads == 0 && !d_run_offsets) return;
    if (!d_run_offsets) throw error(error_kind::argument, "run_offsets pointer is null");
    if (!d_runs && runs_capacity) throw error(error_kind::argument, "runs pointer is null");
    bool launched = false;
    if (n_reads)
        run_kernel_call(device, d_read_offsets, n_reads, total_bases, stream, segment_kmers, nullptr, 0, [&](hipStream_t s, uint64_t nb, uint64_t S) {
            launched = true;
            launch_streaming_runs(rep, d_bases, d_read_offsets, n_reads, nb, d_report, s, nullptr, run_sink{d_run_offsets, d_runs, runs_capacity},
                                  RUNS_COUNT | (runs_capacity ? RUNS_WRITE : 0), S);
        });
    if (!launched) {  // no read, or empty reads only: no run
        device_guard guard(device);
        HIP_CHECK(hipMemsetAsync(d_run_offsets, 0, (n_reads + 1) * sizeof(uint64_t), hipStream_t(stream)));
    }
}

/* Which k-mers of the dictionary the reads hold (sshash_streaming_cover_device): the cover form of the run kernel, one launch. */
void engine::streaming_cover_device(int device, char const* d_bases, uint64_t const* d_read_offsets, uint64_t n_reads, uint64_t total_bases,
                                    uint64_t* d_cover, uint64_t* d_report, void* stream, uint64_t segment_kmers) const {
    device_replica const* rep = replica(device);  // (not resident: that error first)
    if (n_reads == 0) return;
    if (!d_cover) throw error(error_kind::argument, "cover pointer is null");
    run_kernel_call(device, d_read_offsets, n_reads, total_bases, stream, segment_kmers, nullptr, 0, [&](hipStream_t s, uint64_t nb, uint64_t S) {
        launch_streaming_runs(rep, d_bases, d_read_offsets, n_reads, nb, d_report, s, nullptr, run_sink{nullptr, d_cover, 0}, RUNS_COVER, S);
    });
}

/* How often the reads hold each k-mer of the dictionary (sshash_streaming_depth_device): the depth form of the run kernel, one launch,
   into the deltas; depth_finish_device turns deltas into depths. */
void engine::streaming_depth_device(int device, char const* d_bases, uint64_t const* d_read_offsets, uint64_t n_reads, uint64_t total_bases,
                                    uint32_t* d_deltas, uint64_t* d_report, void* stream, uint64_t segment_kmers) const {
    device_replica const* rep = replica(device);  // (not resident: that error first)
    if (n_reads == 0) return;
    if (!d_deltas) throw error(error_kind::argument, "deltas pointer is null");
    /* (a run is measured along the STRING, which a shard holds whole: behind a k-mer of its own it runs on through k-mers of other
       shards, and the shards' arrays added would hold those twice. The cover does not mind -- OR --, a count does.) */
    if (m_idx->num_shards > 1) throw error(error_kind::argument, "a minimizer shard counts per k-mer: use the host call (sshash_streaming_depth)");
    run_kernel_call(device, d_read_offsets, n_reads, total_bases, stream, segment_kmers, nullptr, 0, [&](hipStream_t s, uint64_t nb, uint64_t S) {
        launch_streaming_runs(rep, d_bases, d_read_offsets, n_reads, nb, d_report, s, nullptr, run_sink{nullptr, d_deltas, 0}, RUNS_DEPTH, S);
    });
}

/* exclusive_scan_u64 for the callers outside this file (replica.hpp: the offsets of the string links, engine.hip) */
void exclusive_scan_words(device_replica const* rep, uint64_t* data, uint64_t n, hipStream_t s) {
    device_buffers tmp(rep, s);
    exclusive_scan_u64(data, n, tmp.alloc<uint64_t>(scan_tiles(n)), s);
}

/* The prefix sums of a value per k-mer (sshash_value_prefix_device): widened, word num_kmers zero, scanned in place. */
void engine::value_prefix_device(int device, uint32_t const* d_values, uint32_t at_least, uint64_t* d_prefix, void* stream) const {
    device_replica const* rep = replica(device);
    if (!d_values || !d_prefix) throw error(error_kind::argument, "null pointer");
    device_guard guard(device);
    hipStream_t s = hipStream_t(stream);
    const uint64_t n = rep->view.num_kmers, blocks = (n + 256) / 256;  // (n + 1 words)
    if (blocks >> 31) throw error(error_kind::argument, "too many k-mers for one launch");
    hipLaunchKernelGGL(values_widen_kernel, dim3(uint32_t(blocks)), dim3(256), 0, s, d_values, n, at_least, d_prefix);
    HIP_CHECK(hipGetLastError());
    device_buffers tmp(rep, s);  // (stream-ordered, out of the replica's pool: handed back behind the apply launch)
    exclusive_scan_u64(d_prefix, n + 1, tmp.alloc<uint64_t>(scan_tiles(n + 1)), s);
}

/* Per read, the sum of a value per k-mer over its positive k-mers and their number (sshash_streaming_sums_device): the sums form of the
   run kernel, a memset and one launch. Every row is written: also when no base is there to look at. */
void engine::streaming_sums_device(int device, char const* d_bases, uint64_t const* d_read_offsets, uint64_t n_reads, uint64_t total_bases,
                                   uint64_t const* d_prefix, uint64_t* d_sums, uint64_t* d_report, void* stream, uint64_t segment_kmers) const {
    device_replica const* rep = replica(device);  // (not resident: that error first)
    if (n_reads == 0) return;
    if (!d_prefix || !d_sums) throw error(error_kind::argument, "prefix or sums pointer is null");
    /* (as the depth: a shard's run kernel follows a run through k-mers of other shards, and the shards' rows added would hold those twice) */
    if (m_idx->num_shards > 1) throw error(error_kind::argument, "a minimizer shard counts per k-mer: use the host call (sshash_streaming_sums)");
    run_kernel_call(device, d_read_offsets, n_reads, total_bases, stream, segment_kmers, d_sums, 2 * sizeof(uint64_t), [&](hipStream_t s, uint64_t nb, uint64_t S) {
        launch_streaming_runs(rep, d_bases, d_read_offsets, n_reads, nb, d_report, s, nullptr, run_sink{nullptr, d_sums, 0, d_prefix, nullptr}, RUNS_SUMS, S);
    });
}

/* Per read, its positive k-mers by class of string (sshash_streaming_classes_device): the classes form of the run kernel, a memset and
   one launch. Every row is written: also when no base is there to look at. */
void engine::streaming_classes_device(int device, char const* d_bases, uint64_t const* d_read_offsets, uint64_t n_reads, uint64_t total_bases,
                                      uint32_t const* d_labels, uint32_t num_classes, uint32_t* d_rows, uint64_t* d_report, void* stream,
                                      uint64_t segment_kmers) const {
    device_replica const* rep = replica(device);  // (not resident: that error first)
    if (n_reads == 0) return;
    if (!d_labels || !d_rows) throw error(error_kind::argument, "labels or rows pointer is null");
    if (num_classes == 0 || num_classes > MAX_CLASSES) throw error(error_kind::argument, "num_classes must be 1 .. 4096");
    /* (as the depth and the sums: a shard's run kernel follows a run through k-mers of other shards, and the shards' rows added would hold those twice) */
    if (m_idx->num_shards > 1) throw error(error_kind::argument, "a minimizer shard counts per k-mer: use the host call (sshash_streaming_classes)");
    run_kernel_call(device, d_read_offsets, n_reads, total_bases, stream, segment_kmers, d_rows, num_classes * sizeof(uint32_t), [&](hipStream_t s, uint64_t nb, uint64_t S) {
        launch_streaming_runs(rep, d_bases, d_read_offsets, n_reads, nb, d_report, s, nullptr, class_sink(d_labels, num_classes, d_rows), RUNS_CLASSES, S);
    });
}

/* a shard's run kernel follows a run through k-mers it does not own, and the longest runs of the shards do not combine into the whole
   index's: no route of the best run serves a minimizer shard */
static void best_run_refuse_shard(host_index const& idx) {
    if (idx.num_shards > 1)
        throw error(error_kind::argument, "a minimizer shard has no longest run: its run kernel follows a run through k-mers of other shards, and the shards' "
                                          "longest runs do not combine into the whole index's -- use sshash_streaming_runs on the whole index");
}

/* Per read, its longest run (sshash_streaming_best_run_device): the best-run form of the run kernel, a memset and one launch, never over
   segments. Every record is written: also when no base is there to look at. */
void engine::streaming_best_run_device(int device, char const* d_bases, uint64_t const* d_read_offsets, uint64_t n_reads, uint64_t total_bases,
                                       void* d_best, uint64_t* d_report, void* stream) const {
    device_replica const* rep = replica(device);  // (not resident: that error first)
    if (n_reads == 0) return;
    if (!d_best) throw error(error_kind::argument, "best pointer is null");
    best_run_refuse_shard(*m_idx);
    run_kernel_call(device, d_read_offsets, n_reads, total_bases, stream, 0 /* never over segments */, d_best, 32, [&](hipStream_t s, uint64_t nb, uint64_t) {
        launch_streaming_runs(rep, d_bases, d_read_offsets, n_reads, nb, d_report, s, nullptr, run_sink{nullptr, d_best, 0}, RUNS_BEST_RUN);
    });
}

void engine::depth_finish_device(int device, uint32_t const* d_deltas, uint32_t* d_depth, void* stream) const {
    device_replica const* rep = replica(device);
    if (!d_deltas || !d_depth) throw error(error_kind::argument, "null pointer");
    device_guard guard(device);
    hipStream_t s = hipStream_t(stream);
    const uint64_t n = rep->view.num_kmers;
    device_buffers tmp(rep, s);  // (stream-ordered, out of the replica's pool: handed back behind the apply launch)
    inclusive_scan_u32(d_deltas, d_depth, n, tmp.alloc<uint32_t>(scan_tiles(n)), s);
}

/* ---- per-k-mer results: the streaming query as a position-parallel pipeline -----------------------------------
   The reference asserts, for every k-mer, that its streaming result equals the point lookup
   (include/streaming_query.hpp:107); what the state machine adds is bookkeeping: a k-mer is invalid iff one of its k
   characters is (:59-65: an invalid one resets to full validation), a positive k-mer is an *extension* iff the
   previous k-mer of the read was positive, in the same string, and the id moved by that k-mer's orientation (:86-100;
   `remaining_string_bases > 0` is "same string"), otherwise a *search*; everything else is negative. So:
     1. encode    one lane per base of the reads: which read it lies in (a tile of 256 positions resolves its reads
                  through LDS), whether a k-mer starts there, its validity, the packed k-mer (characters staged in
                  LDS, four packed at a time);
     2. lookup    the batched lookup over all places holding a valid k-mer (engine.hip: first / resume / deferred
                  passes) -- every k-mer at full lookup speed, no serial chain along a read, long reads cost nothing
                  special;
     3. classify  one lane per k-mer: counters, and the default result for invalid k-mers. */
constexpr uint8_t SQ_VALID = 1, SQ_INVALID = 2, SQ_FIRST = 4;  // flags of a place; 0 = no k-mer starts here

__device__ __forceinline__ uint32_t nonzero_bytes(uint32_t v) {  // 0x80 in every byte of v that is not zero
    return (((v & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | v) & 0x80808080u;
}

/* The read holding the first base of every tile of 256 places: one lane per TILE. (Looked up by lane 0 of the tile's own
   workgroup, these ~20 dependent loads were the lifetime of the workgroup: the encode pass was slower than the lookups.) */
__global__ void __launch_bounds__(256)
stream_tile_reads_kernel(const uint64_t* __restrict__ offsets, const uint64_t n_reads, const uint64_t first, const uint64_t tiles,
                         uint64_t* __restrict__ tile_read) {
    const uint64_t t = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (t >= tiles) return;
    const uint64_t g0 = first + t * 256;
    uint64_t lo = 0, hi = n_reads - 1;  // largest r with offsets[r] <= g0
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo + 1) / 2;
        if (offsets[mid] <= g0) lo = mid;
        else hi = mid - 1;
    }
    tile_read[t] = lo;
}

template <int W>
__global__ void __launch_bounds__(256)
stream_encode_kernel(const char* __restrict__ bases, const uint64_t* __restrict__ offsets, const uint64_t* __restrict__ tile_read, const uint64_t n_reads,
                     const uint64_t total_bases, const uint64_t first, const uint64_t count, const uint32_t k,
                     uint64_t* __restrict__ kmers /* relative to `first` */, uint8_t* __restrict__ flags /* absolute */) {
    constexpr uint32_t TILE = 256, SPAN = TILE + 64;
    __shared__ uint32_t chars[SPAN / 4 + 2];
    /* the same characters as 2-bit codes back to back, and one "is A, C, G or T" bit per character: every lane then cuts
       its k-mer and its k validity bits out of these with funnel shifts (packing k characters per lane from `chars`
       cost ~100 VALU instructions per position: the encode pass took longer than the lookups it feeds) */
    __shared__ uint32_t codes[SPAN / 16 + 4];
    __shared__ uint32_t okay[SPAN / 32 + 4];
    __shared__ uint64_t ends[TILE + 2];  // offsets[r0 + 1 ...]: the read boundaries that may fall into the tile
    const uint64_t g0 = first + uint64_t(blockIdx.x) * TILE;
    const uint32_t tid = threadIdx.x;
    const uint64_t r0 = tile_read[blockIdx.x];  // the read holding the tile's first base
    /* the characters of the tile and the k - 1 after it */
    for (uint32_t c = tid; c < SPAN / 4 + 2; c += TILE) {
        const uint64_t at = g0 + 4 * uint64_t(c);
        uint32_t v = 0;
        if (at + 4 <= total_bases && ((reinterpret_cast<uintptr_t>(bases) + at) & 3) == 0) v = *reinterpret_cast<const uint32_t*>(bases + at);
        else
            for (uint32_t b = 0; b < 4; ++b)
                if (at + b < total_bases) v |= uint32_t(uint8_t(bases[at + b])) << (8 * b);
        chars[c] = v;
    }
    __syncthreads();
    for (uint32_t c = tid; c < SPAN / 4 + 2; c += TILE) {
        const uint32_t four = chars[c];
        uint32_t two = (four >> 1) & 0x03030303u;  // (c >> 1) & 3 (include/kmer.hpp:118) for four characters at once
        two = (two | (two >> 6) | (two >> 12) | (two >> 18)) & 0xFFu;
        reinterpret_cast<uint8_t*>(codes)[c] = uint8_t(two);
    }
    for (uint32_t q = tid; q < SPAN + 64; q += TILE) {  // uniform over each wave: whole waves take part in the ballot
        /* A C G T a c g t only (include/kmer.hpp:209-219): fold the case */
        const uint32_t u = (q < 4 * (SPAN / 4 + 2) ? reinterpret_cast<const uint8_t*>(chars)[q] : 0u) & 0xDFu;
        const uint64_t mask = __ballot(u == 0x41u || u == 0x43u || u == 0x47u || u == 0x54u);
        if ((q & 63u) == 0) {
            okay[q / 32] = uint32_t(mask);
            okay[q / 32 + 1] = uint32_t(mask >> 32);
        }
    }
    for (uint32_t c = tid; c < TILE + 2; c += TILE) ends[c] = r0 + 1 + c <= n_reads ? offsets[r0 + 1 + c] : ~uint64_t(0);
    __syncthreads();
    const uint64_t p = g0 + tid;
    if (tid >= count - uint64_t(blockIdx.x) * TILE || p >= total_bases) return;
    /* my read: r0 + the number of boundaries ends[.] <= p */
    uint32_t lo = 0, hi = TILE + 1;  // first index with ends[index] > p
    while (lo < hi) {
        const uint32_t mid = (lo + hi) / 2;
        if (ends[mid] <= p) lo = mid + 1;
        else hi = mid;
    }
    uint64_t begin, end;
    if (lo <= TILE) {
        end = ends[lo];
        begin = lo ? ends[lo - 1] : offsets[r0];
    } else {  // more than TILE reads begin inside the tile (empty reads): resolve this place on its own
        uint64_t a = r0, b = n_reads - 1;
        while (a < b) {
            const uint64_t mid = a + (b - a + 1) / 2;
            if (offsets[mid] <= p) a = mid;
            else b = mid - 1;
        }
        begin = offsets[a];
        end = offsets[a + 1];
    }
    uint8_t f = 0;
    kmer_w<W> x = kmer_zero<W>();
    /* (a place behind the last read's end -- the caller's total_bases exceeds read_offsets[num_reads] -- belongs to no read: no
       k-mer starts there; ADVICE r2: it used to be looked up as part of one endless read) */
    if (end != ~uint64_t(0) && p + k <= end) {
        const uint32_t cw = tid >> 4, cs = 2 * (tid & 15u);
        uint32_t word[2 * W];
        for (int j = 0; j < 2 * W; ++j) word[j] = __builtin_amdgcn_alignbit(codes[cw + j + 1], codes[cw + j], cs);
        for (int j = 0; j < W; ++j) x.w[j] = uint64_t(word[2 * j]) | (uint64_t(word[2 * j + 1]) << 32);
        x = kmer_take_chars<W>(x, k);
        const uint32_t vw = tid >> 5, vs = tid & 31u;
        const uint64_t ok = uint64_t(__builtin_amdgcn_alignbit(okay[vw + 1], okay[vw], vs)) |
                            (uint64_t(__builtin_amdgcn_alignbit(okay[vw + 2], okay[vw + 1], vs)) << 32);
        const bool valid = (~ok & low_mask(k)) == 0;  // k <= 63
        f = (valid ? SQ_VALID : SQ_INVALID) | (p == begin ? SQ_FIRST : 0);
    }
    flags[p] = f;
    for (int j = 0; j < W; ++j) kmers[(p - first) * W + j] = x.w[j];
}

__global__ void __launch_bounds__(256)
stream_classify_kernel(const uint8_t* __restrict__ flags, const uint64_t total_bases, const result_view out,
                       const uint64_t* string_id, const int8_t* orientation /* may be out's own arrays */, uint64_t* __restrict__ report,
                       const bool has_predecessor /* the arrays continue below index 0: a later piece of one call */) {
    /* grid-stride: the six counters are accumulated in registers and reach `report` once per wave -- one hot set of
       atomics per wave of 64 k-mers would serialise at ~90 atomics/us (HISTORY.md) */
    uint64_t c_kmer = 0, c_invalid = 0, c_negative = 0, c_search = 0, c_extension = 0;
    /* Four consecutive places per lane and turn, everything they may need requested at once (what a branch does not use
       is ignored): one load after the other, each behind its test, made a chain of round trips per place, and the pass
       ran at a quarter of the memory rate. `flags` is this file's own array (4-byte loads); the others may be the caller's. */
    constexpr uint32_t PLACES = 4;
    const uint64_t stride = uint64_t(gridDim.x) * blockDim.x * PLACES;
    for (uint64_t p0 = (uint64_t(blockIdx.x) * blockDim.x + threadIdx.x) * PLACES; p0 < total_bases; p0 += stride) {
        const int64_t q = (p0 || has_predecessor) ? int64_t(p0) - 1 : 0;  // only the call's very first place has no predecessor
        uint8_t f[PLACES + 1];
        uint64_t id[PLACES + 1], sid[PLACES + 1];
        int8_t ori[PLACES + 1];
        f[0] = flags[q];
        id[0] = out.kmer_id[q];
        sid[0] = string_id[q];
        ori[0] = orientation[q];
        const bool whole = p0 + PLACES <= total_bases && ((reinterpret_cast<uintptr_t>(flags) + p0) & 3) == 0;
        const uint32_t four = whole ? *reinterpret_cast<const uint32_t*>(flags + p0) : 0u;
#pragma unroll
        for (uint32_t j = 0; j < PLACES; ++j) {
            const uint64_t p = p0 + j < total_bases ? p0 + j : total_bases - 1;
            f[j + 1] = whole ? uint8_t(four >> (8 * j)) : flags[p];
            id[j + 1] = out.kmer_id[p];
            sid[j + 1] = string_id[p];
            ori[j + 1] = orientation[p];
        }
#pragma unroll
        for (uint32_t j = 0; j < PLACES; ++j) {
            const uint64_t p = p0 + j;
            if (p >= total_bases) break;
            if (f[j + 1] & SQ_INVALID) {
                /* what streaming_query::lookup returns after its reset(): a default lookup_result (include/util.hpp:38-62) */
                ++c_kmer;
                ++c_invalid;
                out.kmer_id[p] = INVALID_U64;
                if (out.kmer_id_in_string) out.kmer_id_in_string[p] = INVALID_U64;
                if (out.kmer_offset) out.kmer_offset[p] = INVALID_U64;
                if (out.string_id) out.string_id[p] = INVALID_U64;
                if (out.string_begin) out.string_begin[p] = INVALID_U64;
                if (out.string_end) out.string_end[p] = INVALID_U64;
                if (out.kmer_orientation) out.kmer_orientation[p] = 1;
            } else if (f[j + 1] & SQ_VALID) {
                ++c_kmer;
                if (id[j + 1] == INVALID_U64) {
                    ++c_negative;
                } else {
                    const bool extension = !(f[j + 1] & SQ_FIRST) && (f[j] & SQ_VALID) && continues_run(id[j], sid[j], ori[j], id[j + 1], sid[j + 1]);
                    c_extension += extension;
                    c_search += !extension;
                }
            }
        }
    }
    if (!report) return;  // uniform
    block_report(c_kmer, c_invalid, c_negative, c_search, c_extension, report);
}

/* The classification once more, into one report PER READ: one lane per place; rows[6 r ..] += what the k-mers of read r add to the six
   counters (the rows are zeroed by the caller). A read of a megabase is a million lanes on one row, so the lanes of a wave first sum
   over their runs of equal read: a run begins at the wave's first k-mer and at every k-mer that is the first of its read (a k-mer
   belongs to the read of the k-mer before it unless it is marked SQ_FIRST; places without a k-mer add nothing and need no read), what
   a k-mer adds to a counter is one bit, so a run's sum is a ballot, masked by the run's lanes and counted, and the run's first lane --
   the only one to look its read up in the offsets -- adds the sums that are not zero: at most one atomic per wave, read and counter. */
__global__ void __launch_bounds__(256)
stream_classify_rows_kernel(const uint8_t* __restrict__ flags, const uint64_t total_bases, const uint64_t* __restrict__ kmer_id,
                            const uint64_t* __restrict__ string_id, const int8_t* __restrict__ orientation,
                            const uint64_t* __restrict__ offsets, const uint64_t n_reads, uint64_t* __restrict__ rows) {
    const uint64_t p = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u;
    const uint8_t f = p < total_bases ? flags[p] : uint8_t(0);
    const bool has = (f & (SQ_VALID | SQ_INVALID)) != 0, invalid = (f & SQ_INVALID) != 0;
    bool negative = false, search = false, extension = false;
    if (!invalid && (f & SQ_VALID)) {
        const uint64_t id = kmer_id[p];
        if (id == INVALID_U64) {
            negative = true;
        } else {
            if (!(f & SQ_FIRST) && p > 0 && (flags[p - 1] & SQ_VALID)) {  // (as stream_classify_kernel)
                extension = continues_run(kmer_id[p - 1], string_id[p - 1], orientation[p - 1], id, string_id[p]);
            }
            search = !extension;
        }
    }
    const uint64_t have = __ballot(has);
    if (have == 0) return;  // (uniform)
    const uint64_t below = (uint64_t(1) << lane) - 1;
    const bool head = has && ((f & SQ_FIRST) || (have & below) == 0);
    const uint64_t heads = __ballot(head);
    const uint64_t m_invalid = __ballot(invalid), m_negative = __ballot(negative), m_search = __ballot(search), m_extension = __ballot(extension);
    if (!head) return;
    const uint64_t above = (heads >> lane) >> 1;  // the heads behind this lane
    const uint32_t end = above ? lane + 1 + uint32_t(__builtin_ctzll(above)) : 64u;
    const uint64_t mine = (end == 64 ? ~uint64_t(0) : (uint64_t(1) << end) - 1) & ~below;  // the lanes of my run
    uint64_t lo = 0, hi = n_reads - 1;  // my read: the largest r with offsets[r] <= p
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo + 1) / 2;
        if (offsets[mid] <= p) lo = mid;
        else hi = mid - 1;
    }
    unsigned long long* const row = reinterpret_cast<unsigned long long*>(rows + 6 * lo);
    const unsigned long long n_kmers = __popcll(have & mine), n_invalid = __popcll(m_invalid & mine), n_negative = __popcll(m_negative & mine),
                             n_search = __popcll(m_search & mine), n_extension = __popcll(m_extension & mine);
    atomicAdd(row + 0, n_kmers);
    if (n_search + n_extension) atomicAdd(row + 1, n_search + n_extension);
    if (n_negative) atomicAdd(row + 2, n_negative);
    if (n_invalid) atomicAdd(row + 3, n_invalid);
    if (n_search) atomicAdd(row + 4, n_search);
    if (n_extension) atomicAdd(row + 5, n_extension);
}

/* ---- the runs out of the per-k-mer results (the host call's route for reads too long for one lane): a positive k-mer is the HEAD of a run
        unless it continues the run of the k-mer before it -- the rule of the classification above --; the heads' ranks in place order are
        their places in the CSR layout (reads lie in place order), so one scan over the marks gives run_offsets -- the rank at every
        read's first base -- and every head's place; a head's lane then walks to the first k-mer that does not continue its run. One lane
        a place: rare inputs, correctness first. ---- */
constexpr uint8_t RUN_HEAD = 1, RUN_CONTINUES = 2;

__global__ void __launch_bounds__(256)
stream_run_marks_kernel(const uint8_t* __restrict__ flags, const uint64_t total_bases, const uint64_t* __restrict__ kmer_id,
                        const uint64_t* __restrict__ string_id, const int8_t* __restrict__ orientation, uint8_t* __restrict__ marks /* total_bases + 1 */,
                        uint64_t* __restrict__ rank /* total_bases + 1 */) {
    const uint64_t p = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (p > total_bases) return;
    uint8_t mark = 0;
    if (p < total_bases) {
        const uint8_t f = flags[p];
        if (!(f & SQ_INVALID) && (f & SQ_VALID)) {
            const uint64_t id = kmer_id[p];
            if (id != INVALID_U64) {
                bool extension = false;
                if (!(f & SQ_FIRST) && p > 0 && (flags[p - 1] & SQ_VALID)) {  // (as stream_classify_kernel)
                    extension = continues_run(kmer_id[p - 1], string_id[p - 1], orientation[p - 1], id, string_id[p]);
                }
                mark = extension ? RUN_CONTINUES : RUN_HEAD;
            }
        }
    }
    marks[p] = mark;
    rank[p] = mark == RUN_HEAD ? 1 : 0;
}

__global__ void __launch_bounds__(256)
stream_run_offsets_kernel(const uint64_t* __restrict__ rank, const uint64_t total_bases, const uint64_t* __restrict__ offsets, const uint64_t n_reads,
                          uint64_t* __restrict__ run_offsets) {
    const uint64_t r = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (r > n_reads) return;
    const uint64_t at = offsets[r];
    run_offsets[r] = rank[at < total_bases ? at : total_bases];
}

__global__ void __launch_bounds__(256)
stream_run_records_kernel(const uint8_t* __restrict__ marks, const uint64_t* __restrict__ rank, const uint64_t total_bases,
                          const uint64_t* __restrict__ kmer_id, const uint64_t* __restrict__ string_id, const uint64_t* __restrict__ kmer_id_in_string,
                          const int8_t* __restrict__ orientation, const uint64_t* __restrict__ offsets, const uint64_t n_reads, const run_sink sink) {
    const uint64_t p = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (p >= total_bases || marks[p] != RUN_HEAD) return;
    const uint64_t at = rank[p];
    if (at >= sink.capacity) return;
    uint64_t n = 1;
    while (marks[p + n] == RUN_CONTINUES) ++n;  // (marks[total_bases] = 0 ends the last)
    uint64_t lo = 0, hi = n_reads - 1;  // my read: the largest r with offsets[r] <= p
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo + 1) / 2;
        if (offsets[mid] <= p) lo = mid;
        else hi = mid - 1;
    }
    const uint64_t id = kmer_id[p], in_string = kmer_id_in_string[p];
    uint4* const rec = static_cast<uint4*>(sink.records) + 2 * at;
    rec[0] = make_uint4(uint32_t(id), uint32_t(id >> 32), uint32_t(string_id[p]), uint32_t(string_id[p] >> 32));
    rec[1] = make_uint4(uint32_t(in_string), uint32_t(in_string >> 32), uint32_t(p - offsets[lo]), uint32_t(n) | (orientation[p] > 0 ? 0u : 0x80000000u));
}

/* ---- the cover out of the per-k-mer results (the host calls' route for reads too long for one lane): one lane a place, the bit of its
        k-mer's id ORed into the bitmap. Along a hit the ids of neighbouring places are neighbours, 64 of them in a word: the lanes of a
        wave first OR their bits together wherever a lane further on holds the same word (any two bits of one word may be merged, whatever
        lies between their lanes), and a lane whose predecessor holds that word leaves the atomic to it. ---- */
__global__ void __launch_bounds__(256)
cover_mark_ids_kernel(const uint8_t* __restrict__ flags, const uint64_t* __restrict__ kmer_id, const uint64_t total_bases, uint64_t* __restrict__ cover) {
    const uint64_t p = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u;
    uint64_t word = ~uint64_t(0), bits = 0;  // (no k-mer, or not in the dictionary: no word)
    if (p < total_bases && (flags[p] & SQ_VALID)) {
        const uint64_t id = kmer_id[p];
        if (id != INVALID_U64) {
            word = id >> 6;
            bits = uint64_t(1) << (id & 63u);
        }
    }
    if (__ballot(bits != 0) == 0) return;  // (uniform)
    const uint64_t before = __shfl_up(word, 1, 64);
    for (uint32_t o = 1; o < 64; o <<= 1) {
        const uint64_t w = __shfl_down(word, o, 64), b = __shfl_down(bits, o, 64);
        if (lane + o < 64 && w == word) bits |= b;
    }
    if (bits == 0 || (lane > 0 && before == word)) return;
    (void)__hip_atomic_fetch_or(reinterpret_cast<unsigned long long*>(cover) + word, (unsigned long long)bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

/* ---- the depth's deltas out of the per-k-mer results (the host calls' route for reads too long for one lane): one lane a place, +1 at
        its k-mer's id and -1 behind it. Along a hit the next place holds the next id (forward) or the one before (backward), and then a
        +1 and a -1 meet in one word: the pair (p, p + 1) takes both away -- forward the -1 of p and the +1 of p + 1, backward the +1 of p
        and the -1 of p + 1 --, so that a run costs what it costs the run kernel and only its ends reach memory. A lane looks at both its
        neighbours (whatever read they lie in: the sum is all that counts) and adds what is left of its two words, each -1, 0 or +1. ---- */
__global__ void __launch_bounds__(256)
depth_mark_ids_kernel(const uint8_t* __restrict__ flags, const uint64_t* __restrict__ kmer_id, const uint64_t total_bases, const uint64_t num_kmers,
                      uint32_t* __restrict__ deltas) {
    const uint64_t p = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    auto id_at = [&](uint64_t q) { return q < total_bases && (flags[q] & SQ_VALID) ? kmer_id[q] : INVALID_U64; };  // (p - 1 at p = 0: no place)
    const uint64_t id = id_at(p);
    if (id == INVALID_U64 || id >= num_kmers) return;
    const uint64_t before = id_at(p - 1), after = id_at(p + 1);
    const bool has_before = before != INVALID_U64, has_after = after != INVALID_U64;
    const uint32_t plus = 1u - uint32_t(has_before && before + 1 == id) - uint32_t(has_after && after + 1 == id);
    const uint32_t minus = 1u - uint32_t(has_after && id + 1 == after) - uint32_t(has_before && id + 1 == before);
    if (plus) (void)__hip_atomic_fetch_add(deltas + id, plus, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (minus && id + 1 < num_kmers) (void)__hip_atomic_fetch_add(deltas + id + 1, 0u - minus, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

/* ---- the reads' sums out of the per-k-mer results (the host calls' route for reads too long for one lane, and for minimizer shards): one
        lane a place, its k-mer's value P[id + 1] - P[id] and 1 into the two words of its read's row. The stretches of one read are
        those of stream_classify_rows_kernel -- a stretch begins at the wave's first k-mer and at every k-mer that is the first of its read --;
        the lanes of a wave sum over their stretch (a segmented sum, as stream_segment_rows_kernel), and the stretch's first lane, the only
        one to look its read up in the offsets, adds what is not zero: at most one pair of atomics per wave and read. ---- */
__global__ void __launch_bounds__(256)
sums_add_ids_kernel(const uint8_t* __restrict__ flags, const uint64_t* __restrict__ kmer_id, const uint64_t total_bases, const uint64_t num_kmers,
                    const uint64_t* __restrict__ prefix, const uint64_t* __restrict__ offsets, const uint64_t n_reads, uint64_t* __restrict__ sums) {
    const uint64_t p = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u;
    const uint8_t f = p < total_bases ? flags[p] : uint8_t(0);
    const bool has = (f & (SQ_VALID | SQ_INVALID)) != 0;
    uint64_t v = 0, n = 0;
    if (f & SQ_VALID) {
        const uint64_t id = kmer_id[p];
        if (id < num_kmers) {  // (INVALID_U64: not in the dictionary)
            v = prefix[id + 1] - prefix[id];
            n = 1;
        }
    }
    const uint64_t have = __ballot(has);
    if (__ballot(n != 0) == 0) return;  // (uniform)
    const uint64_t below = (uint64_t(1) << lane) - 1;
    const bool head = has && ((f & SQ_FIRST) || (have & below) == 0);
    const uint64_t heads = __ballot(head);
    const uint64_t mine_or_before = heads & (below | (uint64_t(1) << lane));
    const uint32_t stretch = mine_or_before ? 63u - uint32_t(__builtin_clzll(mine_or_before)) : 64u;  // the head of my stretch (64: a place before the wave's first k-mer)
    for (uint32_t o = 1; o < 64; o <<= 1) {
        const bool same = __shfl_down(stretch, o, 64) == stretch && lane + o < 64;
        const uint64_t further_v = __shfl_down(v, o, 64), further_n = __shfl_down(n, o, 64);
        if (same) {
            v += further_v;
            n += further_n;
        }
    }
    if (!head || n == 0) return;
    uint64_t lo = 0, hi = n_reads - 1;  // my read: the largest r with offsets[r] <= p
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo + 1) / 2;
        if (offsets[mid] <= p) lo = mid;
        else hi = mid - 1;
    }
    unsigned long long* const row = reinterpret_cast<unsigned long long*>(sums + 2 * lo);
    if (v) (void)__hip_atomic_fetch_add(row, (unsigned long long)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    (void)__hip_atomic_fetch_add(row + 1, (unsigned long long)n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

/* ---- the reads' rows by class out of the per-k-mer results (the same two callers): one lane a place, the label of its k-mer's string --
        none where no k-mer of the dictionary (or of this shard) starts, or where the label is no class. A stretch is here a run of
        lanes in one read's stretch (as above) WITH THE SAME LABEL; the lanes count over it, and its first lane, when the label is a
        class, finds its read and adds the count to that column: one atomic per stretch. ---- */
__global__ void __launch_bounds__(256)
classes_add_ids_kernel(const uint8_t* __restrict__ flags, const uint64_t* __restrict__ kmer_id, const uint64_t* __restrict__ string_id,
                       const uint64_t total_bases, const uint64_t num_kmers, const uint32_t* __restrict__ labels, const uint32_t classes,
                       const uint64_t* __restrict__ offsets, const uint64_t n_reads, uint32_t* __restrict__ rows) {
    constexpr uint32_t NO_CLASS = ~0u;
    const uint64_t p = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u;
    const uint8_t f = p < total_bases ? flags[p] : uint8_t(0);
    const bool has = (f & (SQ_VALID | SQ_INVALID)) != 0;
    uint32_t label = NO_CLASS;
    if ((f & SQ_VALID) && kmer_id[p] < num_kmers) {  // (INVALID_U64: not in the dictionary, and then its string means nothing)
        label = labels[string_id[p]];
        if (label >= classes) label = NO_CLASS;
    }
    uint32_t n = label != NO_CLASS ? 1u : 0u;
    const uint64_t have = __ballot(has);
    if (__ballot(n != 0) == 0) return;  // (uniform)
    const uint64_t below = (uint64_t(1) << lane) - 1, upto = below | (uint64_t(1) << lane);
    const uint64_t read_heads = __ballot(has && ((f & SQ_FIRST) || (have & below) == 0));
    const uint64_t mine_or_before = read_heads & upto;
    const uint32_t of_read = mine_or_before ? 63u - uint32_t(__builtin_clzll(mine_or_before)) : 64u;  // the head of my read's stretch (64: a place before the wave's first k-mer)
    /* (both shuffles before anything is decided: inside `a || b` the second would run with the lanes switched off that the first
       settled, and a lane whose neighbour is switched off reads nothing of it) */
    const uint32_t read_before = __shfl_up(of_read, 1, 64), label_before = __shfl_up(label, 1, 64);
    const bool head = lane == 0 || read_before != of_read || label_before != label;
    const uint64_t heads = __ballot(head);  // (lane 0 is one: never empty below)
    const uint32_t stretch = 63u - uint32_t(__builtin_clzll(heads & upto));
    for (uint32_t o = 1; o < 64; o <<= 1) {
        const bool same = __shfl_down(stretch, o, 64) == stretch && lane + o < 64;
        const uint32_t further = __shfl_down(n, o, 64);
        if (same) n += further;
    }
    if (!head || n == 0 || label == NO_CLASS) return;  // (n != 0: the stretch's label, mine, is a class, and a k-mer lies at p -- p lies in a read)
    uint64_t lo = 0, hi = n_reads - 1;  // my read: the largest r with offsets[r] <= p
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo + 1) / 2;
        if (offsets[mid] <= p) lo = mid;
        else hi = mid - 1;
    }
    (void)__hip_atomic_fetch_add(rows + lo * classes + label, n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

/* ---- covered k-mers per string: a segmented popcount of a cover bitmap. The ids of string s are [begin(s), begin(s + 1)),
        begin(s) = endpoints[s] - s * (k - 1); strings hold from one k-mer to millions, so the lanes go over the bitmap's WORDS, one each.
        A lane finds the string of its word's first id -- the workgroup's first lane by bisection over all strings, the others from
        there: every string holds a k-mer, so the string of an id j ids further on is at most j strings further on, and as a rule it
        is the same one or the next (a doubling search, then a bisection inside its last step) --, and cuts its word at every string
        boundary inside it. The strings that END inside the word get their piece with one atomic each; the last piece belongs to a string
        that may go on through the words of the lanes behind, so the lanes of a wave sum their last pieces over neighbours with the same
        string first (stream_classify_rows_kernel does that for rows), and the first lane of such a stretch adds the sum. `counts` is
        zeroed by the caller. The total: the popcount of the words, once a workgroup. ---- */
__device__ __forceinline__ uint64_t string_first_id(const uint64_t* __restrict__ endpoints, uint64_t s, uint32_t k) { return endpoints[s] - s * (k - 1); }

__global__ void __launch_bounds__(256)
cover_string_counts_kernel(const uint64_t* __restrict__ cover, const uint64_t num_kmers, const uint64_t* __restrict__ endpoints, const uint64_t num_strings,
                           const uint32_t k, uint64_t* __restrict__ counts, uint64_t* __restrict__ total) {
    __shared__ uint64_t block_string;
    __shared__ uint64_t block_sum[4];
    const uint64_t words = (num_kmers + 63) / 64;
    const uint64_t w = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u;
    if (threadIdx.x == 0) {  // the string of the workgroup's first id: the largest s with begin(s) <= id (w < words: the grid holds no empty workgroup)
        const uint64_t id = w * 64;
        uint64_t lo = 0, hi = num_strings - 1;
        while (lo < hi) {
            const uint64_t mid = lo + (hi - lo + 1) / 2;
            if (string_first_id(endpoints, mid, k) <= id) lo = mid;
            else hi = mid - 1;
        }
        block_string = lo;
    }
    __syncthreads();
    const bool has = w < words;
    uint64_t bits = 0;
    uint32_t last_string = ~0u, last_count = 0;
    if (has) {
        const uint64_t id0 = w * 64, id_end = id0 + 64 < num_kmers ? id0 + 64 : num_kmers;
        bits = cover[w];
        if (id_end - id0 < 64) bits &= (uint64_t(1) << (id_end - id0)) - 1;  // (bits at or above num_kmers are no k-mers)
        /* my first string: the largest s in [block_string, num_strings) with begin(s) <= id0 */
        uint64_t lo = block_string, step = 1;
        while (lo + step < num_strings && string_first_id(endpoints, lo + step, k) <= id0) {
            lo += step;
            step <<= 1;
        }
        uint64_t hi = lo + step - 1 < num_strings - 1 ? lo + step - 1 : num_strings - 1;  // (begin(lo + step) > id0, or there is no such string)
        while (lo < hi) {
            const uint64_t mid = lo + (hi - lo + 1) / 2;
            if (string_first_id(endpoints, mid, k) <= id0) lo = mid;
            else hi = mid - 1;
        }
        uint64_t s = lo, at = id0;
        for (;;) {
            const uint64_t next = string_first_id(endpoints, s + 1, k);  // (begin(num_strings) = num_kmers)
            if (next >= id_end) break;
            /* string s ends inside the word: ids [at, next) */
            const uint64_t piece = (bits >> (at - id0)) & ((uint64_t(1) << (next - at)) - 1);  // (next - at < 64: next < id_end)
            if (piece) atomicAdd(reinterpret_cast<unsigned long long*>(counts + s), (unsigned long long)__popcll(piece));
            at = next;
            ++s;
        }
        last_string = uint32_t(s);
        last_count = uint32_t(__popcll(bits >> (at - id0)));
    }
    /* the last pieces: summed over the lanes behind that are in the same string (they are neighbours: strings follow each other) */
    const uint32_t before = __shfl_up(last_string, 1, 64);
    for (uint32_t o = 1; o < 64; o <<= 1) {
        const uint32_t s = __shfl_down(last_string, o, 64), c = __shfl_down(last_count, o, 64);
        if (lane + o < 64 && s == last_string) last_count += c;
    }
    if (has && last_count && (lane == 0 || before != last_string))
        atomicAdd(reinterpret_cast<unsigned long long*>(counts + last_string), (unsigned long long)last_count);
    if (!total) return;  // (uniform)
    const uint64_t wave_bits = wave_sum(uint64_t(__popcll(bits)));
    if (lane == 0) block_sum[threadIdx.x >> 6] = wave_bits;
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint64_t sum = block_sum[0] + block_sum[1] + block_sum[2] + block_sum[3];
        if (sum) atomicAdd(reinterpret_cast<unsigned long long*>(total), (unsigned long long)sum);
    }
}

void engine::cover_string_counts_device(int device, uint64_t const* d_cover, uint64_t* d_counts, uint64_t* d_total, void* stream) const {
    device_replica const* rep = replica(device);
    if (!d_cover || !d_counts) throw error(error_kind::argument, "null pointer");
    device_guard guard(device);
    dict_view const& d = rep->view;
    hipStream_t s = hipStream_t(stream);
    HIP_CHECK(hipMemsetAsync(d_counts, 0, d.num_strings * sizeof(uint64_t), s));
    if (d_total) HIP_CHECK(hipMemsetAsync(d_total, 0, sizeof(uint64_t), s));
    const uint64_t words = (d.num_kmers + 63) / 64;
    if (words == 0 || d.num_strings == 0) return;
    hipLaunchKernelGGL(cover_string_counts_kernel, dim3(uint32_t((words + 255) / 256)), dim3(256), 0, s, d_cover, d.num_kmers, d.endpoints, d.num_strings, d.k,
                       d_counts, d_total);
    HIP_CHECK(hipGetLastError());
}

/* ---- depth per string: sums[s] = the 64-bit sum of depth over the ids of string s (the id ranges of cover_string_counts_kernel). One
        lane an id. Every string holds a k-mer, so the 256 ids of a workgroup lie in at most 256 strings, the first of which one lane finds
        by bisection: the first ids of the 256 strings behind it go to LDS, a lane finds its string among them (8 steps, no global load),
        the workgroup sums per string in LDS (a wave that lies inside one string: one add for the wave), and each string it met gets ONE global atomic. `sums` is zeroed by the caller. ---- */
__global__ void __launch_bounds__(256)
depth_string_sums_kernel(const uint32_t* __restrict__ depth, const uint64_t num_kmers, const uint64_t* __restrict__ endpoints, const uint64_t num_strings,
                         const uint32_t k, uint64_t* __restrict__ sums, uint64_t* __restrict__ total) {
    __shared__ uint64_t block_string;
    __shared__ uint64_t first_id_behind[256];       // of string block_string + 1 + j (all-ones: there is no such string)
    __shared__ unsigned long long string_sum[256];  // of string block_string + j
    __shared__ uint64_t block_sum[4];
    const uint64_t id0 = uint64_t(blockIdx.x) * 256, id = id0 + threadIdx.x;
    if (threadIdx.x == 0) {  // the largest s with begin(s) <= id0 (id0 < num_kmers: the grid holds no empty workgroup)
        uint64_t lo = 0, hi = num_strings - 1;
        while (lo < hi) {
            const uint64_t mid = lo + (hi - lo + 1) / 2;
            if (string_first_id(endpoints, mid, k) <= id0) lo = mid;
            else hi = mid - 1;
        }
        block_string = lo;
    }
    __syncthreads();
    const uint64_t behind = block_string + 1 + threadIdx.x;
    first_id_behind[threadIdx.x] = behind <= num_strings ? string_first_id(endpoints, behind, k) : ~uint64_t(0);  // (begin(num_strings) = num_kmers)
    string_sum[threadIdx.x] = 0;
    __syncthreads();
    uint64_t v = 0;
    uint32_t mine_at = 0;  // my string, counted from block_string (a lane behind the last id: none, and nothing to add)
    const bool has = id < num_kmers;
    if (has) {
        v = depth[id];
        /* how many of those strings begin at or before id: first_id_behind[j] > id0 + j, so fewer than 256 */
        uint32_t lo = 0, hi = 256;
        while (lo < hi) {
            const uint32_t mid = (lo + hi) / 2;
            if (first_id_behind[mid] <= id) lo = mid + 1;
            else hi = mid;
        }
        mine_at = lo;
    }
    /* strings hold hundreds of k-mers as a rule: a wave that lies in one string adds its sum once, a wave that does not adds lane by lane */
    const uint32_t wave_at = __shfl(mine_at, 0, 64);
    const uint64_t wave_total = wave_sum(v);
    if (__ballot(has && mine_at != wave_at) == 0) {
        if ((threadIdx.x & 63u) == 0 && wave_total) atomicAdd(string_sum + wave_at, (unsigned long long)wave_total);
    } else if (v) {
        atomicAdd(string_sum + mine_at, (unsigned long long)v);
    }
    __syncthreads();
    const unsigned long long mine = string_sum[threadIdx.x];
    if (mine) atomicAdd(reinterpret_cast<unsigned long long*>(sums + block_string + threadIdx.x), mine);
    if (!total) return;  // (uniform)
    if ((threadIdx.x & 63u) == 0) block_sum[threadIdx.x >> 6] = wave_total;
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint64_t sum = block_sum[0] + block_sum[1] + block_sum[2] + block_sum[3];
        if (sum) atomicAdd(reinterpret_cast<unsigned long long*>(total), (unsigned long long)sum);
    }
}

void engine::depth_string_sums_device(int device, uint32_t const* d_depth, uint64_t* d_sums, uint64_t* d_total, void* stream) const {
    device_replica const* rep = replica(device);
    if (!d_depth || !d_sums) throw error(error_kind::argument, "null pointer");
    device_guard guard(device);
    dict_view const& d = rep->view;
    hipStream_t s = hipStream_t(stream);
    HIP_CHECK(hipMemsetAsync(d_sums, 0, d.num_strings * sizeof(uint64_t), s));
    if (d_total) HIP_CHECK(hipMemsetAsync(d_total, 0, sizeof(uint64_t), s));
    if (d.num_kmers == 0 || d.num_strings == 0) return;
    const uint64_t blocks = (d.num_kmers + 255) / 256;
    if (blocks >> 31) throw error(error_kind::argument, "too many k-mers for one launch");
    hipLaunchKernelGGL(depth_string_sums_kernel, dim3(uint32_t(blocks)), dim3(256), 0, s, d_depth, d.num_kmers, d.endpoints, d.num_strings, d.k, d_sums, d_total);
    HIP_CHECK(hipGetLastError());
}

/* ---- the finish of the class rows. BEST: a group of `group` lanes (a power of two, at most 64: class_group) per read strides over the
        read's row; a lane keeps the largest count it met, the first class that had it and the largest of the others, `group` of those are
        merged by butterfly shuffles, the group's first lane stores the read's four words
        {best_class, best, second, total}. A count takes the lead only when it is LARGER: among equals the smallest class stays, and a
        row of zeros keeps the class it began with, NO_CLASS. ---- */
struct class_lead {
    uint32_t best, cls, second;
};
__device__ __forceinline__ class_lead class_merge(class_lead a, class_lead b) {
    const bool b_leads = b.best > a.best || (b.best == a.best && b.cls < a.cls);
    const class_lead w = b_leads ? b : a, l = b_leads ? a : b;
    return class_lead{w.best, w.cls, l.best > w.second ? l.best : w.second};  // (the loser's second is at most its best)
}
__global__ void __launch_bounds__(256)
class_best_kernel(const uint32_t* __restrict__ rows, const uint64_t n_reads, const uint32_t classes, const uint32_t group, uint32_t* __restrict__ out) {
    const uint64_t t = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    const uint64_t r = t / group;  // (a group lies in one wave: 64 is a multiple of it)
    const uint32_t sub = uint32_t(t) & (group - 1);
    class_lead mine{0u, ~0u, 0u};
    uint32_t total = 0;
    if (r < n_reads) {
        const uint32_t* const row = rows + r * classes;
        for (uint32_t c = sub; c < classes; c += group) {  // (ascending: the first class with the lane's largest count is its smallest)
            const uint32_t v = row[c];
            total += v;
            if (v > mine.best) {
                mine.second = mine.best;
                mine.best = v;
                mine.cls = c;
            } else if (v > mine.second) {
                mine.second = v;
            }
        }
    }
    for (uint32_t o = 1; o < group; o <<= 1) {  // (lane ^ o stays inside the group; every lane of the wave is here)
        const class_lead other{uint32_t(__shfl_xor(mine.best, o, 64)), uint32_t(__shfl_xor(mine.cls, o, 64)), uint32_t(__shfl_xor(mine.second, o, 64))};
        total += uint32_t(__shfl_xor(total, o, 64));
        mine = class_merge(mine, other);
    }
    if (r < n_reads && sub == 0) {
        uint32_t* const words = out + 4 * r;
        words[0] = mine.cls;
        words[1] = mine.best;
        words[2] = mine.second;
        words[3] = total;
    }
}

/* G = min(64, the smallest power of two >= classes) */
static uint32_t class_group(uint32_t classes) {
    uint32_t g = 1;
    while (g < classes && g < 64) g <<= 1;
    return g;
}

void engine::class_best_device(int device, uint32_t const* d_rows, uint64_t n_reads, uint32_t num_classes, uint32_t* d_best, void* stream) const {
    replica(device);  // (not resident: that error first)
    if (n_reads == 0) return;
    if (!d_rows || !d_best) throw error(error_kind::argument, "null pointer");
    if (num_classes == 0 || num_classes > MAX_CLASSES) throw error(error_kind::argument, "num_classes must be 1 .. 4096");
    device_guard guard(device);
    const uint32_t group = class_group(num_classes);
    const uint64_t blocks = (n_reads + 256 / group - 1) / (256 / group);
    if (blocks >> 31) throw error(error_kind::argument, "too many reads for one launch");
    hipLaunchKernelGGL(class_best_kernel, dim3(uint32_t(blocks)), dim3(256), 0, hipStream_t(stream), d_rows, n_reads, num_classes, group, d_best);
    HIP_CHECK(hipGetLastError());
}

/* ---- TOTALS: the 64-bit sum of every column over the reads. A workgroup takes `block_reads` reads. With 256 classes or more lane t sums
        the columns t, t + 256, ... over them; with fewer, 256 / classes reads are taken side by side -- lane t is on column t % classes
        of every (256 / classes)-th read -- and the lanes of a column meet in LDS. Either way consecutive lanes read consecutive words,
        and one 64-bit atomic per column and workgroup goes into the zeroed totals. ---- */
__global__ void __launch_bounds__(256)
class_totals_kernel(const uint32_t* __restrict__ rows, const uint64_t n_reads, const uint32_t classes, const uint64_t block_reads,
                    uint64_t* __restrict__ totals) {
    __shared__ uint64_t part[256];
    const uint64_t first = uint64_t(blockIdx.x) * block_reads, last = first + block_reads < n_reads ? first + block_reads : n_reads;
    unsigned long long* const out = reinterpret_cast<unsigned long long*>(totals);
    if (classes >= 256) {
        for (uint32_t c = threadIdx.x; c < classes; c += 256) {
            uint64_t sum = 0;
            for (uint64_t r = first; r < last; ++r) sum += rows[r * classes + c];
            if (sum) (void)__hip_atomic_fetch_add(out + c, (unsigned long long)sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        return;
    }
    const uint32_t side = 256 / classes, c = threadIdx.x % classes, mine = threadIdx.x / classes;  // (lanes at or past side * classes: none)
    uint64_t sum = 0;
    if (mine < side)
        for (uint64_t r = first + mine; r < last; r += side) sum += rows[r * classes + c];
    part[threadIdx.x] = sum;
    __syncthreads();
    if (threadIdx.x < classes) {
        for (uint32_t i = 1; i < side; ++i) sum += part[threadIdx.x + i * classes];
        if (sum) (void)__hip_atomic_fetch_add(out + c, (unsigned long long)sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

void engine::class_totals_device(int device, uint32_t const* d_rows, uint64_t n_reads, uint32_t num_classes, uint64_t* d_totals, void* stream) const {
    replica(device);  // (not resident: that error first)
    if (!d_totals || (n_reads && !d_rows)) throw error(error_kind::argument, "null pointer");
    if (num_classes == 0 || num_classes > MAX_CLASSES) throw error(error_kind::argument, "num_classes must be 1 .. 4096");
    device_guard guard(device);
    hipStream_t s = hipStream_t(stream);
    HIP_CHECK(hipMemsetAsync(d_totals, 0, num_classes * sizeof(uint64_t), s));
    if (n_reads == 0) return;
    const uint64_t block_reads = std::max<uint64_t>(1, (uint64_t(1) << 16) / num_classes);  // (some 2^16 words a workgroup)
    const uint64_t blocks = (n_reads + block_reads - 1) / block_reads;
    if (blocks >> 31) throw error(error_kind::argument, "too many reads for one launch");
    hipLaunchKernelGGL(class_totals_kernel, dim3(uint32_t(blocks)), dim3(256), 0, s, d_rows, n_reads, num_classes, block_reads, d_totals);
    HIP_CHECK(hipGetLastError());
}

/* ---- the finish of a complete CSR of run records: per read its longest run, among equals the first (sshash_runs_best_device). One lane a
        RECORD, so that a read with thousands of runs costs what any other costs: the lane finds its read by bisection over run_offsets
        (as stream_segment_fill_kernel finds a segment's read) and issues one 64-bit atomic max, nothing coming back, into the read's word
        of `keys`, zeroed before: (length << 32) | (0xFFFFFFFF - the record's index within its read) -- the largest key is the longest run
        and among equals the earliest; bit 31 of num_kmers, the strand, takes no part. A real run has a length of at least 1, so a key of
        0 is "no record". The number of records, run_offsets[n_reads], stays on the device: the lanes stride over them. Then one lane a
        READ copies the record its key names, or stores 32 zero bytes. ---- */
__global__ void __launch_bounds__(256)
runs_best_kernel(const uint64_t* __restrict__ run_offsets, const uint4* __restrict__ runs, const uint64_t n_reads, unsigned long long* __restrict__ keys) {
    const uint64_t n_records = run_offsets[n_reads], stride = uint64_t(gridDim.x) * blockDim.x;
    for (uint64_t i = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < n_records; i += stride) {
        uint64_t lo = 0, hi = n_reads - 1;  // my read: the largest r with run_offsets[r] <= i (i < run_offsets[n_reads]: its range is not empty and holds i)
        while (lo < hi) {
            const uint64_t mid = lo + (hi - lo + 1) / 2;
            if (run_offsets[mid] <= i) lo = mid;
            else hi = mid - 1;
        }
        const uint32_t length = runs[2 * i + 1].w & 0x7FFFFFFFu;
        const unsigned long long key = ((unsigned long long)length << 32) | (0xFFFFFFFFu - uint32_t(i - run_offsets[lo]));
        (void)__hip_atomic_fetch_max(keys + lo, key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

__global__ void __launch_bounds__(256)
runs_best_pick_kernel(const uint64_t* __restrict__ run_offsets, const uint4* __restrict__ runs, const uint64_t n_reads,
                      const unsigned long long* __restrict__ keys, uint4* __restrict__ best) {
    const uint64_t r = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (r >= n_reads) return;
    const unsigned long long key = keys[r];
    uint4 a = make_uint4(0u, 0u, 0u, 0u), b = a;
    if (key) {
        const uint64_t i = run_offsets[r] + (0xFFFFFFFFu - uint32_t(key));
        a = runs[2 * i];
        b = runs[2 * i + 1];
    }
    best[2 * r] = a;
    best[2 * r + 1] = b;
}

void engine::runs_best_device(int device, uint64_t const* d_run_offsets, void const* d_runs, uint64_t n_reads, void* d_best, void* stream) const {
    device_replica const* rep = replica(device);  // (not resident: that error first)
    if (n_reads == 0) return;
    if (!d_run_offsets || !d_best) throw error(error_kind::argument, "null pointer");
    const uint64_t blocks = (n_reads + 255) / 256;
    if (blocks >> 31) throw error(error_kind::argument, "too many reads for one launch");
    device_guard guard(device);
    hipStream_t s = hipStream_t(stream);
    device_buffers tmp(rep, s);  // (stream-ordered, out of the replica's pool: handed back behind the pick launch)
    unsigned long long* keys = tmp.alloc<unsigned long long>(n_reads);
    HIP_CHECK(hipMemsetAsync(keys, 0, n_reads * sizeof(unsigned long long), s));
    /* (as many workgroups as keep the chip busy; a CSR without a record runs the key pass for nothing and reads no record) */
    hipLaunchKernelGGL(runs_best_kernel, dim3(256 * 8), dim3(256), 0, s, d_run_offsets, static_cast<uint4 const*>(d_runs), n_reads, keys);
    hipLaunchKernelGGL(runs_best_pick_kernel, dim3(uint32_t(blocks)), dim3(256), 0, s, d_run_offsets, static_cast<uint4 const*>(d_runs), n_reads, keys,
                       static_cast<uint4*>(d_best));
    HIP_CHECK(hipGetLastError());
}

void engine::streaming_lookup_device(int device, char const* d_bases, uint64_t const* d_read_offsets, uint64_t n_reads,
                                     uint64_t total_bases, result_view const& d_out, uint64_t* d_report, void* stream, per_kmer_outputs const& more) const {
    device_replica const* rep = replica(device);
    run_sink const* const runs = more.runs;
    if ((more.prefix != nullptr) != (more.sums != nullptr)) throw error(error_kind::internal, "the sums go with their prefix");
    if ((more.labels != nullptr) != (more.class_rows != nullptr) || (more.labels && more.num_classes == 0)) throw error(error_kind::internal, "the class rows go with their labels");
    if (!d_out.kmer_id && !d_report && !more.rows && !runs && !more.cover && !more.deltas && !more.sums && !more.class_rows) throw error(error_kind::argument, "neither a kmer_id array nor a report to fill");
    if (d_out.minimizer_found) throw error(error_kind::argument, "the streaming lookup does not report minimizer_found");
    if (n_reads == 0 || total_bases == 0) return;
    device_guard guard(device);
    hipStream_t s = hipStream_t(stream);
    dict_view const& d = rep->view;
    const uint32_t W = d.k <= 31 ? 1 : 2;
    const uint64_t chunk = std::min<uint64_t>(total_bases, uint64_t(1) << 27);
    device_buffers tmp(rep, s);  // (stream-ordered; an exception between allocation and release must not leak them: ADVICE r2)
    uint64_t* sid = d_out.string_id;
    int8_t* ori = d_out.kmer_orientation;
    uint64_t* ids = d_out.kmer_id;  // null: counters only (streaming_query_host over reads too long for one lane each)
    if (!ids) ids = tmp.alloc<uint64_t>(total_bases);
    uint8_t* flags = tmp.alloc<uint8_t>(total_bases);
    uint64_t* kmers = tmp.alloc<uint64_t>(chunk * W);
    uint64_t* tile_read = tmp.alloc<uint64_t>((chunk + 255) / 256);
    if (!sid) sid = tmp.alloc<uint64_t>(total_bases);
    if (!ori) ori = tmp.alloc<int8_t>(total_bases);
    uint64_t* in_string = d_out.kmer_id_in_string;
    if (runs && !in_string) in_string = tmp.alloc<uint64_t>(total_bases);
    result_view all = d_out;
    all.kmer_id_in_string = in_string;
    all.kmer_id = ids;
    all.string_id = sid;
    all.kmer_orientation = ori;
    for (uint64_t first = 0; first < total_bases; first += chunk) {
        const uint64_t count = std::min(chunk, total_bases - first);
        const dim3 grid(uint32_t((count + 255) / 256)), block(256);
        hipLaunchKernelGGL(stream_tile_reads_kernel, dim3((grid.x + 255) / 256), block, 0, s, d_read_offsets, n_reads, first, uint64_t(grid.x), tile_read);
        if (W == 1) hipLaunchKernelGGL(stream_encode_kernel<1>, grid, block, 0, s, d_bases, d_read_offsets, tile_read, n_reads, total_bases, first, count, d.k, kmers, flags);
        else hipLaunchKernelGGL(stream_encode_kernel<2>, grid, block, 0, s, d_bases, d_read_offsets, tile_read, n_reads, total_bases, first, count, d.k, kmers, flags);
        HIP_CHECK(hipGetLastError());
        lookup_packed_masked_device(device, kmers, flags + first, count, true, out_mode::full, advance(all, first), s);
    }
    result_view out = d_out;  // (the caller's arrays, kmer_id or its stand-in)
    out.kmer_id = ids;
    for (uint64_t first = 0; first < total_bases; first += uint64_t(1) << 30) {
        const uint64_t count = std::min<uint64_t>(uint64_t(1) << 30, total_bases - first);
        hipLaunchKernelGGL(stream_classify_kernel, dim3(uint32_t(std::min<uint64_t>((count + 1023) / 1024, 2048))), dim3(256), 0, s, flags + first, count,
                           advance(out, first), sid + first, ori + first, d_report, first != 0);
        HIP_CHECK(hipGetLastError());
    }
    if (more.rows) {
        hipLaunchKernelGGL(stream_classify_rows_kernel, dim3(uint32_t((total_bases + 255) / 256)), dim3(256), 0, s, flags, total_bases, ids, sid, ori,
                           d_read_offsets, n_reads, more.rows);
        HIP_CHECK(hipGetLastError());
    }
    if (more.cover) {
        hipLaunchKernelGGL(cover_mark_ids_kernel, dim3(uint32_t((total_bases + 255) / 256)), dim3(256), 0, s, flags, ids, total_bases, more.cover);
        HIP_CHECK(hipGetLastError());
    }
    if (more.deltas) {
        hipLaunchKernelGGL(depth_mark_ids_kernel, dim3(uint32_t((total_bases + 255) / 256)), dim3(256), 0, s, flags, ids, total_bases, d.num_kmers, more.deltas);
        HIP_CHECK(hipGetLastError());
    }
    if (more.sums) {
        hipLaunchKernelGGL(sums_add_ids_kernel, dim3(uint32_t((total_bases + 255) / 256)), dim3(256), 0, s, flags, ids, total_bases, d.num_kmers, more.prefix,
                           d_read_offsets, n_reads, more.sums);
        HIP_CHECK(hipGetLastError());
    }
    if (more.class_rows) {
        hipLaunchKernelGGL(classes_add_ids_kernel, dim3(uint32_t((total_bases + 255) / 256)), dim3(256), 0, s, flags, ids, sid, total_bases, d.num_kmers, more.labels,
                           more.num_classes, d_read_offsets, n_reads, more.class_rows);
        HIP_CHECK(hipGetLastError());
    }
    if (runs) {
        const uint64_t places = total_bases + 1;
        uint8_t* marks = tmp.alloc<uint8_t>(places);
        uint64_t* rank = tmp.alloc<uint64_t>(places);
        uint64_t* sums = tmp.alloc<uint64_t>(scan_tiles(places));
        hipLaunchKernelGGL(stream_run_marks_kernel, dim3(uint32_t((places + 255) / 256)), dim3(256), 0, s, flags, total_bases, ids, sid, ori, marks, rank);
        HIP_CHECK(hipGetLastError());
        exclusive_scan_u64(rank, places, sums, s);
        hipLaunchKernelGGL(stream_run_offsets_kernel, dim3(uint32_t((n_reads + 256) / 256)), dim3(256), 0, s, rank, total_bases, d_read_offsets, n_reads, runs->run_offsets);
        if (runs->capacity)
            hipLaunchKernelGGL(stream_run_records_kernel, dim3(uint32_t((total_bases + 255) / 256)), dim3(256), 0, s, marks, rank, total_bases, ids, sid, in_string, ori,
                               d_read_offsets, n_reads, *runs);
        HIP_CHECK(hipGetLastError());
    }
}

/* the six counters accumulated at d_report on the device, read back once the work on `s` is done */
static streaming_report read_back(uint64_t const* d_report, hipStream_t s) {
    uint64_t h[6];
    HIP_CHECK(hipMemcpyAsync(h, d_report, sizeof(h), hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    return streaming_report::from_device(h);
}

namespace {

/* Pieces of whole reads: piece i is the reads [cuts[i], cuts[i + 1]), with at most `piece_bases` bases (a single longer read is its own
   piece) and at most `piece_reads` reads. */
struct piece_cuts {
    std::vector<uint64_t> cuts{0};
    uint64_t max_bases = 0, max_reads = 0;  // of the largest piece
    uint64_t count() const { return cuts.size() - 1; }
};

piece_cuts cut_pieces(uint64_t const* read_offsets, uint64_t n_reads, uint64_t piece_bases, uint64_t piece_reads) {
    piece_cuts p;
    for (uint64_t at = 0; at < n_reads;) {
        uint64_t end = at + 1;
        while (end < n_reads && end - at < piece_reads && read_offsets[end + 1] - read_offsets[at] <= piece_bases) ++end;
        p.max_bases = std::max(p.max_bases, read_offsets[end] - read_offsets[at]);
        p.max_reads = std::max(p.max_reads, end - at);
        p.cuts.push_back(end);
        at = end;
    }
    return p;
}

}  // namespace

/* Host buffers: pieces of whole reads (at most ~64 MiB of bases each) go through one stream: H2D, the device pipeline
   above, D2H of the arrays the caller asked for. */
streaming_report engine::streaming_lookup_host(char const* bases, uint64_t const* read_offsets, uint64_t n_reads,
                                               result_view const& h_out) const {
    if (n_reads == 0) return {};
    if (!h_out.kmer_id) throw error(error_kind::argument, "kmer_id output pointer is null");
    const int device = resident_devices(*this)[0];
    device_guard guard(device);
    device_buffers own;
    const own_stream call(replica(device));  // (drained and its lookup scratch handed back before `own` frees the buffers)
    hipStream_t s = call.s;
    const piece_cuts pieces = cut_pieces(read_offsets, n_reads, uint64_t(64) << 20, ~uint64_t(0));
    char* d_bases = own.alloc<char>(pieces.max_bases + 8);
    uint64_t* d_offsets = own.alloc<uint64_t>(pieces.max_reads + 1);
    uint64_t* d_report = own.alloc<uint64_t>(6);
    HIP_CHECK(hipMemsetAsync(d_report, 0, 48, s));
    if (h_out.minimizer_found) throw error(error_kind::argument, "the streaming lookup does not report minimizer_found");
    result_view d_out{};
    for_each_field([&](int, auto* h, auto*& d, uint64_t) {
        if (h) d = own.alloc<std::remove_reference_t<decltype(*d)>>(pieces.max_bases);
    }, h_out, d_out);
    std::vector<uint64_t> rel(pieces.max_reads + 1);
    for (size_t piece = 0; piece < pieces.count(); ++piece) {
        const uint64_t first = pieces.cuts[piece], last = pieces.cuts[piece + 1];
        const uint64_t b0 = read_offsets[first], nb = read_offsets[last] - b0;
        if (nb == 0) continue;
        for (uint64_t i = first; i <= last; ++i) rel[i - first] = read_offsets[i] - b0;
        HIP_CHECK(hipMemcpyAsync(d_offsets, rel.data(), (last - first + 1) * 8, hipMemcpyHostToDevice, s));
        HIP_CHECK(hipMemcpyAsync(d_bases, bases + b0, nb, hipMemcpyHostToDevice, s));
        /* places without a k-mer keep what the caller's arrays hold (sshash_amd.h: "left untouched"): EVERY requested
           device array is seeded with the caller's (only kmer_id was, the others came back as stale device memory) */
        for_each_field([&](int, auto* h, auto* d, uint64_t width) {
            if (h) HIP_CHECK(hipMemcpyAsync(d, h + b0, nb * width, hipMemcpyHostToDevice, s));
        }, h_out, d_out);
        streaming_lookup_device(device, d_bases, d_offsets, last - first, nb, d_out, d_report, s);
        for_each_field([&](int, auto* h, auto* d, uint64_t width) {
            if (h) HIP_CHECK(hipMemcpyAsync(h + b0, d, nb * width, hipMemcpyDeviceToHost, s));
        }, h_out, d_out);
        HIP_CHECK(hipStreamSynchronize(s));
    }
    return read_back(d_report, s);
}

namespace {

/* Host buffers: the reads are cut into pieces of at most ~32 MiB of bases; per replica up to eight lanes (the
   pooled pinned pipelines of the lookup host path, replica.hpp) pull pieces from a shared counter and run
   copy-in -> H2D -> kernel, accumulating the six counters in device memory; one read-back per lane. */
piece_cuts cut_lane_pieces(uint64_t const* read_offsets, uint64_t n_reads, uint64_t reads_cap = ~uint64_t(0) /* the call's own cap on a piece's reads */) {
    return cut_pieces(read_offsets, n_reads, uint64_t(32) << 20,
                      std::min(reads_cap, test_hook_u64("stream_piece_reads", uint64_t(1) << 20, 1, uint64_t(1) << 20)));  // (tests: seams between pieces inside a small batch)
}

/* One lane walks one read: a read of megabases (a contig, a multiline FASTA record) would keep a single lane busy for minutes. Where the
   reads are not cut into segments (SSHASH_SEGMENTS_OFF, a minimizer shard, the best run) a piece that holds such a read goes through
   the position-parallel pipeline, which gives the same results. */
bool holds_long_read(uint64_t const* offsets, uint64_t n_reads) {
    constexpr uint64_t LONG_READ_BASES = uint64_t(1) << 16;
    for (uint64_t i = 0; i < n_reads; ++i)
        if (offsets[i + 1] - offsets[i] > LONG_READ_BASES) return true;
    return false;
}

/* With segments of S k-mers: a piece that holds a read of more than S k-mers takes the run kernel over segments (returns S), a piece of
   short reads exactly the launches it took before there were segments (returns 0). */
uint64_t piece_segments(uint64_t const* offsets, uint64_t n_reads, uint32_t k, uint64_t S) {
    if (S == 0) return 0;
    for (uint64_t i = 0; i < n_reads; ++i)
        if (read_kmers(offsets[i + 1] - offsets[i], k) > S) return S;
    return 0;
}

/* Does a piece take the per-k-mer pipeline, and not the run kernel? One that holds a long read which is not cut into segments; and, of a
   call that COUNTS per k-mer (`counts`: depth, sums, classes), every piece of a minimizer shard -- only that pipeline asks of every k-mer
   whether the shard owns it (streaming_depth_device). */
bool takes_per_kmer_pipeline(engine const& eng, bool long_read, uint64_t segments, bool counts) {
    return (long_read && !segments) || (counts && eng.index().num_shards > 1);
}

/* the six counters of one staged piece, added to d_report */
void piece_totals(engine const& eng, int device, bool long_read, uint64_t segments, char const* d_bases, uint64_t const* d_offsets, uint64_t n_reads,
                  uint64_t n_bases, uint64_t* d_report, hipStream_t s) {
    if (takes_per_kmer_pipeline(eng, long_read, segments, false)) eng.streaming_lookup_device(device, d_bases, d_offsets, n_reads, n_bases, result_view{}, d_report, s);
    else eng.streaming_query_device(device, d_bases, d_offsets, n_reads, n_bases, d_report, s, segments);
}

/* a piece as a lane hands it to the call's own work: uploaded, nothing launched yet */
struct staged_piece {
    uint64_t index, first, n, nb;  // which piece; its first read, its reads, its bases
    bool long_read;
    uint64_t segments;  // S: the piece holds a read of more than S k-mers and the call cuts such reads into segments; 0 otherwise
    int device;
    hipStream_t s;
    char const* d_bases;
    uint64_t const* d_offsets;  // n + 1, relative to the piece's first base
    uint64_t* d_report;         // the lane's six counters
    char *h_extra, *d_extra;    // the call's own `extra_bytes` of the lane's pinned and device block
};

/* The lanes of a host call over its pieces. A lane's block: the piece's offsets, its bases, the six counters, `extra_bytes` for the
   caller, each 256-byte aligned. `body` launches what the call wants of the piece on p.s and synchronizes before it returns: the
   pinned block is reused by the next piece. Returns the lanes' counters, summed. */
template <class Body>  // void(staged_piece const&)
streaming_report run_piece_lanes(engine const& eng, char const* bases, uint64_t const* read_offsets, piece_cuts const& pieces, uint64_t extra_bytes,
                                 Body const& body) {
    const std::vector<int> devs = resident_devices(eng);
    const uint64_t G = devs.size(), num_pieces = pieces.count();
    const uint64_t bases_at = ((pieces.max_reads + 1) * sizeof(uint64_t) + 255) & ~uint64_t(255);
    const uint64_t report_at = (bases_at + pieces.max_bases + 255) & ~uint64_t(255);
    const uint64_t extra_at = (report_at + 6 * sizeof(uint64_t) + 255) & ~uint64_t(255);
    const uint64_t lane_bytes = extra_bytes ? extra_at + extra_bytes : report_at + 6 * sizeof(uint64_t);

    std::atomic<uint64_t> next{0};
    const uint64_t host_S = eng.host_segments();
    const uint64_t hw = std::max(1u, std::thread::hardware_concurrency());
    const uint64_t lanes_per_device = std::min<uint64_t>({(num_pieces + G - 1) / G, 8, std::max<uint64_t>(1, hw / G)});
    std::vector<int> lane_devs(lanes_per_device * G);
    for (uint64_t li = 0; li < lane_devs.size(); ++li) lane_devs[li] = devs[li % G];
    std::vector<streaming_report> partial(lane_devs.size());
    run_lanes(eng, lane_devs, lane_bytes, [&](size_t li, int device, host_lane& lane) {
        char* hp = static_cast<char*>(lane.pinned);
        char* dp = static_cast<char*>(lane.device);
        staged_piece p{};
        p.device = device;
        p.s = lane.stream;
        p.d_bases = dp + bases_at;
        p.d_offsets = reinterpret_cast<uint64_t const*>(dp);
        p.d_report = reinterpret_cast<uint64_t*>(dp + report_at);
        p.h_extra = hp + extra_at;
        p.d_extra = dp + extra_at;
        HIP_CHECK(hipMemsetAsync(p.d_report, 0, 6 * sizeof(uint64_t), p.s));
        for (;;) {
            p.index = next.fetch_add(1);
            if (p.index >= num_pieces) break;
            p.first = pieces.cuts[p.index];
            p.n = pieces.cuts[p.index + 1] - p.first;
            uint64_t const* offsets = read_offsets + p.first;
            p.nb = offsets[p.n] - offsets[0];
            uint64_t* rel = reinterpret_cast<uint64_t*>(hp);
            for (uint64_t i = 0; i <= p.n; ++i) rel[i] = offsets[i] - offsets[0];
            std::memcpy(hp + bases_at, bases + offsets[0], p.nb);
            HIP_CHECK(hipMemcpyAsync(dp, hp, (p.n + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, p.s));
            HIP_CHECK(hipMemcpyAsync(dp + bases_at, hp + bases_at, p.nb, hipMemcpyHostToDevice, p.s));
            p.long_read = holds_long_read(offsets, p.n);
            p.segments = piece_segments(offsets, p.n, eng.index().k, host_S);
            body(p);
        }
        partial[li] = read_back(p.d_report, p.s);
    });
    streaming_report total;
    for (auto const& part : partial) total += part;
    return total;
}

/* A piece's records, `row_bytes` a read at p.d_extra, come back through the lane's pinned block (the caller's array is pageable) to the
   piece's first read in `h_rows`. */
void piece_rows_back(staged_piece const& p, uint64_t row_bytes, void* h_rows) {
    HIP_CHECK(hipMemcpyAsync(p.h_extra, p.d_extra, p.n * row_bytes, hipMemcpyDeviceToHost, p.s));
    HIP_CHECK(hipStreamSynchronize(p.s));
    std::memcpy(static_cast<char*>(h_rows) + p.first * row_bytes, p.h_extra, p.n * row_bytes);
}

/* The calls that return one record per read (rows, sums, classes, the best run), for one piece: the records are made at p.d_extra --
   zeroed where the per-k-mer pass (`by_ids`) will add to them or, no bases, no kernel runs at all; else the run kernel (`by_runs`)
   writes every one of them -- and come back. */
template <class ByIds, class ByRuns>
void piece_rows(staged_piece const& p, bool per_kmer, uint64_t row_bytes, void* h_rows, ByIds const& by_ids, ByRuns const& by_runs) {
    if (per_kmer || p.nb == 0) HIP_CHECK(hipMemsetAsync(p.d_extra, 0, p.n * row_bytes, p.s));
    if (per_kmer) by_ids();
    else if (p.nb) by_runs();
    piece_rows_back(p, row_bytes, h_rows);
}

}  // namespace

streaming_report engine::streaming_query_host(char const* bases, uint64_t const* read_offsets, uint64_t n_reads) const {
    if (n_reads == 0) return {};
    return run_piece_lanes(*this, bases, read_offsets, cut_lane_pieces(read_offsets, n_reads), 0, [&](staged_piece const& p) {
        piece_totals(*this, p.device, p.long_read, p.segments, p.d_bases, p.d_offsets, p.n, p.nb, p.d_report, p.s);
        HIP_CHECK(hipStreamSynchronize(p.s));
    });
}

/* A lane's device block also holds a row for every read of the largest piece, and a piece's rows come back into the caller's array at
   the piece's first read. */
streaming_report engine::streaming_query_per_read_host(char const* bases, uint64_t const* read_offsets, uint64_t n_reads, uint64_t* rows) const {
    if (!rows) return streaming_query_host(bases, read_offsets, n_reads);
    if (n_reads == 0) return {};
    const piece_cuts pieces = cut_lane_pieces(read_offsets, n_reads);
    const uint64_t row_bytes = 6 * sizeof(uint64_t);
    return run_piece_lanes(*this, bases, read_offsets, pieces, pieces.max_reads * row_bytes, [&](staged_piece const& p) {
        uint64_t* d_rows = reinterpret_cast<uint64_t*>(p.d_extra);
        piece_rows(p, takes_per_kmer_pipeline(*this, p.long_read, p.segments, false), row_bytes, rows,
                   [&] {
                       per_kmer_outputs more;
                       more.rows = d_rows;
                       streaming_lookup_device(p.device, p.d_bases, p.d_offsets, p.n, p.nb, result_view{}, p.d_report, p.s, more);
                   },
                   [&] { streaming_query_per_read_device(p.device, p.d_bases, p.d_offsets, p.n, p.nb, d_rows, p.d_report, p.s, p.segments); });
    });
}

/* ---- one device array per resident replica (engine.hpp) ---- */
static void* replica_alloc(uint64_t bytes) {
    void* p = nullptr;
    HIP_CHECK(hipMalloc(&p, bytes));
    return p;
}

/* (a fill) zeroed by the time it returns: the lanes' streams do not wait for the null stream */
static void zero_now(int, void* p, uint64_t bytes) {
    HIP_CHECK(hipMemsetAsync(p, 0, bytes, nullptr));
    HIP_CHECK(hipStreamSynchronize(nullptr));
}

template <class T>
replica_arrays<T>::replica_arrays(engine const& eng, uint64_t count, char const* none_here, fill_fn const& fill)
    : m_count(count), m_devices(resident_devices(eng)), m_none_here(none_here) {
    int prev = 0;
    HIP_CHECK(hipGetDevice(&prev));
    try {
        for (int device : m_devices) {
            HIP_CHECK(hipSetDevice(device));
            const uint64_t bytes = std::max<uint64_t>(count, 1) * sizeof(T);
            m_arrays.push_back(static_cast<T*>(replica_alloc(bytes)));
            fill(device, m_arrays.back(), bytes);
        }
    } catch (...) {
        free_all(prev);
        throw;
    }
    (void)hipSetDevice(prev);
}

template <class T>
void replica_arrays<T>::free_all(int then_device) {
    for (size_t i = 0; i < m_arrays.size(); ++i) {
        (void)hipSetDevice(m_devices[i]);
        (void)hipFree(m_arrays[i]);
    }
    (void)hipSetDevice(then_device);
}

template <class T>
replica_arrays<T>::~replica_arrays() {
    int prev = 0;
    if (hipGetDevice(&prev) == hipSuccess) free_all(prev);
}

template <class T>
T* replica_arrays<T>::on(int device) const {
    for (size_t i = 0; i < m_devices.size(); ++i)
        if (m_devices[i] == device) return m_arrays[i];
    throw error(error_kind::internal, m_none_here);
}

template class replica_arrays<uint32_t>;
template class replica_arrays<uint64_t>;

/* ---- the cover bitmaps of a host call: zeroed, ORed into the caller's host bitmap at the end ---- */
cover_bitmaps::cover_bitmaps(engine const& eng) : replica_arrays(eng, (eng.index().num_kmers + 63) / 64, "no cover bitmap on this device", zero_now) {}

void cover_bitmaps::or_into(uint64_t* h_cover) const {
    const uint64_t chunk = uint64_t(1) << 21;  // 16 MiB of words at a time: the host side stays bounded
    std::vector<uint64_t> part(std::min(chunk, m_count));
    for (size_t i = 0; i < m_devices.size(); ++i) {
        device_guard guard(m_devices[i]);
        for (uint64_t at = 0; at < m_count; at += chunk) {
            const uint64_t n = std::min(chunk, m_count - at);
            HIP_CHECK(hipMemcpy(part.data(), m_arrays[i] + at, n * sizeof(uint64_t), hipMemcpyDeviceToHost));
            for (uint64_t j = 0; j < n; ++j) h_cover[at + j] |= part[j];
        }
    }
}

/* A piece's k-mers are marked in the bitmap that `cover` keeps on the lane's device: the lanes of a device share it, OR commutes. */
streaming_report engine::streaming_cover_host(char const* bases, uint64_t const* read_offsets, uint64_t n_reads, cover_bitmaps const& cover) const {
    if (n_reads == 0) return {};
    return run_piece_lanes(*this, bases, read_offsets, cut_lane_pieces(read_offsets, n_reads), 0, [&](staged_piece const& p) {
        if (takes_per_kmer_pipeline(*this, p.long_read, p.segments, false)) {
            per_kmer_outputs more;
            more.cover = cover.on(p.device);
            streaming_lookup_device(p.device, p.d_bases, p.d_offsets, p.n, p.nb, result_view{}, p.d_report, p.s, more);
        } else if (p.nb) {
            streaming_cover_device(p.device, p.d_bases, p.d_offsets, p.n, p.nb, cover.on(p.device), p.d_report, p.s, p.segments);
        }
        HIP_CHECK(hipStreamSynchronize(p.s));
    });
}

/* ---- the depth arrays of a host call: deltas, zeroed; at the end every replica finishes its own on the device and the depths are added
        into the caller's host array ---- */
depth_arrays::depth_arrays(engine const& eng) : replica_arrays(eng, eng.index().num_kmers, "no depth array on this device", zero_now), m_eng(eng) {}

void depth_arrays::add_into(uint32_t* h_depth) const {
    const uint64_t chunk = uint64_t(1) << 22;  // 16 MiB of words at a time: the host side stays bounded
    std::vector<uint32_t> part(std::min(chunk, m_count));
    for (size_t i = 0; i < m_devices.size(); ++i) {
        if (m_count == 0) break;
        device_guard guard(m_devices[i]);
        m_eng.depth_finish_device(m_devices[i], m_arrays[i], m_arrays[i], nullptr);  // in place: the deltas are gone
        HIP_CHECK(hipStreamSynchronize(nullptr));
        for (uint64_t at = 0; at < m_count; at += chunk) {
            const uint64_t n = std::min(chunk, m_count - at);
            HIP_CHECK(hipMemcpy(part.data(), m_arrays[i] + at, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
            for (uint64_t j = 0; j < n; ++j) h_depth[at + j] += part[j];
        }
    }
}

/* A piece's runs are added to the deltas that `depth` keeps on the lane's device: addition commutes as the cover's OR does. */
streaming_report engine::streaming_depth_host(char const* bases, uint64_t const* read_offsets, uint64_t n_reads, depth_arrays const& depth) const {
    if (n_reads == 0) return {};
    return run_piece_lanes(*this, bases, read_offsets, cut_lane_pieces(read_offsets, n_reads), 0, [&](staged_piece const& p) {
        if (takes_per_kmer_pipeline(*this, p.long_read, p.segments, true)) {
            per_kmer_outputs more;
            more.deltas = depth.on(p.device);
            streaming_lookup_device(p.device, p.d_bases, p.d_offsets, p.n, p.nb, result_view{}, p.d_report, p.s, more);
        } else if (p.nb) {
            streaming_depth_device(p.device, p.d_bases, p.d_offsets, p.n, p.nb, depth.on(p.device), p.d_report, p.s, p.segments);
        }
        HIP_CHECK(hipStreamSynchronize(p.s));
    });
}

/* ---- the prefix sums of a host call's values: uploaded to every resident replica and built there; the 4-byte copy goes, the 8 bytes per
        k-mer stay ---- */
value_prefixes::value_prefixes(engine const& eng, uint32_t const* h_values, uint32_t at_least)
    : replica_arrays(eng, eng.index().num_kmers + 1, "no value prefix on this device", [&](int device, uint64_t* prefix, uint64_t) {
          const uint64_t n = eng.index().num_kmers;
          const std::unique_ptr<void, void (*)(void*)> values(replica_alloc(std::max<uint64_t>(n, 1) * sizeof(uint32_t)), [](void* p) { (void)hipFree(p); });
          HIP_CHECK(hipMemcpy(values.get(), h_values, n * sizeof(uint32_t), hipMemcpyHostToDevice));
          eng.value_prefix_device(device, static_cast<uint32_t const*>(values.get()), at_least, prefix, nullptr);
          HIP_CHECK(hipStreamSynchronize(nullptr));  // (the lanes' streams do not wait for the null stream)
      }) {}

/* A lane's device block holds two words for every read of the largest piece, out of the prefix sums that `prefix` keeps on its device;
   they come back as the rows do. */
streaming_report engine::streaming_sums_host(char const* bases, uint64_t const* read_offsets, uint64_t n_reads, value_prefixes const& prefix,
                                             uint64_t* sums) const {
    if (n_reads == 0) return {};
    const piece_cuts pieces = cut_lane_pieces(read_offsets, n_reads);
    const uint64_t row_bytes = 2 * sizeof(uint64_t);
    return run_piece_lanes(*this, bases, read_offsets, pieces, pieces.max_reads * row_bytes, [&](staged_piece const& p) {
        uint64_t* d_sums = reinterpret_cast<uint64_t*>(p.d_extra);
        piece_rows(p, takes_per_kmer_pipeline(*this, p.long_read, p.segments, true), row_bytes, sums,
                   [&] {
                       per_kmer_outputs more;
                       more.prefix = prefix.on(p.device);
                       more.sums = d_sums;
                       streaming_lookup_device(p.device, p.d_bases, p.d_offsets, p.n, p.nb, result_view{}, p.d_report, p.s, more);
                   },
                   [&] { streaming_sums_device(p.device, p.d_bases, p.d_offsets, p.n, p.nb, prefix.on(p.device), d_sums, p.d_report, p.s, p.segments); });
    });
}

/* ---- the labels of a host call: one copy on every resident replica ---- */
class_labels_on_devices::class_labels_on_devices(engine const& eng, uint32_t const* h_labels)
    : replica_arrays(eng, eng.index().num_strings, "no labels on this device", [&](int, uint32_t* labels, uint64_t) {
          HIP_CHECK(hipMemcpy(labels, h_labels, eng.index().num_strings * sizeof(uint32_t), hipMemcpyHostToDevice));  // (synchronous: the lanes' streams find it there)
      }) {}

/* The rows travel as the sums' do, through `num_classes` words a read of the lane's blocks; a piece holds no more reads than make
   CLASS_PIECE_BYTES of rows (beside cut_lane_pieces' bytes of bases and its hook: 4096 reads at the cap of 4096 classes). */
streaming_report engine::streaming_classes_host(char const* bases, uint64_t const* read_offsets, uint64_t n_reads, class_labels_on_devices const& labels,
                                                uint32_t num_classes, uint32_t* rows) const {
    if (n_reads == 0) return {};
    if (num_classes == 0 || num_classes > MAX_CLASSES) throw error(error_kind::argument, "num_classes must be 1 .. 4096");
    constexpr uint64_t CLASS_PIECE_BYTES = uint64_t(64) << 20;
    const uint64_t row_bytes = num_classes * sizeof(uint32_t);
    const piece_cuts pieces = cut_lane_pieces(read_offsets, n_reads, CLASS_PIECE_BYTES / row_bytes);
    return run_piece_lanes(*this, bases, read_offsets, pieces, pieces.max_reads * row_bytes, [&](staged_piece const& p) {
        uint32_t* d_rows = reinterpret_cast<uint32_t*>(p.d_extra);
        piece_rows(p, takes_per_kmer_pipeline(*this, p.long_read, p.segments, true), row_bytes, rows,
                   [&] {
                       per_kmer_outputs more;
                       more.labels = labels.on(p.device);
                       more.num_classes = num_classes;
                       more.class_rows = d_rows;
                       streaming_lookup_device(p.device, p.d_bases, p.d_offsets, p.n, p.nb, result_view{}, p.d_report, p.s, more);
                   },
                   [&] { streaming_classes_device(p.device, p.d_bases, p.d_offsets, p.n, p.nb, labels.on(p.device), num_classes, d_rows, p.d_report, p.s, p.segments); });
    });
}

/* the per-k-mer pipeline with the reads' runs for its one output: what the run records and the best run take for a piece with a long read */
static void piece_runs_by_ids(engine const& eng, staged_piece const& p, run_sink const& sink, uint64_t* d_report) {
    per_kmer_outputs more;
    more.runs = &sink;
    eng.streaming_lookup_device(p.device, p.d_bases, p.d_offsets, p.n, p.nb, result_view{}, d_report, p.s, more);
}

/* The runs of every read, host buffers (sshash_streaming_runs): pieces and lanes as above (run_piece_lanes). A piece's
   run_offsets are local to the piece and its record count is known only after its counting pass, so a lane counts, reads the count
   back, sizes the piece's device records from it and writes them; the pieces' records wait on the host until every piece's count is
   known -- only then is a piece's place in the caller's array --, and are stitched in piece order (runs_host_stitch).
   A piece that holds a read of more than S k-mers (p.segments) takes both passes over segments; the writing pass makes the table, the
   counts and E again (launch_streaming_runs): the scratch they lie in is the stream's, not the call's. With the segments off, a piece
   that holds a read above 2^16 bases takes the per-k-mer pipeline as it always did. */
namespace {
struct host_runs {
    streaming_report report;
    piece_cuts pieces;
    std::vector<std::vector<uint64_t>> piece_records;  // (four words a record)
    std::vector<uint64_t> piece_total;
};

/* run_offsets: n_reads + 1 words, on return [r] for r >= 1 local to r's piece */
host_runs runs_host_pieces(engine const& eng, char const* bases, uint64_t const* read_offsets, uint64_t n_reads, uint64_t* run_offsets, bool want_records) {
    constexpr uint64_t RECORD_BYTES = 32;
    for (uint64_t r = 0; r < n_reads; ++r)
        if ((read_offsets[r + 1] - read_offsets[r]) >> 31) throw error(error_kind::argument, "a read of 2^31 bases or more: a run record could not hold its positions");
    host_runs out;
    out.pieces = cut_lane_pieces(read_offsets, n_reads);
    const uint64_t num_pieces = out.pieces.count();
    out.piece_records.resize(num_pieces);
    out.piece_total.assign(num_pieces, 0);
    out.report = run_piece_lanes(eng, bases, read_offsets, out.pieces, (out.pieces.max_reads + 1) * sizeof(uint64_t), [&](staged_piece const& p) {
        uint64_t* d_counts = reinterpret_cast<uint64_t*>(p.d_extra);
        uint64_t const* counts = reinterpret_cast<uint64_t const*>(p.h_extra);
        const bool by_ids = p.long_read && !p.segments;  // (a long read that is not cut into segments: the per-k-mer pipeline)
        if (p.nb == 0) HIP_CHECK(hipMemsetAsync(d_counts, 0, (p.n + 1) * sizeof(uint64_t), p.s));
        else if (by_ids) piece_runs_by_ids(eng, p, run_sink{d_counts, nullptr, 0}, p.d_report);
        else eng.streaming_runs_device(p.device, p.d_bases, p.d_offsets, p.n, p.nb, d_counts, nullptr, 0, p.d_report, p.s, p.segments);
        HIP_CHECK(hipMemcpyAsync(p.h_extra, d_counts, (p.n + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, p.s));
        HIP_CHECK(hipStreamSynchronize(p.s));
        const uint64_t total = counts[p.n];
        out.piece_total[p.index] = total;
        for (uint64_t i = 1; i <= p.n; ++i) run_offsets[p.first + i] = counts[i];  // (local to the piece until the pieces are stitched)
        if (want_records && total) {
            std::vector<uint64_t>& mine = out.piece_records[p.index];
            mine.resize(total * (RECORD_BYTES / 8));
            device_buffers records(eng.replica(p.device), p.s);
            void* d_records = records.alloc<uint64_t>(total * (RECORD_BYTES / 8));
            const run_sink writing{d_counts, d_records, total};
            if (by_ids) piece_runs_by_ids(eng, p, writing, nullptr);
            else streaming_runs_write(eng, p.device, p.d_bases, p.d_offsets, p.n, p.nb, writing, p.s, p.segments);
            HIP_CHECK(hipMemcpyAsync(mine.data(), d_records, total * RECORD_BYTES, hipMemcpyDeviceToHost, p.s));
            HIP_CHECK(hipStreamSynchronize(p.s));
        }
    });
    return out;
}

/* the pieces' offsets made global and their records put behind one another, clipped at `runs_capacity` */
void runs_host_stitch(host_runs const& got, uint64_t* run_offsets, void* runs, uint64_t runs_capacity) {
    constexpr uint64_t RECORD_BYTES = 32;
    run_offsets[0] = 0;
    uint64_t base = 0;
    for (uint64_t piece = 0; piece < got.pieces.count(); ++piece) {
        for (uint64_t r = got.pieces.cuts[piece] + 1; r <= got.pieces.cuts[piece + 1]; ++r) run_offsets[r] += base;
        if (base < runs_capacity && got.piece_total[piece])
            std::memcpy(static_cast<char*>(runs) + base * RECORD_BYTES, got.piece_records[piece].data(), std::min(got.piece_total[piece], runs_capacity - base) * RECORD_BYTES);
        base += got.piece_total[piece];
    }
}
}  // namespace

streaming_report engine::streaming_runs_host(char const* bases, uint64_t const* read_offsets, uint64_t n_reads, uint64_t* run_offsets,
                                             void* runs, uint64_t runs_capacity) const {
    if (n_reads == 0) {
        if (run_offsets) run_offsets[0] = 0;
        return {};
    }
    const host_runs got = runs_host_pieces(*this, bases, read_offsets, n_reads, run_offsets, runs_capacity != 0);
    runs_host_stitch(got, run_offsets, runs, runs_capacity);
    return got.report;
}

streaming_report engine::streaming_runs_host(char const* bases, uint64_t const* read_offsets, uint64_t n_reads, std::vector<uint64_t>& run_offsets,
                                             std::vector<uint64_t>& records) const {
    run_offsets.assign(n_reads + 1, 0);
    records.clear();
    if (n_reads == 0) return {};
    const host_runs got = runs_host_pieces(*this, bases, read_offsets, n_reads, run_offsets.data(), true);
    uint64_t total = 0;
    for (uint64_t t : got.piece_total) total += t;
    records.resize(total * 4);
    runs_host_stitch(got, run_offsets.data(), records.data(), total);
    return got.report;
}

/* what every route of the best run asks of the dictionary before it looks at a read: a resident replica, and no minimizer shard */
void engine::best_run_ready() const {
    (void)resident_devices(*this);  // (throws no_device)
    best_run_refuse_shard(*m_idx);
}

/* Per read, its longest run, host buffers (sshash_streaming_best_run): pieces and lanes as above (run_piece_lanes), a record per read of
   the largest piece in the lane's blocks, never over segments. A piece that holds a read above 2^16 bases takes the route
   streaming_runs_host takes for it -- the position-parallel pipeline with a counting sink, then a writing one: the piece's CSR records
   -- and the finish of those (runs_best_device) on the same stream. */
streaming_report engine::streaming_best_run_host(char const* bases, uint64_t const* read_offsets, uint64_t n_reads, void* best) const {
    constexpr uint64_t RECORD_BYTES = 32;
    if (n_reads == 0) return {};
    best_run_ready();
    for (uint64_t r = 0; r < n_reads; ++r)
        if ((read_offsets[r + 1] - read_offsets[r]) >> 31) throw error(error_kind::argument, "a read of 2^31 bases or more: a run record could not hold its positions");
    const piece_cuts pieces = cut_lane_pieces(read_offsets, n_reads);
    return run_piece_lanes(*this, bases, read_offsets, pieces, pieces.max_reads * RECORD_BYTES, [&](staged_piece const& p) {
        void* d_best = p.d_extra;
        if (!p.long_read) {
            piece_rows(p, false, RECORD_BYTES, best, [] {}, [&] { streaming_best_run_device(p.device, p.d_bases, p.d_offsets, p.n, p.nb, d_best, p.d_report, p.s); });
            return;
        }
        device_buffers tmp(replica(p.device), p.s);  // (stream-ordered; freed behind the piece's last launch)
        uint64_t* d_counts = tmp.alloc<uint64_t>(p.n + 1);
        piece_runs_by_ids(*this, p, run_sink{d_counts, nullptr, 0}, p.d_report);
        uint64_t* const h_total = reinterpret_cast<uint64_t*>(p.h_extra);  // (the pinned block's first word, until the records come back into it)
        HIP_CHECK(hipMemcpyAsync(h_total, d_counts + p.n, sizeof(uint64_t), hipMemcpyDeviceToHost, p.s));
        HIP_CHECK(hipStreamSynchronize(p.s));
        const uint64_t total = *h_total;
        void* d_records = tmp.alloc<uint64_t>(std::max<uint64_t>(total, 1) * (RECORD_BYTES / 8));
        if (total) piece_runs_by_ids(*this, p, run_sink{d_counts, d_records, total}, nullptr);
        runs_best_device(p.device, d_counts, d_records, p.n, d_best, p.s);
        piece_rows_back(p, RECORD_BYTES, best);
    });
}

/* The file query of an uncompressed FASTQ (engine.hpp). One reader thread feeding batches through streaming_query_host splits
   9 GB/s of file and the devices wait for it nine tenths of the time (HISTORY.md); here parsing is the lanes' own
   work: lane = host thread + stream + pinned block + device block, as many lanes as usable CPUs, dealt round-robin to the
   resident replicas. */
bool engine::streaming_query_fastq_pieces(std::string const& filename, streaming_report& total) const {
    const std::vector<int> devs = resident_devices(*this);
    const uint64_t G = devs.size();
    uint64_t want_lanes = std::max<uint64_t>(G, std::min<uint64_t>(32, usable_cpus()));
    if (char const* e = std::getenv("SSHASH_AMD_READER_THREADS")) want_lanes = std::max<uint64_t>(1, std::strtoull(e, nullptr, 10));
    /* pieces of 32 MiB of file; a smaller file is cut finer, so that every lane still gets several (4 MiB at least) */
    uint64_t piece_bytes = uint64_t(32) << 20;
    {
        struct stat st;
        if (stat(filename.c_str(), &st) == 0)
            piece_bytes = std::min<uint64_t>(piece_bytes, std::max<uint64_t>(uint64_t(4) << 20, uint64_t(st.st_size) / (want_lanes * 8)));
    }
    piece_bytes = test_hook_u64("fastq_piece_bytes", piece_bytes, 4096, ~uint64_t(0));  // (tests: many pieces of a small file)
    const fastq_pieces file(filename, piece_bytes);
    const uint64_t num_pieces = file.num_pieces();
    if (num_pieces == 0) return true;  // an empty file: an empty report
    const uint32_t k = m_idx->k;
    const uint64_t off_capacity = file.offsets_capacity(k), bases_capacity = file.bases_capacity();
    const uint64_t bases_at = (off_capacity * sizeof(uint64_t) + 255) & ~uint64_t(255);
    const uint64_t report_at = (bases_at + bases_capacity + 255) & ~uint64_t(255);
    const uint64_t lane_bytes = report_at + 6 * sizeof(uint64_t);
    std::vector<int> lane_devs(std::min(num_pieces, want_lanes));
    for (uint64_t li = 0; li < lane_devs.size(); ++li) lane_devs[li] = devs[li % G];

    std::atomic<uint64_t> next{0};
    const uint64_t host_S = host_segments();
    std::atomic<bool> give_up{false};  // a lane threw, or a piece did not fit: the others take no more pieces
    std::vector<fastq_pieces::parsed> seen(num_pieces);
    std::vector<streaming_report> partial(lane_devs.size());
    run_lanes(*this, lane_devs, lane_bytes, [&](size_t li, int device, host_lane& lane) {
        hipStream_t s = lane.stream;
        char* hp = static_cast<char*>(lane.pinned);
        char* dp = static_cast<char*>(lane.device);
        uint64_t* d_report = reinterpret_cast<uint64_t*>(dp + report_at);
        HIP_CHECK(hipMemsetAsync(d_report, 0, 6 * sizeof(uint64_t), s));
        std::vector<char> raw;
        for (;;) {
            const uint64_t piece = next.fetch_add(1);
            if (piece >= num_pieces || give_up) break;
            uint64_t* offsets = reinterpret_cast<uint64_t*>(hp);
            const fastq_pieces::parsed got = file.parse(piece, k, hp + bases_at, bases_capacity, offsets, off_capacity, raw);
            seen[piece] = got;
            if (got.overflow) {
                give_up = true;
                break;
            }
            if (got.num_reads == 0) continue;
            HIP_CHECK(hipMemcpyAsync(dp, hp, (got.num_reads + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, s));
            HIP_CHECK(hipMemcpyAsync(dp + bases_at, hp + bases_at, got.num_bases, hipMemcpyHostToDevice, s));
            piece_totals(*this, device, holds_long_read(offsets, got.num_reads), piece_segments(offsets, got.num_reads, k, host_S), dp + bases_at, reinterpret_cast<uint64_t const*>(dp), got.num_reads, got.num_bases, d_report, s);
            HIP_CHECK(hipStreamSynchronize(s));  // the pinned block is parsed into again
        }
        partial[li] = read_back(d_report, s);
    }, &give_up);
    if (give_up) return false;
    /* every piece began where its predecessor stopped, the first at 0, the last stopped at the end of the file: the pieces
       together are the sequential reader's records (reads.hpp) */
    uint64_t expect = 0;
    for (uint64_t i = 0; i < num_pieces; ++i) {
        if (seen[i].first_record != expect) return false;
        expect = seen[i].next_record;
    }
    if (expect != file.file_bytes()) return false;
    for (auto const& p : partial) total += p;
    return true;
}

}  // namespace sshash_amd
