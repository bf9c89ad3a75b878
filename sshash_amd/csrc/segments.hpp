// segments.hpp -- long reads cut into SEGMENTS for the run kernel (streaming.hip): the arithmetic of the cut and the sizes of what it
// needs in scratch. Plain host code, no device call: the launch sizes everything from here without a synchronisation, and a stand-alone
// program (tests/cpp/check_segment_sizes.cpp) goes over it under the sanitizers.
//
// With S the segment length in k-mers and K = max(len - k + 1, 0) the k-mers of a read, the read becomes max(1, ceil(K / S)) segments;
// segment j holds the k-mers that start at bases [j S, min((j + 1) S, K)) of the read, so it spans the bases
// [begin + j S, min(begin + (j + 1) S + k - 1, end)): neighbours overlap by k - 1 bases of the packed copy, nothing is copied.
#pragma once

#include <cstdint>

namespace sshash_amd {

constexpr uint64_t SEGMENTS_OFF = ~uint64_t(0);            // never segment (SSHASH_SEGMENTS_OFF)
constexpr uint64_t SEGMENT_KMERS_MAX = uint64_t(1) << 30;  // the largest segment length a caller may set
/* The S that kmers_per_segment = 0 stands for (RESULTS.md, "Long reads"; a new dictionary does not segment at all). Of 256, 1024 and 4096
   it measured best through the host call, whose pieces of 32 MiB have the fewest lanes to spare -- on one reduced k = 31 dictionary,
   three repetitions. The device calls favour 1024 by 3 % on 10-kb reads and are level on reads of 2^20 bases. A seam costs a seed in the run kernel and
   two in the seam kernel, so a short S pays per base; a long S leaves a piece of 32 MiB with too few lanes for the chip. */
constexpr uint64_t SEGMENT_KMERS_DEFAULT = 256;

/* what sshash_set_read_segments accepts: 0 (the default), SEGMENTS_OFF, or 1 .. 2^30 */
inline bool segment_setting_valid(uint64_t kmers_per_segment) {
    return kmers_per_segment == SEGMENTS_OFF || kmers_per_segment <= SEGMENT_KMERS_MAX;
}

/* the k-mers of a read of `len` bases (constexpr: the kernels that build the table count with the same two functions) */
constexpr uint64_t read_kmers(uint64_t len, uint32_t k) { return len >= k ? len - k + 1 : 0; }

/* the segments of a read of `kmers` k-mers: at least one, also for a read without a k-mer */
constexpr uint64_t segments_of_read(uint64_t kmers, uint64_t S) {
    const uint64_t n = kmers / S + (kmers % S ? 1 : 0);  // (no kmers + S - 1: that sum may wrap)
    return n ? n : 1;
}

/* What the host knows without looking at the reads: n_seg <= n_reads + total_bases / S (a read has at most 1 + K / S <= 1 + len / S
   segments). The table has that many entries; those past the true count are empty segments. Saturates instead of wrapping. */
inline uint64_t segment_bound(uint64_t n_reads, uint64_t total_bases, uint64_t S) {
    const uint64_t more = total_bases / S;
    return more > ~uint64_t(0) - n_reads ? ~uint64_t(0) : n_reads + more;
}

/* Where the parts of the segment scratch lie, in 8-byte words from its first: the reads' segment counts, scanned in place into the
   index of every read's first segment (n_reads + 1 words, the last the true number of segments); the scan's tile sums; seg_begin,
   seg_end, seg_read (`bound` words each); with rows, six words a segment and the seam flags, a byte a segment. `words` is the size of
   it all; 0 when that does not fit 2^61 words (the caller refuses). */
struct segment_layout {
    uint64_t bound, first, sums, begin, end, read, rows, joined, words;
};

inline segment_layout segment_scratch(uint64_t n_reads, uint64_t total_bases, uint64_t S, uint64_t scan_tile, bool with_rows) {
    segment_layout L{};
    L.bound = segment_bound(n_reads, total_bases, S);
    const uint64_t limit = uint64_t(1) << 56;
    if (L.bound >= limit || n_reads >= limit) return L;  // (words = 0)
    uint64_t at = 0;
    L.first = at, at += n_reads + 1;
    L.sums = at, at += (n_reads + 1 + scan_tile - 1) / scan_tile;
    L.begin = at, at += L.bound;
    L.end = at, at += L.bound;
    L.read = at, at += L.bound;
    L.rows = at, at += with_rows ? 6 * L.bound : 0;
    L.joined = at, at += with_rows ? (L.bound + 7) / 8 : 0;
    L.words = at;
    return L;
}

/* What the run RECORDS over a segment table need besides it, in 8-byte words from their first, for a table of `bound` entries: the
   runs of every segment, scanned in place into E -- the final index of the first record that starts in the segment -- (`bound` + 1 words,
   the last the number of records); right behind them, where the record form of the run kernel finds them from E and the number of
   entries alone, `cont` -- 32 bits a segment: the length of its first run when that continues the run of the segment before -- and the seam
   flags, a byte a segment; the tile sums of the scan. `words` is the size of it all; 0 when that does not fit 2^61 words (the caller
   refuses): a bound that segment_bound saturated lands there, nothing wraps. */
struct segment_runs_layout {
    uint64_t counts, cont, joined, sums, words;
};

constexpr uint64_t segment_runs_cont_words(uint64_t bound) { return bound / 2 + (bound & 1); }  // (no bound + 1: that sum may wrap)

inline segment_runs_layout segment_runs_scratch(uint64_t bound, uint64_t scan_tile) {
    segment_runs_layout R{};
    if (bound >= (uint64_t(1) << 56) || scan_tile == 0) return R;  // (words = 0)
    uint64_t at = 0;
    R.counts = at, at += bound + 1;
    R.cont = at, at += segment_runs_cont_words(bound);
    R.joined = at, at += (bound + 7) / 8;
    R.sums = at, at += (bound + 1 + scan_tile - 1) / scan_tile;
    R.words = at;
    return R;
}

/* A record of 32 bytes as eight words of 32 bits: the one that holds the run's length, the strand in its bit 31 (include/sshash_amd.h:
   sshash_streaming_run.num_kmers). A run that goes on over a seam gets the rest of its length added there. */
constexpr uint32_t RUN_RECORD_LENGTH_WORD = 7;

}  // namespace sshash_amd
