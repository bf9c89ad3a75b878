// check_segment_runs.cpp -- the run RECORDS over segments as a host model (sshash_amd/csrc/streaming.hip, "the run RECORDS over
// segments"; the arithmetic and the scratch layout are those of sshash_amd/csrc/segments.hpp): synthetic reads given as one (string, id,
// orientation) per k-mer -- or negative, or invalid -- are cut at S in {1, 2, 7, 64}; per segment the runs are counted as the run kernel
// counts them (a segment's first positive k-mer starts a run), joined[g] is what the seam kernel finds, c' = c - joined, E its exclusive
// scan, the record form stores every run that starts in its segment at E[g] and on and hands a joined first run's length to cont[g], and
// the merge adds cont[g] to the length word of record E[g] - 1. What comes out must be, byte for byte, the runs of the uncut reads, at
// every capacity, with nothing written at or behind the capacity. No GPU call, no library: built with -fsanitize=address,undefined.
//   [A] crafted reads per S: a run across at least three whole segments, a run that ends on a seam's last k-mer (the next k-mer negative,
//       and the next k-mer positive elsewhere), a run that starts on a seam's first k-mer, a backward run across a seam, seams on negative
//       and invalid k-mers, reads without a k-mer, a long read last (empty table entries behind the true count);
//   [B] random reads;
//   [C] every capacity from 0 to the total + 3 -- below, at and above E[g] - 1 of every joined seam;
//   [D] segment_runs_scratch: the parts follow each other, and a saturated bound gives 0 words instead of a wrapped size.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "../../sshash_amd/csrc/segments.hpp"

using namespace sshash_amd;

static int failures = 0;
#define CHECK(cond)                                                      \
    do {                                                                 \
        if (!(cond)) {                                                   \
            std::printf("line %d: %s does not hold\n", __LINE__, #cond); \
            ++failures;                                                  \
        }                                                                \
    } while (0)

constexpr uint32_t K = 5;  // the model's k: a read of n k-mers has n + K - 1 bases
constexpr uint32_t BACKWARD = 0x80000000u;

struct kmer {
    int state;  // 0 negative, 1 positive, 2 invalid
    uint64_t string, id;
    int ori;
};
using read_t = std::vector<kmer>;

struct record {  // (sshash_streaming_run: 32 bytes, the length in word RUN_RECORD_LENGTH_WORD)
    uint64_t kmer_id, string_id, kmer_id_in_string;
    uint32_t read_pos, num_kmers;
};
static_assert(sizeof(record) == 32, "a run record is 32 bytes");

static bool continues(kmer const& a, kmer const& b) {  // (the header's rule)
    return a.state == 1 && b.state == 1 && a.string == b.string && b.id == a.id + uint64_t(int64_t(a.ori));
}

/* the runs of the k-mers [from, to) of `r`, each a search and its extensions; `base`: what read_pos is counted from */
static void runs_of(read_t const& r, uint64_t from, uint64_t to, std::vector<record>& out) {
    for (uint64_t j = from; j < to;) {
        if (r[j].state != 1) {
            ++j;
            continue;
        }
        uint64_t n = 1;
        while (j + n < to && continues(r[j + n - 1], r[j + n])) ++n;
        out.push_back(record{r[j].id, r[j].string, r[j].id % 1000, uint32_t(j), uint32_t(n) | (r[j].ori > 0 ? 0u : BACKWARD)});
        j += n;
    }
}

static void add_run(read_t& r, uint64_t string, uint64_t id, int ori, uint64_t n) {
    for (uint64_t j = 0; j < n; ++j) r.push_back(kmer{1, string, id + uint64_t(int64_t(ori) * int64_t(j)), ori});
}
static void add_other(read_t& r, int state, uint64_t n) {
    for (uint64_t j = 0; j < n; ++j) r.push_back(kmer{state, 0, 0, 1});
}

struct coverage {
    uint64_t chains3 = 0, ends_on_seam = 0, starts_on_seam = 0, backward_joined = 0, forward_joined = 0, seam_negative = 0, seam_invalid = 0, capacity_below = 0,
             capacity_at = 0, capacity_above = 0;
};

static void check_batch(std::vector<read_t> const& reads, uint64_t S, coverage& seen) {
    const uint64_t n_reads = reads.size();
    /* the uncut truth */
    std::vector<uint64_t> want_offsets(n_reads + 1, 0);
    std::vector<record> want;
    uint64_t total_bases = 0;
    for (uint64_t r = 0; r < n_reads; ++r) {
        runs_of(reads[r], 0, reads[r].size(), want);
        want_offsets[r + 1] = want.size();
        total_bases += reads[r].empty() ? (r % 2 ? K - 1 : 0) : reads[r].size() + K - 1;  // (a read without a k-mer: empty, or shorter than k)
    }
    /* the table: first[], and per entry its read and its k-mers [begin, end) */
    const uint64_t bound = segment_bound(n_reads, total_bases, S);
    std::vector<uint64_t> first(n_reads + 1, 0);
    for (uint64_t r = 0; r < n_reads; ++r) first[r + 1] = first[r] + segments_of_read(reads[r].size(), S);
    const uint64_t n_segments = first[n_reads];
    CHECK(n_segments <= bound);
    std::vector<uint64_t> seg_read(bound, ~uint64_t(0)), seg_from(bound, 0), seg_to(bound, 0);
    for (uint64_t r = 0; r < n_reads; ++r)
        for (uint64_t g = first[r]; g < first[r + 1]; ++g) {
            seg_read[g] = r;
            seg_from[g] = (g - first[r]) * S;
            seg_to[g] = std::min<uint64_t>(seg_from[g] + S, reads[r].size());
        }
    /* the scratch, laid out as the launch lays it out */
    const segment_runs_layout R = segment_runs_scratch(bound, 4096);
    CHECK(R.words != 0);
    std::vector<uint64_t> scratch(R.words, 0xDDDDDDDDDDDDDDDDull);
    uint64_t* const E = scratch.data() + R.counts;
    uint32_t* const cont = reinterpret_cast<uint32_t*>(scratch.data() + R.cont);
    uint8_t* const joined = reinterpret_cast<uint8_t*>(scratch.data() + R.joined);
    CHECK(reinterpret_cast<uint32_t*>(E + bound + 1) == cont);  // (where the run kernel looks for them: behind E)
    CHECK(reinterpret_cast<uint8_t*>(E + bound + 1 + segment_runs_cont_words(bound)) == joined);
    /* count, seams */
    std::vector<std::vector<record>> seg_runs(bound);
    for (uint64_t g = 0; g < bound; ++g) {
        if (g < n_segments) runs_of(reads[seg_read[g]], seg_from[g], seg_to[g], seg_runs[g]);
        E[g] = seg_runs[g].size();
        bool join = false;
        if (g > 0 && g < n_segments && seg_read[g] == seg_read[g - 1]) {
            read_t const& r = reads[seg_read[g]];
            const uint64_t p = seg_from[g];
            join = continues(r[p - 1], r[p]);
            if (join) ++(r[p].ori > 0 ? seen.forward_joined : seen.backward_joined);
            else if (r[p - 1].state == 1 && r[p].state != 1) ++seen.ends_on_seam;  // a run ends on the seam's last k-mer
            else if (r[p - 1].state == 1 && r[p].state == 1) ++seen.ends_on_seam, ++seen.starts_on_seam;
            else if (r[p].state == 1) ++seen.starts_on_seam;
            if (r[p].state == 0) ++seen.seam_negative;
            if (r[p].state == 2) ++seen.seam_invalid;
        }
        joined[g] = join ? 1 : 0;
    }
    E[bound] = 0xABCDEF;  // (whatever the scratch held)
    /* starts, scan */
    uint64_t chain = 0;
    for (uint64_t g = 0; g <= bound; ++g) {
        uint64_t starts = 0;
        if (g < bound && g < n_segments) {
            CHECK(E[g] >= joined[g]);
            starts = E[g] > joined[g] ? E[g] - joined[g] : 0;
            chain = joined[g] && starts == 0 ? chain + 1 : 0;  // segments that lie wholly inside one run, in a row
            if (chain >= 3) ++seen.chains3;                    // (three whole segments in a row inside one run that began before them)
        }
        E[g] = starts;
    }
    for (uint64_t g = 0, sum = 0; g <= bound; ++g) {
        const uint64_t v = E[g];
        E[g] = sum;
        sum += v;
    }
    /* offsets */
    for (uint64_t r = 0; r <= n_reads; ++r) CHECK(E[first[r]] == want_offsets[r]);
    const uint64_t total = want.size();
    CHECK(E[bound] == total);
    /* write and merge, at every capacity */
    for (uint64_t capacity = 0; capacity <= total + 3; ++capacity) {
        std::vector<record> got(capacity + 2);
        std::memset(got.data(), 0x5A, got.size() * sizeof(record));
        for (uint64_t g = 0; g < bound; ++g) {
            uint64_t cursor = E[g];
            bool seam_open = joined[g] != 0;
            cont[g] = 0;
            for (record const& run : seg_runs[g]) {
                if (seam_open) {
                    cont[g] = run.num_kmers & ~BACKWARD;
                    seam_open = false;
                    continue;
                }
                if (cursor < capacity && cursor < E[g + 1]) got[cursor] = run;
                ++cursor;
            }
            CHECK(!seam_open && cursor == E[g + 1]);
        }
        for (uint64_t g = 0; g < bound; ++g) {
            if (g >= n_segments || !joined[g]) continue;
            CHECK(E[g] > 0);
            if (E[g] - 1 < capacity) {
                reinterpret_cast<uint32_t*>(&got[E[g] - 1])[RUN_RECORD_LENGTH_WORD] += cont[g];
                if (E[g] == capacity) ++seen.capacity_above;  // (capacity = (E[g] - 1) + 1)
            } else {
                ++(E[g] - 1 == capacity ? seen.capacity_at : seen.capacity_below);
            }
        }
        const uint64_t kept = std::min(capacity, total);
        CHECK(kept == 0 || std::memcmp(got.data(), want.data(), kept * sizeof(record)) == 0);
        for (uint64_t i = kept; i < got.size(); ++i) {
            const unsigned char* bytes = reinterpret_cast<const unsigned char*>(&got[i]);
            bool untouched = true;
            for (uint64_t b = 0; b < sizeof(record); ++b) untouched = untouched && bytes[b] == 0x5A;
            CHECK(untouched);
        }
    }
}

int main() {
    const uint64_t MAX = ~uint64_t(0);
    std::mt19937_64 rng(11);
    for (uint64_t S : {uint64_t(1), uint64_t(2), uint64_t(7), uint64_t(64)}) {
        coverage seen;
        /* [A] */
        std::vector<read_t> reads;
        {
            read_t r;  // a forward run across more than four whole segments, begun inside a segment
            add_other(r, 0, 3);
            add_run(r, 4, 100000, +1, 4 * S + 9);
            add_other(r, 0, 2);
            reads.push_back(r);
        }
        reads.push_back(read_t{});  // no k-mer (an empty read)
        {
            read_t r;  // a run that ends on a seam's last k-mer, the next k-mer negative; then a run that starts on a seam's first k-mer
            add_other(r, 0, S > 1 ? 1 : 0);
            add_run(r, 7, 500, +1, 2 * S - (S > 1 ? 1 : 0));  // ends at k-mer 2 S - 1
            add_other(r, 0, S);                               // k-mers 2 S .. 3 S - 1
            add_run(r, 8, 900, -1, S + 3);                    // starts at k-mer 3 S, backward, over the seam at 4 S
            reads.push_back(r);
        }
        {
            read_t r;  // a run that ends on a seam's last k-mer and another that starts right behind it: positive on both sides, not joined
            add_run(r, 2, 40, +1, S);
            add_run(r, 3, 77, +1, S + 1);
            add_run(r, 3, 5000, -1, 3 * S);  // the same string elsewhere, backward, over whole segments
            add_other(r, 2, S + 1);          // invalid k-mers over a seam
            add_run(r, 3, 5000 - 3 * S + 1, +1, 2);
            reads.push_back(r);
        }
        reads.push_back(read_t{});  // no k-mer (shorter than k)
        {
            read_t r;  // a backward run whose id would continue FORWARD at the seam: not joined (the id moves by the orientation of the k-mer before)
            add_run(r, 9, 300, -1, S);
            add_run(r, 9, 300 - S + 2, -1, S);
            reads.push_back(r);
        }
        {
            read_t r;  // the last read is a long one: the empty entries of the table lie behind its segments
            add_run(r, 11, 70000, -1, 3 * S + 1);
            add_other(r, 0, 1);
            add_run(r, 11, 1, +1, 5 * S);
            reads.push_back(r);
        }
        check_batch(reads, S, seen);
        CHECK(seen.chains3 > 0 && seen.ends_on_seam > 0 && seen.starts_on_seam > 0 && seen.backward_joined > 0 && seen.forward_joined > 0);
        CHECK(seen.seam_negative > 0 && seen.seam_invalid > 0);
        CHECK(seen.capacity_below > 0 && seen.capacity_at > 0 && seen.capacity_above > 0);
        /* [B] */
        for (int round = 0; round < 40; ++round) {
            std::vector<read_t> batch(1 + rng() % 6);
            for (read_t& r : batch) {
                const uint64_t parts = rng() % 7;
                for (uint64_t p = 0; p < parts; ++p) {
                    const uint64_t n = 1 + rng() % (3 * S + 2);
                    switch (rng() % 4) {
                        case 0: add_other(r, 0, n); break;
                        case 1: add_other(r, 2, n); break;
                        case 2: add_run(r, rng() % 3, 1000 + rng() % 50, +1, n); break;
                        default: add_run(r, rng() % 3, 1000 + n + rng() % 50, -1, n); break;
                    }
                }
            }
            check_batch(batch, S, seen);
        }
    }
    /* [D] */
    for (int round = 0; round < 500; ++round) {
        const uint64_t bound = rng() % (uint64_t(1) << (round % 40));
        const segment_runs_layout R = segment_runs_scratch(bound, 4096);
        CHECK(R.counts == 0 && R.cont == bound + 1 && R.joined == R.cont + (bound + 1) / 2 && R.sums == R.joined + (bound + 7) / 8);
        CHECK(R.words == R.sums + (bound + 1 + 4095) / 4096 && R.words != 0 && R.words < (uint64_t(1) << 61));
    }
    CHECK(segment_runs_cont_words(MAX) == (MAX >> 1) + 1 && segment_runs_cont_words(0) == 0 && segment_runs_cont_words(1) == 1);
    CHECK(segment_runs_scratch(MAX, 4096).words == 0);  // (segment_bound saturates there: refused, not wrapped into a small size)
    CHECK(segment_runs_scratch(segment_bound(MAX, MAX, 1), 4096).words == 0);
    CHECK(segment_runs_scratch(uint64_t(1) << 56, 4096).words == 0 && segment_runs_scratch((uint64_t(1) << 56) - 1, 4096).words != 0);
    CHECK(segment_runs_scratch(5, 0).words == 0);
    if (failures == 0) std::printf("EVERYTHING OK!\n");
    return failures ? 1 : 0;
}
