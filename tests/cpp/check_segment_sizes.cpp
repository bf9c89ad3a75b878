// check_segment_sizes.cpp -- the host arithmetic of long-read segments (sshash_amd/csrc/segments.hpp) on its own: what
// sshash_set_read_segments accepts, how many segments a read becomes, the bound the launch sizes its table from, and where the parts of
// the segment scratch lie. No GPU call, no library: built with -fsanitize=address,undefined and run on the CPU (make sanitize).
//   [A] segments_of_read against the definition, and the segments' base ranges tile the read's k-mers exactly once;
//   [B] the true number of segments of random batches never exceeds segment_bound;
//   [C] the parts of the scratch follow each other without overlap and fit `words`; values at the edge of 64 bits neither wrap nor trap.
#include <cstdint>
#include <cstdio>
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

int main() {
    const uint64_t MAX = ~uint64_t(0);
    /* the setting */
    CHECK(segment_setting_valid(0) && segment_setting_valid(1) && segment_setting_valid(SEGMENT_KMERS_MAX) && segment_setting_valid(SEGMENTS_OFF));
    CHECK(!segment_setting_valid(SEGMENT_KMERS_MAX + 1) && !segment_setting_valid(MAX - 1) && !segment_setting_valid(uint64_t(1) << 63));
    CHECK(SEGMENT_KMERS_DEFAULT >= 1 && SEGMENT_KMERS_DEFAULT <= SEGMENT_KMERS_MAX);
    /* [A] */
    CHECK(read_kmers(0, 31) == 0 && read_kmers(30, 31) == 0 && read_kmers(31, 31) == 1 && read_kmers(MAX, 63) == MAX - 62);
    CHECK(segments_of_read(0, 7) == 1 && segments_of_read(7, 7) == 1 && segments_of_read(8, 7) == 2 && segments_of_read(MAX, 1) == MAX);
    CHECK(segments_of_read(MAX, SEGMENT_KMERS_MAX) == (MAX >> 30) + 1);
    std::mt19937_64 rng(5);
    for (int round = 0; round < 2000; ++round) {
        const uint32_t k = round % 2 ? 31 : 63;
        const uint64_t S = 1 + rng() % (round % 3 ? 70 : 5000), len = rng() % 9000, begin = rng() % 1000, end = begin + len;
        const uint64_t K = read_kmers(len, k), n = segments_of_read(K, S);
        CHECK(n == (K + S - 1) / S || (K == 0 && n == 1));
        uint64_t covered = 0;
        for (uint64_t j = 0; j < n; ++j) {  // (as stream_segment_fill_kernel cuts)
            const uint64_t at = begin + j * S, stop = end - at > S + k - 1 ? at + S + k - 1 : end;
            CHECK(at <= stop && stop <= end);
            const uint64_t kmers = read_kmers(stop - at, k);
            CHECK(K == 0 || (kmers >= 1 && kmers <= S));
            CHECK(j + 1 == n || kmers == S);
            covered += kmers;
        }
        CHECK(covered == K);
    }
    /* [B] */
    for (int round = 0; round < 300; ++round) {
        const uint32_t k = round % 2 ? 31 : 63;
        const uint64_t S = 1 + rng() % 300, n_reads = 1 + rng() % 200;
        uint64_t total = 0, segments = 0;
        for (uint64_t r = 0; r < n_reads; ++r) {
            const uint64_t len = rng() % 4 ? rng() % 700 : rng() % 100000;
            total += len;
            segments += segments_of_read(read_kmers(len, k), S);
        }
        CHECK(segments <= segment_bound(n_reads, total, S));
    }
    CHECK(segment_bound(MAX, MAX, 1) == MAX && segment_bound(5, MAX, 1) == MAX && segment_bound(MAX - 1, 2, 2) == MAX);
    CHECK(segment_bound(3, 100, 7) == 3 + 14 && segment_bound(0, 0, 1) == 0);
    /* [C] */
    for (int with_rows = 0; with_rows < 2; ++with_rows) {
        for (int round = 0; round < 500; ++round) {
            const uint64_t S = 1 + rng() % 5000, n_reads = 1 + rng() % 100000, total = rng() % (uint64_t(1) << 36);
            const segment_layout L = segment_scratch(n_reads, total, S, 4096, with_rows != 0);
            CHECK(L.bound == segment_bound(n_reads, total, S) && L.words != 0);
            CHECK(L.first == 0 && L.sums == n_reads + 1 && L.begin == L.sums + (n_reads + 1 + 4095) / 4096);
            CHECK(L.end == L.begin + L.bound && L.read == L.end + L.bound && L.rows == L.read + L.bound);
            CHECK(L.joined == L.rows + (with_rows ? 6 * L.bound : 0) && L.words == L.joined + (with_rows ? (L.bound + 7) / 8 : 0));
            CHECK(L.words < (uint64_t(1) << 61));
        }
        CHECK(segment_scratch(MAX, MAX, 1, 4096, with_rows != 0).words == 0);
        CHECK(segment_scratch(1, MAX, 1, 4096, with_rows != 0).words == 0);
        CHECK(segment_scratch(MAX, 0, 1024, 4096, with_rows != 0).words == 0);
        CHECK(segment_scratch((uint64_t(1) << 56) - 1, 0, 1024, 4096, with_rows != 0).words != 0);
        std::vector<uint64_t> table(segment_scratch(100, 5000, 7, 4096, with_rows != 0).words, 0);  // (the sanitizer watches the last word)
        table.back() = 1;
        CHECK(table.size() > 100);
    }
    if (failures == 0) std::printf("EVERYTHING OK!\n");
    return failures ? 1 : 0;
}
