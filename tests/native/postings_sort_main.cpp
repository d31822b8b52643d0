// postings_sort_main.cpp -- the pass plan of the postings sort (csrc/am_postings.h) run on the CPU with the header's own functions, against std::stable_sort.
// A stand-alone program: g++ -I alfred-margaret_amd/csrc, plain or with -fsanitize=address,undefined.  What the kernels of am_postings.hip do with wavefronts is done
// here with plain loops over the same arithmetic: per tile the count of every digit value into cell post_cell(d, tile), the exclusive sum over the cells in
// (digit, tile) order, the placement of every key at base[cell] + its rank among the keys of its tile with the same digit, then the next pass.  Every array is a
// std::vector sized exactly: an index beyond a table is a sanitizer report.  Also checked: the plan itself (passes, bits, shifts) and post_lower_bound.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <numeric>
#include <vector>

#include "am_postings.h"

using namespace am::dev;

namespace {

int g_failed = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (g_failed++ < 20) { std::printf("FAILED %s:%d %s: ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

uint64_t g_rng = 0x9E3779B97F4A7C15ull;
uint64_t rnd() { g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17; return g_rng; }

uint32_t bitlen(uint64_t x) { uint32_t b = 0; while (x) { b++; x >>= 1; } return b; }

void check_plan(uint64_t N)
{
    const PostPlan p = post_plan(N);
    const uint32_t B = N <= 1 ? 0 : bitlen(N - 1);
    CHECK(post_key_bits(N) == B, "N %llu", (unsigned long long)N);
    CHECK(p.passes == (B + 7) / 8 && p.passes <= kPostMaxPasses && p.passes == post_passes(N), "N %llu passes %u", (unsigned long long)N, p.passes);
    uint32_t sum = 0;
    for (uint32_t k = 0; k < p.passes; k++) {
        CHECK(p.bits[k] >= 1 && p.bits[k] <= kPostMaxDigitBits && p.shift[k] == sum, "N %llu pass %u bits %u shift %u", (unsigned long long)N, k, p.bits[k], p.shift[k]);
        if (k) CHECK(p.bits[k] <= p.bits[k - 1] && p.bits[k - 1] - p.bits[k] <= 1, "N %llu: the bits are not even", (unsigned long long)N);
        sum += p.bits[k];
    }
    CHECK(sum == B, "N %llu sum %u", (unsigned long long)N, sum);
    // the digits of a key put together again are the key
    for (int t = 0; t < 64 && N; t++) {
        const uint32_t key = (uint32_t)(t == 0 ? N - 1 : t == 1 ? 0 : rnd() % N);
        uint32_t back = 0;
        for (uint32_t k = 0; k < p.passes; k++) { const uint32_t d = post_digit(p, key, k); CHECK(d < post_digits(p, k), "digit"); back |= d << p.shift[k]; }
        CHECK(back == key, "N %llu key %u back %u", (unsigned long long)N, key, back);
    }
}

// the pass plan over (key, index) pairs, as the kernels run it
void plan_sort(uint64_t N, const std::vector<uint32_t>& keys_in, std::vector<uint32_t>& keys, std::vector<uint32_t>& idx)
{
    const uint64_t n = keys_in.size(), n_tiles = post_tiles(n);
    const PostPlan p = post_plan(N);
    keys = keys_in;
    idx.resize(n);
    std::iota(idx.begin(), idx.end(), 0u);
    std::vector<uint32_t> keys2(n), idx2(n);
    for (uint32_t pass = 0; pass < p.passes; pass++) {
        const uint32_t digits = post_digits(p, pass);
        std::vector<uint32_t> counts((size_t)digits * n_tiles, 0);
        for (uint64_t i = 0; i < n; i++) counts[post_cell(post_digit(p, keys[i], pass), i / kPostTileSpans, n_tiles)]++;
        std::vector<uint64_t> base(counts.size());
        uint64_t run = 0;
        for (size_t c = 0; c < counts.size(); c++) { base[c] = run; run += counts[c]; }
        CHECK(run == n, "the cells hold every key once");
        std::vector<uint32_t> rank(digits);
        for (uint64_t t = 0; t < n_tiles; t++) {
            std::fill(rank.begin(), rank.end(), 0u);
            const uint64_t end = std::min<uint64_t>(n, (t + 1) * kPostTileSpans);
            for (uint64_t i = t * kPostTileSpans; i < end; i++) {
                const uint32_t d = post_digit(p, keys[i], pass);
                const uint64_t dest = base[post_cell(d, t, n_tiles)] + rank[d]++;
                CHECK(dest < n, "dest %llu n %llu", (unsigned long long)dest, (unsigned long long)n);
                if (dest < n) { keys2[dest] = keys[i]; idx2[dest] = idx[i]; }
            }
        }
        keys.swap(keys2); idx.swap(idx2);
    }
}

void check_sort(uint64_t N, const std::vector<uint32_t>& keys_in, const char* what)
{
    std::vector<uint32_t> keys, idx;
    plan_sort(N, keys_in, keys, idx);
    const size_t n = keys_in.size();
    std::vector<uint32_t> want(n);
    std::iota(want.begin(), want.end(), 0u);
    std::stable_sort(want.begin(), want.end(), [&](uint32_t a, uint32_t b) { return keys_in[a] < keys_in[b]; });
    bool same = idx == want;
    for (size_t k = 0; k < n && same; k++) same = keys[k] == keys_in[want[k]];
    CHECK(same, "N %llu n %zu %s", (unsigned long long)N, n, what);
    // the offsets: a lower bound per needle over the sorted keys (checked for small N and at the ends of a large one)
    const uint64_t probes[] = {0, 1, N / 2, N ? N - 1 : 0, N};
    for (uint64_t v : probes) {
        if (v > N) continue;
        const uint64_t lb = post_lower_bound(keys.data(), n, 1, v);
        const uint64_t ref = (uint64_t)(std::lower_bound(keys.begin(), keys.end(), v, [](uint32_t k, uint64_t x) { return (uint64_t)k < x; }) - keys.begin());
        CHECK(lb == ref, "lower bound of %llu: %llu, not %llu", (unsigned long long)v, (unsigned long long)lb, (unsigned long long)ref);
    }
}

void check_row_search()
{
    // the haystack field of 24-byte rows: stride 6 words from word 4
    struct Row { uint64_t start, len; uint32_t haystack, needle; };
    static_assert(sizeof(Row) == 24, "24-byte rows");
    for (uint32_t n : {0u, 1u, 2u, 7u, 64u, 65u}) {
        std::vector<Row> rows(n);
        uint32_t h = 0;
        for (uint32_t k = 0; k < n; k++) { h += (uint32_t)(rnd() % 3); rows[k] = Row{k, 1, h, 5}; }
        for (uint32_t x = 0; x <= h + 2; x++) {
            uint64_t ref = 0;
            while (ref < n && rows[ref].haystack < x) ref++;
            const uint64_t got = n ? post_lower_bound((const uint32_t*)rows.data() + 4, n, sizeof(Row) / 4, x) : post_lower_bound(nullptr, 0, 6, x);
            CHECK(got == ref, "row search n %u x %u: %llu, not %llu", n, x, (unsigned long long)got, (unsigned long long)ref);
        }
    }
}

}  // namespace

int main()
{
    const uint64_t Ns[] = {1, 2, 255, 256, 257, 65535, 65536, 65537, (1ull << 24) + 2};
    for (uint64_t N : {0ull, 3ull, 4ull, 5ull, 127ull, 128ull, 129ull, (1ull << 24), (1ull << 24) + 1, (1ull << 32) - 1, 1ull << 32}) check_plan(N);
    const uint64_t T = kPostTileSpans;
    CHECK(kPostTileSpans % kPostWaveSpans == 0 && kPostWaveSpans % 64 == 0, "a tile is whole portions of whole rounds");
    const uint64_t sizes[] = {0, 1, 2, 63, 64, 65, T - 1, T, T + 1, 3 * T + 1};
    for (uint64_t N : Ns) {
        check_plan(N);
        for (uint64_t n : sizes) {
            std::vector<uint32_t> k(n);
            std::fill(k.begin(), k.end(), (uint32_t)(N - 1));
            check_sort(N, k, "all equal");
            for (uint64_t i = 0; i < n; i++) k[i] = (uint32_t)(i & 1 ? N - 1 : 0);
            check_sort(N, k, "two alternating keys");
            for (uint64_t i = 0; i < n; i++) k[i] = (uint32_t)(i & 1 ? (N - 1) ^ ((N - 1) & 1) : N - 1);
            check_sort(N, k, "two keys that differ in the lowest bit");
            for (uint64_t i = 0; i < n; i++) {                 // skewed: half of the keys from 4 hot needles, the rest uniform
                const uint64_t r = rnd();
                k[i] = (uint32_t)((r & 1) ? (r >> 8) % std::min<uint64_t>(N, 4) : (r >> 8) % N);
            }
            check_sort(N, k, "skewed random");
            for (uint64_t i = 0; i < n; i++) k[i] = (uint32_t)((N - 1 - i % N));      // descending cycles: every digit value of a small N inside one round
            check_sort(N, k, "descending cycles");
        }
    }
    check_row_search();
    if (g_failed) { std::printf("%d checks failed\n", g_failed); return 1; }
    std::printf("all checks passed\n");
    return 0;
}
