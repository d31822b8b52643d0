// near_pick_main.cpp -- a stand-alone program that runs the proximity join of csrc/am_near.h (near_pick, near_prev / near_next, near_bit_below / near_bit_above and
// the running maximum behind the word links: the __host__ __device__ functions k_near_bits, k_near_words, k_near_count and k_near_emit call) ON THE CPU, step by step
// as the kernels run it, and holds it to a brute-force loop over all spans, so that the join is checked -- every index it forms included, under a sanitizer --
// before it meets a GPU:
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=undefined -static-libasan -static-libubsan -I alfred-margaret_amd/csrc tests/native/near_pick_main.cpp \
//       -o near_pick && ./near_pick
// The bitmap rows and the links are heap blocks of exactly their size: a read beyond one is a sanitizer report.  Inputs: random sorted disjoint spans over a few
// haystacks (touching spans, empty haystacks, haystack seams inside a word), random group masks (needles in no group, in several), group_a == group_b, ordered and
// not, max_gap in {0, 1, small, 2^64 - 1}; 1, 2 and 5 words of 64 spans and the sizes around them; the links taken in sweeps of 1, 2 and 4 words with a carry.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "am_near.h"

using namespace am::dev;

namespace {

int g_failed = 0;
long g_pairs = 0, g_ties = 0, g_left = 0, g_right = 0;

// exact-size heap block: what the sanitizer watches
template <class T>
struct Block {
    T* p; size_t n;
    explicit Block(size_t count) : p(static_cast<T*>(std::calloc(count ? count : 1, sizeof(T)))), n(count) {}
    ~Block() { std::free(p); }
    Block(const Block&) = delete;
    Block& operator=(const Block&) = delete;
};

struct S { uint64_t start, len; uint32_t haystack, needle; };

// the definition: the minimum gap over ALL other spans of the group in the haystack, a tie to the lower index
NearPicked brute(const std::vector<S>& sp, const std::vector<uint32_t>& mask, size_t i, const NearQuery& q)
{
    bool has = false; uint64_t best = 0, b = 0;
    for (size_t j = 0; j < sp.size(); j++) {
        if (j == i || sp[j].haystack != sp[i].haystack || !(mask[sp[j].needle] >> q.group_b & 1u)) continue;
        if (j < i && (q.flags & kNearOrdered)) continue;
        const uint64_t gap = j < i ? sp[i].start - (sp[j].start + sp[j].len) : sp[j].start - (sp[i].start + sp[i].len);
        if (!has || gap < best) { has = true; best = gap; b = j; }
    }
    return NearPicked{has && best <= q.max_gap, b, best};
}

void run(std::mt19937_64& rng, size_t n, uint32_t sweep_words, uint32_t n_needles, uint32_t n_groups)
{
    // spans: ascending by (haystack, start), disjoint, len > 0
    std::vector<S> sp(n);
    uint32_t h = 0; uint64_t cursor = 0;
    for (size_t i = 0; i < n; i++) {
        if (rng() % 9 == 0) { h += 1 + (uint32_t)(rng() % 3 == 0); cursor = 0; }      // the next haystack, sometimes an empty one between
        cursor += rng() % 3 == 0 ? 0 : rng() % 6;                                     // touching spans are common
        sp[i] = S{cursor, 1 + rng() % 4, h, (uint32_t)(rng() % n_needles)};
        cursor += sp[i].len;
    }
    std::vector<uint32_t> mask(n_needles);
    for (auto& m : mask) m = rng() % 4 == 0 ? 0u : (uint32_t)(rng() & rng()) & ((n_groups >= 32 ? 0u : 1u << n_groups) - 1u);
    std::vector<NearQuery> qs;
    const uint64_t gaps[] = {0, 1, 2 + rng() % 5, ~0ull};
    for (int k = 0; k < 12; k++) {
        const uint32_t a = (uint32_t)(rng() % n_groups), b = k % 4 == 0 ? a : (uint32_t)(rng() % n_groups);
        qs.push_back(NearQuery{a, b, (uint32_t)(rng() & 1), 0, gaps[k % 4]});
    }
    const NearPlan plan = near_plan(qs.data(), (uint32_t)qs.size());
    const uint32_t n_words = (uint32_t)((n + 63) / 64);
    // k_near_bits: one word per 64 spans and row
    Block<uint64_t> bits((size_t)plan.n_rows * n_words);
    uint32_t row = 0;
    for (uint32_t g = 0; g < kNearMaxGroups; g++) {
        if (!(plan.used >> g & 1u)) continue;
        if (plan.row_of[g] != row) { std::printf("FAIL plan: group %u row %u expected %u\n", g, plan.row_of[g], row); g_failed++; }
        for (size_t i = 0; i < n; i++)
            if (mask[sp[i].needle] >> g & 1u) bits.p[(size_t)row * n_words + i / 64] |= 1ull << (i % 64);
        row++;
    }
    // k_near_words: sweeps of sweep_words words with a carry, both directions
    Block<uint32_t> prev_nz((size_t)plan.n_rows * n_words), next_nz((size_t)plan.n_rows * n_words);
    for (uint32_t r = 0; r < plan.n_rows; r++)
        for (int backwards = 0; backwards < 2; backwards++) {
            const uint64_t* b = bits.p + (size_t)r * n_words;
            uint32_t* link = (backwards ? next_nz.p : prev_nz.p) + (size_t)r * n_words;
            uint32_t carry = 0;
            for (uint32_t s0 = 0; s0 < n_words; s0 += sweep_words) {
                uint32_t run = carry;
                for (uint32_t k = 0; k < sweep_words && s0 + k < n_words; k++) {
                    const uint32_t step = s0 + k, w = near_link_index(step, backwards != 0, n_words);
                    link[w] = near_link_word(run, backwards != 0, n_words);
                    const uint32_t v = near_link_value(b[w], step);
                    run = v > run ? v : run;
                }
                carry = run;
            }
        }
    // the links against their definition
    for (uint32_t r = 0; r < plan.n_rows; r++)
        for (uint32_t w = 0; w < n_words; w++) {
            uint32_t ep = kNearNoWord, en = kNearNoWord;
            for (uint32_t k = 0; k < w; k++) if (bits.p[(size_t)r * n_words + k]) ep = k;
            for (uint32_t k = n_words; k-- > w + 1;) if (bits.p[(size_t)r * n_words + k]) en = k;
            if (prev_nz.p[(size_t)r * n_words + w] != ep || next_nz.p[(size_t)r * n_words + w] != en) { std::printf("FAIL links: row %u word %u\n", r, w); g_failed++; }
        }
    // k_near_count / k_near_emit: a lane per span, every query
    for (size_t i = 0; i < n; i++)
        for (size_t k = 0; k < qs.size(); k++) {
            const NearQuery& q = qs[k];
            if (!(mask[sp[i].needle] >> q.group_a & 1u)) continue;
            const uint32_t rb = plan.row_of[q.group_b];
            NearSide p{false, 0, 0, 0, 0}, nn{false, 0, 0, 0, 0};
            if (!(q.flags & kNearOrdered)) {
                const uint64_t j = near_prev(bits.p + (size_t)rb * n_words, prev_nz.p + (size_t)rb * n_words, i);
                if (j != kNearNone) { if (j >= i) { std::printf("FAIL prev index\n"); g_failed++; continue; } p = NearSide{true, j, sp[j].start, sp[j].len, sp[j].haystack}; }
            }
            const uint64_t j = near_next(bits.p + (size_t)rb * n_words, next_nz.p + (size_t)rb * n_words, i);
            if (j != kNearNone) { if (j <= i || j >= n) { std::printf("FAIL next index\n"); g_failed++; continue; } nn = NearSide{true, j, sp[j].start, sp[j].len, sp[j].haystack}; }
            const NearPicked got = near_pick(sp[i].start, sp[i].len, sp[i].haystack, p, nn, q.flags, q.max_gap), exp = brute(sp, mask, i, q);
            if (got.hit != exp.hit || (got.hit && (got.b != exp.b || got.gap != exp.gap))) {
                std::printf("FAIL pick: n %zu span %zu query %zu: got %d (%llu, %llu) expected %d (%llu, %llu)\n", n, i, k, (int)got.hit, (unsigned long long)got.b,
                            (unsigned long long)got.gap, (int)exp.hit, (unsigned long long)exp.b, (unsigned long long)exp.gap);
                g_failed++;
            }
            if (got.hit) {
                g_pairs++;
                const bool both = p.has && nn.has && p.haystack == sp[i].haystack && nn.haystack == sp[i].haystack;
                if (both && sp[i].start - (p.start + p.len) == nn.start - (sp[i].start + sp[i].len)) g_ties++;
                if (got.b < i) g_left++; else g_right++;
            }
        }
}

}  // namespace

int main()
{
    std::mt19937_64 rng(20251);
    // the bit arithmetic at its edges
    if (near_bit_below(~0ull, 0) != 64 || near_bit_below(1, 1) != 0 || near_bit_below(~0ull, 63) != 62 || near_bit_below(1ull << 63, 63) != 64) { std::printf("FAIL bit_below\n"); g_failed++; }
    if (near_bit_above(~0ull, 63) != 64 || near_bit_above(1ull << 63, 62) != 63 || near_bit_above(~0ull, 0) != 1 || near_bit_above(1, 0) != 64) { std::printf("FAIL bit_above\n"); g_failed++; }
    const size_t sizes[] = {1, 2, 63, 64, 65, 127, 128, 129, 257, 319, 320};      // 1, 2 and 5 words of 64 and the sizes around them
    for (size_t n : sizes)
        for (uint32_t sweep : {1u, 2u, 4u})
            for (int rep = 0; rep < 6; rep++) {
                run(rng, n, sweep, 1 + (uint32_t)(rng() % 9), rep % 2 ? 32u : 1u + (uint32_t)(rng() % 5));
            }
    if (g_pairs == 0 || g_ties == 0 || g_left == 0 || g_right == 0) { std::printf("FAIL coverage: pairs %ld ties %ld left %ld right %ld\n", g_pairs, g_ties, g_left, g_right); g_failed++; }
    if (g_failed) { std::printf("%d FAILED\n", g_failed); return 1; }
    std::printf("near_pick: all checks passed (%ld pairs, %ld ties, %ld left, %ld right)\n", g_pairs, g_ties, g_left, g_right);
    return 0;
}
