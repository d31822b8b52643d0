// chain_select_main.cpp -- a stand-alone program that runs the chain selector of csrc/am_chain.h (chain_walk, chain_next, chain_double: the code the kernels of
// am_chain.hip run, one call per lane) and the owner search of csrc/am_rows.h ON THE CPU, element by element, and holds them to the sequential definition and to
// std::upper_bound.  Every array is a vector of exactly the size the device gives it, so a sanitizer build checks the bounds as well.
//   g++ -std=c++17 -g -O1 [-fsanitize=address,undefined -fno-sanitize-recover=undefined -static-libasan -static-libubsan] -I alfred-margaret_amd/csrc
//       tests/native/chain_select_main.cpp -o chain_select && ./chain_select
// No HIP, no GPU, no Python.
#include <algorithm>
#include <cstdio>
#include <random>
#include <vector>

#include "am_chain.h"

using namespace am::dev;

namespace {

int g_failed = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (g_failed++ < 20) { std::printf("FAILED %s:%d %s: ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

// an ascending list of intervals: per row the starts ascend strictly and the ends do not descend (the Splitter's records are sorted by end)
struct Interval { uint32_t row; uint64_t start, end; };

// the sequential definition: keep an element iff it is the first of its row or starts at or after the end of the last kept element of its row
std::vector<uint32_t> definition(const std::vector<Interval>& v)
{
    std::vector<uint32_t> kept(v.size() + 1, 0);
    uint64_t last_end = 0;
    for (size_t i = 0; i < v.size(); i++) {
        const bool first = i == 0 || v[i].row != v[i - 1].row;
        if (first || v[i].start >= last_end) { kept[i] = 1; last_end = v[i].end; }
    }
    return kept;
}

uint32_t ceil_log2(uint64_t k) { uint32_t r = 0; while ((1ull << r) < k) r++; return r; }

// what the device does with a view and its heads: kept = head, the heads' lanes walk with the limit, and -- when a chain was left over, or always (force) -- next[]
// for every element and doubling rounds until a round marks nothing.  Returns the rounds.
template <class View>
uint32_t select_on_cpu(const View& view, const std::vector<uint8_t>& head, uint32_t limit, bool force, std::vector<uint32_t>& kept, bool* doubled)
{
    const uint64_t n = view.n;
    kept.assign(n + 1, 0);
    for (uint64_t i = 0; i < n; i++) kept[i] = head[i];
    bool long_chains = false;
    for (uint64_t i = 0; i < n; i++) if (head[i] && chain_walk(view, head.data(), kept.data(), limit, i)) long_chains = true;
    *doubled = n != 0 && (long_chains || force);
    if (!*doubled) return 0;
    std::vector<uint64_t> jump[2] = {std::vector<uint64_t>(n), std::vector<uint64_t>(n)};
    for (uint64_t i = 0; i < n; i++) {
        const uint64_t j = chain_next(view, head.data(), i);
        CHECK(j == i || (j > i && j < n && !head[j] && view.same_row(i, j) && view.start(j) >= view.end(i) && view.start(j - 1) < view.end(i)), "next[%llu] = %llu", (unsigned long long)i, (unsigned long long)j);
        jump[0][i] = j;
    }
    uint32_t rounds = 0;
    for (bool marked = true; marked && rounds < 64; rounds++) {
        marked = false;
        for (uint64_t i = 0; i < n; i++) if (chain_double(jump[rounds & 1].data(), jump[(rounds & 1) ^ 1].data(), n, kept.data(), i)) marked = true;
    }
    return rounds;
}

// the longest kept path of a chain
uint64_t longest_path(const std::vector<uint8_t>& head, const std::vector<uint32_t>& kept)
{
    uint64_t best = 0, run = 0;
    for (size_t i = 0; i < head.size(); i++) { if (head[i]) run = 0; run += kept[i]; best = std::max(best, run); }
    return best;
}

template <class View>
void run_view(const char* what, const char* view_name, const View& view, const std::vector<uint8_t>& head, const std::vector<uint32_t>& want)
{
    for (uint32_t limit : {1u, 2u, 32u}) {
        for (bool force : {false, true}) {
            std::vector<uint32_t> kept;
            bool doubled = false;
            const uint32_t rounds = select_on_cpu(view, head, limit, force, kept, &doubled);
            CHECK(kept == want, "%s, %s, n %llu, limit %u, force %d: kept differs from the definition", what, view_name, (unsigned long long)view.n, limit, (int)force);
            if (doubled) {
                const uint32_t bound = ceil_log2(longest_path(head, want)) + 1;
                CHECK(rounds >= 1 && rounds <= bound, "%s, %s, n %llu, limit %u: %u rounds, bound %u", what, view_name, (unsigned long long)view.n, limit, rounds, bound);
            }
        }
    }
}

void run_case(const char* what, const std::vector<Interval>& v)
{
    const uint64_t n = v.size();
    const std::vector<uint32_t> want = definition(v);
    // the Splitter's view: positions relative to the row; a head is the first of its row or starts at or after the end of its predecessor
    {
        std::vector<Record> recs(n);
        std::vector<uint64_t> starts(n);
        std::vector<uint8_t> head(n + 1, 0);
        for (uint64_t i = 0; i < n; i++) {
            recs[i] = Record{v[i].end, v[i].row, 0};
            starts[i] = v[i].start;
            head[i] = i == 0 || v[i].row != v[i - 1].row || v[i].start >= v[i - 1].end;
        }
        run_view(what, "records", SplitChain{recs.data(), starts.data(), n}, head, want);
    }
    // the spans' view: global positions, the rows laid out back to back; a head starts at or after every end before it (an exclusive prefix maximum)
    {
        std::vector<uint64_t> cand_g(n), best(n);
        std::vector<uint8_t> head(n + 1, 0);
        uint64_t base = 0, max_end = 0;
        for (uint64_t i = 0; i < n; i++) {
            if (i > 0 && v[i].row != v[i - 1].row) base = max_end;
            cand_g[i] = base + v[i].start;
            best[i] = ((v[i].end - v[i].start) << 32) | (uint32_t)~(uint32_t)(i % 7);
            head[i] = cand_g[i] >= max_end;
            max_end = std::max(max_end, base + v[i].end);
        }
        run_view(what, "candidates", SpansChain{cand_g.data(), best.data(), n}, head, want);
    }
}

void chains()
{
    run_case("nothing", {});
    for (uint64_t n = 1; n <= 70; n++) {                    // "aa" over a run of a's: one chain through everything, a kept path of 1 .. 35 (across 2, 4, ..., 32)
        std::vector<Interval> v;
        for (uint64_t i = 0; i < n; i++) v.push_back({0, i, i + 2});
        run_case("one chain", v);
    }
    for (uint64_t n = 1; n <= 140; n += 3) {                // ... and over 64 kept with length 2 at step 1
        std::vector<Interval> v;
        for (uint64_t i = 0; i < n; i++) v.push_back({0, i, i + 2});
        run_case("one long chain", v);
    }
    std::mt19937_64 rng(20260101);
    for (int rep = 0; rep < 200; rep++) {                   // two lengths at steps of 1 and 2: next skips one or two elements
        std::vector<Interval> v;
        const uint64_t n = 1 + rng() % 90;
        uint64_t s = 0, e = 0;
        for (uint64_t i = 0; i < n; i++) {
            s += 1 + rng() % 2;
            e = std::max(e, s + 2 + rng() % 2);
            v.push_back({0, s, e});
        }
        run_case("two lengths", v);
    }
    for (uint64_t n : {1, 2, 3, 64, 65}) {                  // disjoint intervals: every element is a head
        std::vector<Interval> v;
        for (uint64_t i = 0; i < n; i++) v.push_back({0, 3 * i, 3 * i + 2 + i % 2});
        run_case("all heads", v);
    }
    for (int rep = 0; rep < 200; rep++) {                   // several rows: each begins again at relative starts below the ends of the row before it
        std::vector<Interval> v;
        const uint32_t rows = 2 + (uint32_t)(rng() % 5);
        for (uint32_t r = 0; r < rows; r++) {
            const uint64_t n = (r == 0 ? 3 : 1) + rng() % 40;
            uint64_t s = rng() % 2, e = 0;
            for (uint64_t i = 0; i < n; i++) {
                e = std::max(e, s + 2 + rng() % 3);
                v.push_back({r, s, e});
                s += 1 + (rng() % 8 == 0 ? 5 : rng() % 2);
            }
        }
        run_case("several rows", v);
    }
    {                                                       // "aa" over 9, 2 and 11 a's: chains of three and more that end at a row boundary
        std::vector<Interval> v;
        uint32_t r = 0;
        for (uint64_t len : {9, 2, 11}) { for (uint64_t i = 0; i + 2 <= len; i++) v.push_back({r, i, i + 2}); r++; }
        run_case("aa over three rows", v);
        for (Interval& x : v) if (x.row == 2) { x.start++; x.end++; }      // ... the last one behind a "b": its kept starts are odd, a jump that strays into it shows
        run_case("aa over three rows, the last one shifted", v);
    }
}

template <class T, class I>
void owner_search(const char* what)
{
    std::mt19937_64 rng(7);
    for (size_t len : {1, 2, 3, 64, 65}) {
        for (int rep = 0; rep < 50; rep++) {
            std::vector<T> off(len);
            T x = (T)(rng() % 3);
            for (size_t i = 0; i < len; i++) { off[i] = x; if (rng() % 3) x = (T)(x + rng() % 4); }      // ascending, with repeated values
            for (I lo = 0; lo < (I)len; lo += (I)(1 + len / 5)) {
                for (I hi = lo; hi < (I)len; hi += (I)(1 + len / 7)) {
                    for (uint64_t q = off[lo]; q <= (uint64_t)off[hi] + 1; q++) {
                        const I got = last_at_or_before(off.data(), lo, hi, q);
                        const I want = (I)(std::upper_bound(off.begin() + lo, off.begin() + hi + 1, q, [](uint64_t a, T b) { return a < (uint64_t)b; }) - off.begin() - 1);
                        CHECK(got == want, "%s, len %zu, [%llu, %llu], x %llu: %llu, upper_bound says %llu", what, len, (unsigned long long)lo, (unsigned long long)hi,
                              (unsigned long long)q, (unsigned long long)got, (unsigned long long)want);
                    }
                }
            }
        }
    }
}

}  // namespace

int main()
{
    chains();
    owner_search<uint64_t, uint64_t>("uint64_t offsets, 64-bit indices");
    owner_search<uint16_t, uint32_t>("uint16_t offsets, 32-bit indices");
    if (g_failed) { std::printf("%d checks FAILED\n", g_failed); return 1; }
    std::printf("all checks passed\n");
    return 0;
}
