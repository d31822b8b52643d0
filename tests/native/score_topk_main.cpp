// score_topk_main.cpp -- a stand-alone program that runs the top-k selection of csrc/am_score.h (score_key, topk_pick, topk_in_prefix, topk_digit: the
// __host__ __device__ functions k_topk_hist, k_topk_pick, k_topk_ties and k_topk_flags call) ON THE CPU, pass by pass as the kernels run it, and holds it to
// std::sort, so that the select is checked -- every index it forms included, under a sanitizer -- before it meets a GPU:
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=undefined -I alfred-margaret_amd/csrc tests/native/score_topk_main.cpp \
//       -o score_topk && ./score_topk
// The scores and the 256 bins are heap blocks of exactly their size: a read beyond one is a sanitizer report.  Inputs: random arrays over the whole int64 range and
// over small ranges (many ties), all keys equal, keys that differ only in the top byte or only in the bottom byte, INT64_MIN and INT64_MAX, n around a power of two;
// k in {0, 1, n - 1, n, n + 7} and a few inside; both directions.  k == 0 and k >= n are answered by the caller (am_select_top_k, am_scores_top_k) without a pass, as
// here.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "am_score.h"

using namespace am::dev;

namespace {

int g_failed = 0;

// exact-size heap copy: what the sanitizer watches
template <class T>
struct Block {
    T* p; size_t n;
    explicit Block(size_t count) : p(static_cast<T*>(std::calloc(count ? count : 1, sizeof(T)))), n(count) {}
    ~Block() { std::free(p); }
    Block(const Block&) = delete;
    Block& operator=(const Block&) = delete;
};

// the flags of the min(k, n) best scores, as the device computes them
std::vector<uint8_t> select(const std::vector<int64_t>& scores, uint64_t k, bool largest)
{
    const size_t n = scores.size();
    std::vector<uint8_t> flags(n, 0);
    if (k == 0 || n == 0) return flags;
    if (k >= n) { std::fill(flags.begin(), flags.end(), 1); return flags; }
    Block<int64_t> col(n);
    for (size_t i = 0; i < n; i++) col.p[i] = scores[i];
    Block<uint64_t> hist(kTopkBins);
    TopkState st{0, k};                                     // k_topk_init
    for (uint32_t digit = kTopkDigits; digit-- > 0;) {
        for (size_t i = 0; i < n; i++) {                    // k_topk_hist
            const uint64_t key = score_key(col.p[i], largest);
            if (topk_in_prefix(key, st.prefix, digit)) hist.p[topk_digit(key, digit)]++;
        }
        uint64_t left = st.k_left;                          // k_topk_pick
        const uint32_t d = topk_pick(hist.p, &left);
        if (d >= kTopkBins || left == 0 || left > hist.p[d]) { std::printf("FAIL pick: digit %u bin %u left %llu\n", digit, d, (unsigned long long)left); g_failed++; }
        st.prefix = (st.prefix << 8) | d;
        st.k_left = left;
        for (uint32_t b = 0; b < kTopkBins; b++) hist.p[b] = 0;
    }
    uint64_t rank = 0;                                      // k_topk_ties, the exclusive sum, k_topk_flags
    for (size_t i = 0; i < n; i++) {
        const uint64_t key = score_key(col.p[i], largest);
        flags[i] = key > st.prefix || (key == st.prefix && rank < st.k_left) ? 1 : 0;
        if (key == st.prefix) rank++;
    }
    return flags;
}

void check(const char* what, const std::vector<int64_t>& scores, uint64_t k, bool largest)
{
    const size_t n = scores.size();
    std::vector<uint32_t> order(n);
    for (size_t i = 0; i < n; i++) order[i] = (uint32_t)i;
    std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) {
        if (scores[a] != scores[b]) return largest ? scores[a] > scores[b] : scores[a] < scores[b];
        return a < b;
    });
    std::vector<uint8_t> expect(n, 0);
    for (size_t i = 0; i < std::min<uint64_t>(k, n); i++) expect[order[i]] = 1;
    const std::vector<uint8_t> got = select(scores, k, largest);
    if (got != expect) {
        size_t at = 0;
        while (at < n && got[at] == expect[at]) at++;
        std::printf("FAIL %s: n %zu k %llu largest %d: haystack %zu got %d expected %d\n", what, n, (unsigned long long)k, (int)largest, at, (int)got[at], (int)expect[at]);
        g_failed++;
    }
}

void check_all_k(const char* what, const std::vector<int64_t>& scores, std::mt19937_64& rng)
{
    const uint64_t n = scores.size();
    std::vector<uint64_t> ks{0, 1, n ? n - 1 : 0, n, n + 7, n / 2, n / 3 + 1};
    for (int i = 0; i < 3 && n; i++) ks.push_back(rng() % n);
    for (uint64_t k : ks)
        for (int largest = 0; largest < 2; largest++) check(what, scores, k, largest != 0);
}

}  // namespace

int main()
{
    std::mt19937_64 rng(20241);
    // the key is order-preserving in both directions
    const int64_t edge[] = {INT64_MIN, INT64_MIN + 1, -1, 0, 1, INT64_MAX - 1, INT64_MAX};
    for (int64_t a : edge)
        for (int64_t b : edge) {
            if ((a < b) != (score_key(a, true) < score_key(b, true)) || (a < b) != (score_key(a, false) > score_key(b, false))) { std::printf("FAIL key %lld %lld\n", (long long)a, (long long)b); g_failed++; }
        }
    const size_t sizes[] = {1, 2, 3, 63, 64, 65, 255, 256, 257, 1000, 4099};
    for (size_t n : sizes) {
        std::vector<int64_t> v(n);
        for (auto& x : v) x = (int64_t)rng();
        check_all_k("random 64-bit", v, rng);
        for (auto& x : v) x = (int64_t)(rng() % 7) - 3;
        check_all_k("seven values", v, rng);
        for (auto& x : v) x = 42;
        check_all_k("all equal", v, rng);
        for (auto& x : v) x = INT64_MIN;
        check_all_k("all INT64_MIN", v, rng);
        for (size_t i = 0; i < n; i++) v[i] = i % 2 ? 42 : -7;
        check_all_k("half equal", v, rng);
        for (auto& x : v) x = (int64_t)((rng() & 0xFFull) << 56);          // the top byte only (the sign among its bits)
        check_all_k("top byte", v, rng);
        for (auto& x : v) x = (int64_t)(0x0123456789ABCD00ull | (rng() & 0xFFull));      // the bottom byte only
        check_all_k("bottom byte", v, rng);
        for (auto& x : v) x = (int64_t)((rng() & 0xFFull) << 24) | 0x11;   // one byte in the middle
        check_all_k("middle byte", v, rng);
        for (size_t i = 0; i < n; i++) v[i] = i % 3 == 0 ? INT64_MIN : (i % 3 == 1 ? INT64_MAX : (int64_t)(rng() % 3) - 1);
        check_all_k("extremes", v, rng);
        for (size_t i = 0; i < n; i++) v[i] = (int64_t)i * ((int64_t)1 << 32) - ((int64_t)n << 31);      // ascending, the signs split
        check_all_k("ascending", v, rng);
    }
    check_all_k("empty", {}, rng);
    if (g_failed) { std::printf("%d FAILED\n", g_failed); return 1; }
    std::printf("score_topk: all checks passed\n");
    return 0;
}
