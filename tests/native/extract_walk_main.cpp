// extract_walk_main.cpp -- a stand-alone program that runs the group walk of csrc/am_extract.hip (start_mask16, nth_set_from_*, walk_left, walk_right: __host__
// __device__ functions) ON THE CPU and holds it to the byte-at-a-time definition of host/spans.hpp (extractWindow), so that the walk is checked -- bounds included,
// under a sanitizer -- before it meets a GPU:
//   hipcc --offload-arch=gfx950 -std=c++17 -g -O1 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined -I include \
//       -I alfred-margaret_amd/host -I alfred-margaret_amd/csrc -x hip tests/native/extract_walk_main.cpp -L alfred-margaret_amd/lib -lam \
//       -Wl,-rpath,alfred-margaret_amd/lib -o extract_walk && ./extract_walk
// The text is a heap block of exactly round_up(total, 16) bytes, 16-byte aligned, whose bytes from `total` on are START bytes (0x41): a read beyond the padded end is
// a sanitizer report, a padding byte that is counted is a wrong window.  Haystacks lie back to back at every residue mod 16, their neighbours end and begin with START
// bytes, and the fillers are 1- to 4-byte code points, runs of continuation bytes and a seeded mixture.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "../../alfred-margaret_amd/csrc/am_extract.hip"
#include "spans.hpp"

using namespace alfred_margaret;

namespace {

int g_failed = 0;

struct Block {
    uint8_t* p; uint64_t total, padded;
    explicit Block(const std::string& text) : total(text.size()), padded((text.size() + 15) & ~15ull)
    {
        p = static_cast<uint8_t*>(std::aligned_alloc(16, padded ? padded : 16));
        std::memset(p, 0x41, padded ? padded : 16);
        std::memcpy(p, text.data(), text.size());
    }
    ~Block() { std::free(p); }
};

std::string filler(std::mt19937& rng, int kind, size_t bytes)
{
    static const char* cp[] = {"a", "\xC3\xA9", "\xE2\x84\xAA", "\xF0\x9F\x98\x80"};
    std::string s;
    while (s.size() < bytes) {
        if (kind < 4) s += cp[kind];
        else if (kind == 4) s += (char)0x80;                // continuation bytes only
        else if (rng() % 7 == 0) s.append(1 + rng() % 40, (char)(0x80 + rng() % 64));
        else s += cp[rng() % 4];
    }
    s.resize(bytes);                                        // (may cut a code point: the definition is on bytes)
    return s;
}

void check(const Block& blk, uint64_t base, uint64_t next, uint64_t s, uint64_t l, uint32_t before, uint32_t after)
{
    const Text hay(blk.p, (size_t)base, (size_t)(next - base));
    const am_fragment want = extractWindow(hay, s, l, before, after);
    const uint64_t as = base + s, ae = as + l;
    const uint64_t ws = (before ? am::dev::walk_left(blk.p, base, as, before, blk.padded) : as) - base;
    const uint64_t we = (after ? am::dev::walk_right(blk.p, ae, next, after, blk.padded) : ae) - base;
    if (ws != want.start || we - ws != want.len) {
        if (g_failed++ < 10)
            std::printf("FAILED: base %llu next %llu span (%llu, %llu) before %u after %u: [%llu, %llu) != [%llu, %llu)\n", (unsigned long long)base, (unsigned long long)next,
                        (unsigned long long)s, (unsigned long long)l, before, after, (unsigned long long)ws, (unsigned long long)we, (unsigned long long)want.start,
                        (unsigned long long)(want.start + want.len));
    }
}

}  // namespace

int main()
{
    // the bit helpers, exhaustively
    for (uint32_t m = 1; m < 65536; m++) {
        uint32_t seen = 0;
        for (uint32_t j = 0; j < 16; j++) if (m >> j & 1) { seen++; if (am::dev::nth_set_from_bottom(m, seen) != j) g_failed++; }
        seen = 0;
        for (int j = 15; j >= 0; j--) if (m >> j & 1) { seen++; if (am::dev::nth_set_from_top(m, seen) != (uint32_t)j) g_failed++; }
    }
    std::mt19937 rng(20260101);
    for (int t = 0; t < 4096; t++) {
        uint8_t b[16]; uint32_t want = 0;
        for (int j = 0; j < 16; j++) { b[j] = (uint8_t)(t < 256 ? (j == t % 16 ? t : 0x80) : rng()); if ((b[j] & 0xC0) != 0x80) want |= 1u << j; }
        uint4 v; std::memcpy(&v, b, 16);
        if (am::dev::start_mask16(v) != want) g_failed++;
    }
    if (g_failed) { std::printf("%d checks of the bit helpers failed\n", g_failed); return 1; }

    const uint32_t widths[] = {0, 1, 2, 5, 15, 16, 17, 33, 1000, 0xFFFFFFFFu};
    uint64_t n_checks = 0;
    for (int kind = 0; kind < 6; kind++)
        for (size_t pad = 0; pad < 16; pad++)
            for (size_t tail = 0; tail < 16; tail += 5) {
                // [pad bytes ending in START bytes][the haystack][a neighbour beginning with START bytes, `tail` bytes]
                const size_t len = 90 + rng() % 40;
                const std::string text = std::string(pad, 'A') + filler(rng, kind, len) + std::string(tail, 'A');
                const Block blk(text);
                const uint64_t base = pad, next = pad + len;
                for (int k = 0; k < 24; k++) {
                    uint64_t s = rng() % (len + 1), l = rng() % 6;
                    if (k == 0) { s = 0; l = 0; }
                    if (k == 1) { s = len; l = 0; }
                    if (k == 2) { s = 0; l = len; }
                    if (s + l > len) l = len - s;
                    for (uint32_t bw : widths)
                        for (uint32_t aw : widths) { check(blk, base, next, s, l, bw, aw); n_checks++; }
                }
                // the empty haystack between the two neighbours
                check(blk, base, base, 0, 0, 3, 3);
                check(blk, next, next, 0, 0, 3, 3);
            }
    if (g_failed) std::printf("%d of %llu checks failed\n", g_failed, (unsigned long long)n_checks);
    else std::printf("extract_walk: all %llu checks passed\n", (unsigned long long)n_checks);
    return g_failed ? 1 : 0;
}
