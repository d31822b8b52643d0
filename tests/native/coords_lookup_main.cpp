// coords_lookup_main.cpp -- a stand-alone program that runs the class masks, the tile counts' host twin and the lookup of csrc/am_coords.h (the code the kernels of
// am_coords.hip run) ON THE CPU and holds them to the byte loops of the definition (include/am.h "coordinates"), so that the arithmetic is checked -- bounds included,
// under a sanitizer -- before it meets a GPU:
//   g++ -std=c++17 -g -O1 [-fsanitize=address,undefined -fno-sanitize-recover=undefined -static-libasan -static-libubsan] -I alfred-margaret_amd/csrc \
//       tests/native/coords_lookup_main.cpp -o coords_lookup && ./coords_lookup
// The text is a heap block of exactly round_up(total, 16) bytes, 16-byte aligned, whose bytes from `total` on are 0x0A, 0xF0, 0x41, ...: a read beyond the padded end
// is a sanitizer report, a padding byte that is counted is a wrong number.  The prefix arrays hold exactly n_tiles + 1 entries.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "am_coords.h"

using namespace am::dev;

namespace {

int g_failed = 0;
unsigned long long g_checked = 0;

const uint8_t kAlphabet[] = {0x41, 0x0A, 0x80, 0xBF, 0xC3, 0xE2, 0xF0, 0xF4, 0xFF};
const uint8_t kPadding[] = {0x0A, 0xF0, 0x41};

bool in_class(uint32_t cls, uint8_t b)
{
    return cls == kCoordsStart ? (b & 0xC0) != 0x80 : cls == kCoordsFour ? b >= 0xF0 : b == 0x0A;
}

struct Index {
    uint8_t* text; uint64_t total, padded;
    uint64_t* prefix[kCoordsClasses];
    explicit Index(const std::vector<uint8_t>& bytes) : total(bytes.size()), padded((bytes.size() + 15) & ~15ull)
    {
        text = static_cast<uint8_t*>(std::aligned_alloc(16, padded ? padded : 16));
        for (uint64_t i = 0; i < (padded ? padded : 16); i++) text[i] = kPadding[i % 3];
        if (total) std::memcpy(text, bytes.data(), total);
        const uint64_t n_tiles = (total + kCoordsTile - 1) / kCoordsTile;
        std::vector<uint32_t> counts(n_tiles + 1);
        for (uint32_t c = 0; c < kCoordsClasses; c++) {
            if (c == kCoordsStart) coords_tile_counts_host<kCoordsStart>(text, total, counts.data());
            else if (c == kCoordsFour) coords_tile_counts_host<kCoordsFour>(text, total, counts.data());
            else coords_tile_counts_host<kCoordsNewline>(text, total, counts.data());
            prefix[c] = static_cast<uint64_t*>(std::malloc((n_tiles + 1) * 8));      // exactly n_tiles + 1 entries: an index beyond them is a report
            uint64_t run = 0;
            for (uint64_t t = 0; t <= n_tiles; t++) { prefix[c][t] = run; run += counts[t]; }
        }
    }
    ~Index() { std::free(text); for (auto* p : prefix) std::free(p); }
    CoordsIn in(const uint64_t* offsets, uint32_t n_hay) const
    {
        CoordsIn x{};
        x.text = text; x.offsets = offsets; x.total = total; x.padded = padded; x.n_hay = n_hay;
        for (uint32_t c = 0; c < kCoordsClasses; c++) x.prefix[c] = prefix[c];
        return x;
    }
};

void fail(const char* what, uint64_t base, uint64_t p, uint64_t got, uint64_t want)
{
    if (g_failed++ < 12) std::printf("FAILED: %s base %llu p %llu: %llu != %llu\n", what, (unsigned long long)base, (unsigned long long)p, (unsigned long long)got, (unsigned long long)want);
}

// every position of the haystack [base, end) against the byte loops: the three class counts, the line start, line and column in the three units
void check_haystack(const Index& ix, uint64_t base, uint64_t end)
{
    const uint64_t offsets[2] = {base, end};
    const CoordsIn in = ix.in(offsets, 1);
    const uint64_t c0[kCoordsClasses] = {coords_count<kCoordsStart>(ix.text, ix.prefix[0], base, ix.padded), coords_count<kCoordsFour>(ix.text, ix.prefix[1], base, ix.padded),
                                         coords_count<kCoordsNewline>(ix.text, ix.prefix[2], base, ix.padded)};
    uint64_t want[kCoordsClasses] = {0, 0, 0}, linestart = 0, at_linestart[kCoordsClasses] = {0, 0, 0};
    for (uint64_t p = 0; p <= end - base; p++) {
        const uint64_t g = base + p;
        const uint64_t got[kCoordsClasses] = {coords_count<kCoordsStart>(ix.text, ix.prefix[0], g, ix.padded) - c0[0],
                                              coords_count<kCoordsFour>(ix.text, ix.prefix[1], g, ix.padded) - c0[1],
                                              coords_count<kCoordsNewline>(ix.text, ix.prefix[2], g, ix.padded) - c0[2]};
        for (uint32_t c = 0; c < kCoordsClasses; c++) if (got[c] != want[c]) fail(c == 0 ? "cp" : c == 1 ? "four" : "line", base, p, got[c], want[c]);
        const uint64_t ls = coords_linestart(ix.text, ix.prefix[2], base, g, got[2] + c0[2], c0[2], ix.padded);
        if (ls != base + linestart) fail("linestart", base, p, ls - base, linestart);
        for (int unit = 0; unit < 3; unit++) {
            const uint64_t u = coords_units(in, unit, g) - coords_units(in, unit, base);
            const uint64_t wu = unit == 0 ? p : unit == 1 ? want[0] : want[0] + want[1];
            if (u != wu) fail("units", base, p, u, wu);
            const CoordsLineCol lc = coords_line_col(in, unit, base, c0[2], g, nullptr);
            const uint64_t wcol = unit == 0 ? p - linestart : unit == 1 ? want[0] - at_linestart[0] : want[0] + want[1] - at_linestart[0] - at_linestart[1];
            if (lc.line != want[2]) fail("line_col.line", base, p, lc.line, want[2]);
            if (lc.col != wcol) fail("line_col.col", base, p, lc.col, wcol);
            const CoordsLineCol again = coords_line_col(in, unit, base, c0[2], g, &lc);      // the reuse path: the same line
            if (again.col != wcol || again.linestart != lc.linestart) fail("line_col reuse", base, p, again.col, wcol);
        }
        g_checked++;
        if (p < end - base) {
            const uint8_t b = ix.text[g];
            for (uint32_t c = 0; c < kCoordsClasses; c++) want[c] += in_class(c, b);
            if (b == 0x0A) { linestart = p + 1; for (uint32_t c = 0; c < kCoordsClasses; c++) at_linestart[c] = want[c]; }
        }
    }
}

void masks_of_every_byte()
{
    for (uint32_t b = 0; b < 256; b++)
        for (uint32_t at = 0; at < 16; at++) {
            alignas(16) uint8_t grp[16];
            std::memset(grp, 0x80, 16);                     // (a continuation byte: in no class)
            grp[at] = (uint8_t)b;
            const CoordsWords v = coords_load(grp, 0);
            const uint32_t got[kCoordsClasses] = {coords_mask16<kCoordsStart>(v), coords_mask16<kCoordsFour>(v), coords_mask16<kCoordsNewline>(v)};
            for (uint32_t c = 0; c < kCoordsClasses; c++)
                if (got[c] != (in_class(c, (uint8_t)b) ? 1u << at : 0u)) fail("mask16", b, at, got[c], in_class(c, (uint8_t)b) ? 1u << at : 0u);
        }
    for (uint32_t m = 1; m < 65536; m += 7)
        for (uint32_t n = 1; n <= (uint32_t)__builtin_popcount(m); n++) {
            uint32_t want = 0, seen = 0;
            for (; want < 16; want++) if ((m >> want & 1) && ++seen == n) break;
            if (coords_nth_set(m, n) != want) fail("nth_set", m, n, coords_nth_set(m, n), want);
        }
}

}  // namespace

int main()
{
    std::mt19937 rng(20261020);
    masks_of_every_byte();
    // random byte strings at every base residue: a filler haystack of r bytes in front of the haystack under test, lengths up to 3 tiles + 17 bytes; a third of them
    // end the text exactly, so the last position is `total` (and with total % 128 == 0 the lookup there must load nothing: the block ends at total)
    const uint64_t lengths[] = {0, 1, 15, 16, 17, 127, 128, 129, 255, 256, 300, 384, 3 * 128 + 17};
    for (uint64_t r = 0; r < 16; r++)
        for (uint64_t len : lengths)
            for (int tail = 0; tail < 3; tail++) {
                std::vector<uint8_t> bytes;
                for (uint64_t i = 0; i < r; i++) bytes.push_back(kAlphabet[rng() % sizeof kAlphabet]);
                for (uint64_t i = 0; i < len; i++) bytes.push_back(rng() % 5 == 0 ? 0x41 : kAlphabet[rng() % sizeof kAlphabet]);
                const uint64_t extra = tail == 0 ? 0 : tail == 1 ? (128 - (r + len) % 128) % 128 : 1 + rng() % 40;      // ends the text / ends on a tile edge / a neighbour
                for (uint64_t i = 0; i < extra; i++) bytes.push_back(tail == 1 ? 0x41 : kAlphabet[rng() % sizeof kAlphabet]);
                Index ix(bytes);
                check_haystack(ix, r, r + len);
                if (tail == 1) check_haystack(ix, r, bytes.size());      // ends exactly at total, total % 128 == 0
                check_haystack(ix, 0, r);                   // the filler itself
                check_haystack(ix, r + len, bytes.size()); // what follows
            }
    // a planted line start 0, 1 and 5 tiles back: one newline in a text of letters and multi-byte sequences, the haystack beginning before it, at it, after it and in
    // the middle of the run behind it
    for (uint64_t back : std::vector<uint64_t>{0, 1, 5})
        for (uint64_t at : std::vector<uint64_t>{0, 1, 77, 127}) {
            std::vector<uint8_t> bytes(8 * 128 + 9);
            for (auto& b : bytes) { const uint32_t k = rng() % 8; b = k == 0 ? 0xC3 : k == 1 ? 0xF0 : k == 2 ? 0x80 : 0x41; }
            const uint64_t nl = (6 - back) * 128 + at;      // the positions of tile 6 look `back` tiles back
            bytes[nl] = 0x0A;
            Index ix(bytes);
            for (uint64_t base : std::vector<uint64_t>{0, 3, nl, nl + 1, nl + 2, nl + 130, 6 * 128 + 5}) check_haystack(ix, base < bytes.size() ? base : 0, bytes.size());
            check_haystack(ix, 0, nl);
            check_haystack(ix, 0, nl + 1);
        }
    // many newlines, and none
    for (int kind = 0; kind < 2; kind++) {
        std::vector<uint8_t> bytes(5 * 128, kind ? 0x0A : 0x41);
        Index ix(bytes);
        for (uint64_t base : std::vector<uint64_t>{0, 1, 128, 200}) check_haystack(ix, base, bytes.size());
    }
    { Index ix(std::vector<uint8_t>{}); check_haystack(ix, 0, 0); }
    if (g_failed) { std::printf("%d checks FAILED\n", g_failed); return 1; }
    std::printf("all checks passed (%llu positions)\n", g_checked);
    return 0;
}
