// cased_compare_main.cpp -- a stand-alone program over the comparator of csrc/am_cased.h (include/am.h "exact case"), run on the CPU against memcmp: the very function
// the kernels call.  Every buffer is a vector of exactly the size the comparator may read -- the text round_up(total, 16) bytes, the pool the spelling rounded up to a
// group --, so under AddressSanitizer a read beyond either is reported, and what lies in the text's padding and beside the span is filled with non-zero bytes, so a
// result that depended on it would differ from memcmp's.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "am_cased.h"

namespace {

int failures = 0;

void expect(bool ok, const char* what, uint64_t a = 0, uint64_t b = 0, uint64_t c = 0)
{
    if (ok) return;
    if (++failures <= 20) std::fprintf(stderr, "FAILED: %s (%llu, %llu, %llu)\n", what, (unsigned long long)a, (unsigned long long)b, (unsigned long long)c);
}

uint64_t up16(uint64_t n) { return (n + 15) & ~15ull; }

uint8_t spell(uint64_t i) { return (uint8_t)(0x41 + (i * 7 + i / 5) % 53); }      // never 0, never 0xEE

// a text of `total` bytes in a buffer of round_up(total, 16), filled with 0xEE (the padding too), the spelling at `start`; the pool: the spelling at `at`, zero-filled
// to the next group, exactly that long
struct Case {
    std::vector<uint8_t> text, pool;
    uint64_t total, start, len, at;
    Case(uint64_t total_, uint64_t start_, uint64_t len_, uint64_t groups_before) : total(total_), start(start_), len(len_), at(groups_before * am::kCasedGroup)
    {
        text.assign((size_t)up16(total), 0xEE);
        pool.assign((size_t)(at + am::cased_padded(len)), 0);
        for (uint64_t i = 0; i < at; i++) pool[(size_t)i] = 0xDD;      // another spelling's bytes before this one
        for (uint64_t i = 0; i < len; i++) text[(size_t)(start + i)] = pool[(size_t)(at + i)] = spell(i);
    }
    bool run(uint64_t lo, uint64_t hi) const { return am::cased_equal(text.data(), lo, hi, start, pool.data(), at, len); }
    bool want() const { return len == 0 || std::memcmp(text.data() + start, pool.data() + at, (size_t)len) == 0; }
};

}  // namespace

int main()
{
    uint64_t checks = 0;
    // every spelling length 0 .. 48 at every start residue 0 .. 15, in the middle of a text; then a single differing byte at every position, on the text's side and
    // on the pool's
    for (uint64_t len = 0; len <= 48; len++) {
        for (uint64_t res = 0; res < 16; res++) {
            Case c(16 + res + len + 21, 16 + res, len, res % 3);
            expect(c.run(0, c.total) && c.want(), "equal bytes compare equal", len, res);
            expect(c.run(c.start, c.start + len), "a span that is its whole haystack", len, res);
            checks += 2;
            for (uint64_t p = 0; p < len; p++) {
                Case d = c;
                d.text[(size_t)(d.start + p)] ^= 0x20;                 // the other case of a letter
                expect(!d.run(0, d.total) && !d.want(), "one differing byte in the text", len, res, p);
                Case e = c;
                e.pool[(size_t)(e.at + p)] ^= 0x01;
                expect(!e.run(0, e.total) && !e.want(), "one differing byte in the pool", len, res, p);
                checks += 2;
            }
            // the bytes right before and right behind the span do not count, whatever they are
            Case f = c;
            f.text[(size_t)(f.start - 1)] = 0x00;
            f.text[(size_t)(f.start + len)] = 0x00;
            expect(f.run(0, f.total), "the neighbours of the span are not compared", len, res);
            checks++;
        }
    }
    // a span that ends on the last byte of its haystack, another haystack behind it; and one that ends on the last byte of the TEXT, with 0xEE where the padding is
    for (uint64_t len = 1; len <= 48; len++) {
        for (uint64_t res = 0; res < 16; res++) {
            Case c(res + len + 9, res, len, 1);
            expect(c.run(0, res + len), "a span that ends on the last byte of its haystack", len, res);
            expect(!c.run(0, res + len - 1), "a span that leaves its haystack at the end is unequal", len, res);
            expect(res == 0 || !c.run(res + 1, c.total), "a span that begins before its haystack is unequal", len, res);
            Case t(res + len, res, len, 0);                           // total = start + len: the buffer ends at round_up(total, 16)
            expect(t.run(0, t.total) && t.want(), "a span that ends on the last byte of the text", len, res);
            Case u = t;
            u.text[(size_t)(u.start + len - 1)] ^= 0x20;
            expect(!u.run(0, u.total), "... and differs in that byte", len, res);
            checks += 5;
        }
    }
    // long spellings: 17, 257 and 66 000 bytes, identical, differing in the first byte, differing in the last byte
    const uint64_t longs[3] = {17, 257, 66000};
    for (uint64_t len : longs) {
        for (uint64_t res = 0; res < 16; res += 5) {
            Case c(res + len, res, len, 2);
            expect(c.run(0, c.total) && c.want(), "a long spelling", len, res);
            Case d = c; d.text[(size_t)d.start] ^= 0x20;
            expect(!d.run(0, d.total), "a long spelling that differs in its first byte", len, res);
            Case e = c; e.text[(size_t)(e.start + len - 1)] ^= 0x20;
            expect(!e.run(0, e.total), "a long spelling that differs in its last byte", len, res);
            checks += 3;
        }
    }
    if (failures) { std::fprintf(stderr, "%d checks failed\n", failures); return 1; }
    std::printf("%llu checks, all checks passed\n", (unsigned long long)checks);
    return 0;
}
