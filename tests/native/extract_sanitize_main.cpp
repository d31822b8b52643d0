// extract_sanitize_main.cpp -- a stand-alone program over extractFold / extractWindow of host/spans.hpp (include/am.h "extract"), for a sanitizer run of HOST code
// without Python:
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=undefined -I include -I alfred-margaret_amd/host tests/native/extract_sanitize_main.cpp \
//       -L alfred-margaret_amd/lib -lam -Wl,-rpath,alfred-margaret_amd/lib -o extract_sanitize && ./extract_sanitize
// The spans are written out by hand (no automaton, no device).  Every haystack is a heap block of EXACTLY its own length, so a walk that leaves its haystack by one
// byte is a sanitizer report: windows that reach both ends exactly, one short and beyond, 1- to 4-byte code points, a haystack of continuation bytes only, the empty
// haystack, zero-length spans, the three-byte IgnoreCase span of U+212A, touching windows and windows one byte apart, a haystack that ends in a match followed by one
// that begins with a match.
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "spans.hpp"

using namespace alfred_margaret;

namespace {

int g_failed = 0;
void expect(bool ok, const char* what)
{
    if (!ok) { std::printf("FAILED: %s\n", what); g_failed++; }
}

// the texts, each in a heap block of its own length (a block of 1 byte for the empty one, never read)
struct Hays {
    std::vector<std::unique_ptr<uint8_t[]>> blocks;
    std::vector<Text> texts;
    explicit Hays(const std::vector<std::string>& s)
    {
        for (const std::string& t : s) {
            blocks.emplace_back(new uint8_t[t.size() ? t.size() : 1]);
            std::memcpy(blocks.back().get(), t.data(), t.size());
            texts.emplace_back(blocks.back().get(), 0, t.size());
        }
    }
};

Spans rows(const std::vector<std::vector<am_span>>& per_hay)
{
    Spans s;
    s.offsets.push_back(0);
    for (const auto& r : per_hay) { s.spans.insert(s.spans.end(), r.begin(), r.end()); s.offsets.push_back(s.spans.size()); }
    return s;
}

bool is(const am_fragment& f, uint64_t start, uint64_t len) { return f.start == start && f.len == len; }
std::vector<am_fragment> row(const Extracted& e, size_t h) { return std::vector<am_fragment>(e.fragments.begin() + (long)e.offsets[h], e.fragments.begin() + (long)e.offsets[h + 1]); }

}  // namespace

int main()
{
    // "the he she": he (0), the (1) in fold order -- (0,3,the) (1,2,he) (4,2,he) (8,2,he)
    {
        const Hays h({"the he she"});
        const Spans all = rows({{{0, 3, 0, 1}, {1, 2, 0, 0}, {4, 2, 0, 0}, {8, 2, 0, 0}}});
        const Extracted e = extractFold(all, h.texts, 1, 1, false);
        expect(e.fragments.size() == 4 && is(e.fragments[0], 0, 4) && is(e.fragments[1], 0, 4) && is(e.fragments[2], 3, 4) && is(e.fragments[3], 7, 3), "the he she, one code point either side");
        const Spans ll = rows({{{0, 3, 0, 1}, {4, 2, 0, 0}, {8, 2, 0, 0}}});
        const Extracted m0 = extractFold(ll, h.texts, 0, 0, true), m1 = extractFold(ll, h.texts, 0, 1, true), m2 = extractFold(ll, h.texts, 1000, 1000, true);
        expect(m0.fragments.size() == 3, "no context: a gap of one byte separates");
        expect(m1.fragments.size() == 2 && is(m1.fragments[0], 0, 7) && is(m1.fragments[1], 8, 2), "touching windows join: [0, 4) and [4, 7); [8, 10) is one byte away");
        expect(m2.fragments.size() == 1 && is(m2.fragments[0], 0, 10), "windows beyond both ends: the whole haystack, once");
        bool threw = false;
        try { (void)extractFold(all, h.texts, 0, 0, true); } catch (const AmError&) { threw = true; }
        expect(threw, "merged refuses rows that overlap");
    }
    // 1- to 4-byte code points: a (1) e-acute (2) Kelvin (3) emoji (4) x (1) emoji Kelvin e-acute a
    {
        const std::string t = std::string("a\xC3\xA9\xE2\x84\xAA\xF0\x9F\x98\x80") + "x" + "\xF0\x9F\x98\x80\xE2\x84\xAA\xC3\xA9" "a";
        const Hays h({t});
        const Spans s = rows({{{10, 1, 0, 0}}});
        const uint64_t ws[] = {10, 6, 3, 1, 0, 0}, we[] = {11, 15, 18, 20, 21, 21};
        for (uint32_t n = 0; n < 6; n++) {
            const Extracted e = extractFold(s, h.texts, n, n, false);
            expect(e.fragments.size() == 1 && is(e.fragments[0], ws[n], we[n] - ws[n]), "n code points of 4, 3, 2, 1 bytes either side; the ends exactly at n = 4, beyond at n = 5");
        }
        // the Kelvin sign matched by k under IgnoreCase: the span is three bytes
        const Extracted k = extractFold(rows({{{3, 3, 0, 0}}}), h.texts, 1, 1, false);
        expect(is(k.fragments[0], 1, 9), "U+212A: one code point before its three bytes, one after");
    }
    // continuation bytes only, the empty haystack, zero-length spans
    {
        const Hays h({std::string(40, (char)0x80), "", "ab"});
        const Spans s = rows({{{20, 1, 0, 0}, {0, 0, 0, 0}, {40, 0, 0, 0}}, {{0, 0, 1, 0}}, {{0, 0, 2, 0}, {1, 0, 2, 0}, {2, 0, 2, 0}}});
        const Extracted e = extractFold(s, h.texts, 2, 2, false), z = extractFold(s, h.texts, 0, 0, false);
        expect(is(e.fragments[0], 0, 40) && is(e.fragments[1], 0, 40) && is(e.fragments[2], 0, 40), "no START byte: both walks run to the ends");
        expect(is(e.fragments[3], 0, 0), "the empty haystack");
        expect(is(e.fragments[4], 0, 2) && is(e.fragments[5], 0, 2) && is(e.fragments[6], 0, 2), "zero-length spans of ab: the byte AT e is not counted, the one behind it is");
        expect(z.fragments.size() == 7 && is(z.fragments[5], 1, 0) && z.offsets == s.offsets, "no context: zero-length fragments are kept, the rows are the spans'");
        const Extracted one = extractFold(rows({{}, {}, {{1, 0, 2, 0}}}), h.texts, 0, 1, false);
        expect(is(one.fragments[0], 1, 1), "after = 1 at e = 1 of ab: the START byte at index 2 does not exist, we = L");
    }
    // a haystack that ends in a match followed by one that begins with a match: two pieces, both clamped to the shared boundary
    {
        const Hays h({"..ab", "ab..", "", "ab"});
        const Spans s = rows({{{2, 2, 0, 0}}, {{0, 2, 1, 0}}, {}, {{0, 2, 3, 0}}});
        const Extracted m = extractFold(s, h.texts, 5, 5, true);
        expect(m.fragments.size() == 3 && is(m.fragments[0], 0, 4) && is(m.fragments[1], 0, 4) && is(m.fragments[2], 0, 2), "one piece per haystack");
        expect(m.offsets == std::vector<uint64_t>({0, 1, 2, 2, 3}), "the empty haystack and the rows' offsets");
        expect(row(m, 2).empty(), "no span, no piece");
    }
    // no haystacks, and spans that are not those of the texts
    {
        const Extracted e = extractFold(rows({}), {}, 3, 3, true);
        expect(e.offsets == std::vector<uint64_t>({0}) && e.fragments.empty(), "no haystacks: offsets [0]");
        const Hays h({"ab"});
        bool threw = false;
        try { (void)extractFold(rows({{{1, 2, 0, 0}}}), h.texts, 1, 1, false); } catch (const AmError&) { threw = true; }
        expect(threw, "a span that leaves its haystack is refused without a read");
        threw = false;
        try { (void)extractFold(rows({{}, {}}), h.texts, 1, 1, false); } catch (const AmError&) { threw = true; }
        expect(threw, "rows of another haystack count are refused");
    }
    std::printf(g_failed ? "%d checks failed\n" : "extract_sanitize: all checks passed\n", g_failed);
    return g_failed ? 1 : 0;
}
