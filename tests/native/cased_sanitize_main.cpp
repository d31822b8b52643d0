// cased_sanitize_main.cpp -- a stand-alone program over the exact-case code of host/spans.hpp (exactCase, spansFold and substituteFold with spellings), for a
// sanitizer run of HOST code without Python:
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=undefined -I include -I alfred-margaret_amd/host tests/native/cased_sanitize_main.cpp \
//       -L alfred-margaret_amd/lib -lam -Wl,-rpath,alfred-margaret_amd/lib -o cased_sanitize && ./cased_sanitize
// The fold steps are written out by hand (no automaton, no device): the examples of include/am.h "exact case", haystacks back to back in ONE buffer so that a read
// across a seam would find the spelling's missing byte, a spelling longer than its haystack, a list of spellings shorter than the table, both case modes, a class.
#include <cstdio>
#include <cstring>
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

std::vector<am_span> row(const Spans& s, size_t h) { return std::vector<am_span>(s.spans.begin() + (long)s.offsets[h], s.spans.begin() + (long)s.offsets[h + 1]); }
bool is(const am_span& s, uint64_t start, uint64_t len, uint32_t v) { return s.start == start && s.len == len && s.needle == v; }

}  // namespace

int main()
{
    const CaseSensitivity ic = CaseSensitivity::IgnoreCase, cs = CaseSensitivity::CaseSensitive;
    uint8_t dflt[256];
    defaultWordBytes(dflt);
    // one buffer: "us, US and NIKE's apple" "U" "S" "bonUS" -- needles us (0), apple (1), nike (2); U | S: neighbouring haystacks never complete each other
    const std::string buf = std::string("us, US and NIKE's apple") + "U" + "S" + "bonUS";
    const uint8_t* p = reinterpret_cast<const uint8_t*>(buf.data());
    const std::vector<Text> texts = {Text(p, 0, 23), Text(p, 23, 1), Text(p, 24, 1), Text(p, 25, 5)};
    const std::vector<uint32_t> lb = {2, 5, 4}, lc = {2, 5, 4};
    const std::vector<FoldStep> steps = {{0, 2, 0}, {0, 6, 0}, {0, 15, 2}, {0, 23, 1}, {3, 5, 0}};
    const ExactSpellings exact = {std::string("US"), std::string("Apple"), std::nullopt};
    for (int ll = 0; ll < 2; ll++) {
        const Spans s = spansFold(ic, ll != 0, steps, texts, lb, lc, nullptr, &exact);
        expect(s.offsets == std::vector<uint64_t>({0, 2, 2, 2, 3}), "plain filtering: the offsets");
        expect(s.spans.size() == 3 && is(s.spans[0], 4, 2, 0) && is(s.spans[1], 11, 4, 2) && is(s.spans[2], 3, 2, 0), "plain filtering: (4,2,us) (11,4,nike), and the US of bonUS");
        const Spans w = spansFold(ic, ll != 0, steps, texts, lb, lc, dflt, &exact);
        expect(w.spans.size() == 2 && row(w, 3).empty(), "with the default class both predicates must hold");
        const Spans none = spansFold(ic, ll != 0, steps, texts, lb, lc, nullptr, nullptr), empty = spansFold(ic, ll != 0, steps, texts, lb, lc, nullptr, nullptr);
        expect(none.spans.size() == 5 && empty.offsets == none.offsets, "no spellings: every span is a row");
        const ExactSpellings shorter = {std::string("US")};
        expect(spansFold(ic, ll != 0, steps, texts, lb, lc, nullptr, &shorter).spans.size() == 5 - 1, "a list shorter than the table: the handles beyond it have no spelling");
    }
    expect(substituteFold(ic, steps, texts, lb, lc, {"<0>", "<1>", "<2>"}, nullptr, &exact) == std::vector<std::string>({"us, <0> and <2>'s apple", "U", "S", "bon<0>"}),
           "substituteFold over the kept rows");
    const Spans sens = spansFold(cs, false, {{0, 2, 0}, {0, 15, 2}}, texts, lb, lc, nullptr, &exact);
    expect(sens.spans.size() == 1 && is(sens.spans[0], 11, 4, 2), "case-sensitive: the needle's own length, the same rule -- us is not spelled US, nike has no spelling");
    // exactCase itself: a span at the end of its haystack, a spelling longer than the haystack, a span that leaves it, the empty span
    expect(exactCase(texts[3], 3, 2, exact[0]) && !exactCase(texts[3], 2, 2, exact[0]) && !exactCase(texts[3], 3, 3, exact[0]), "bonUS: only [3, 5) spells US");
    expect(!exactCase(texts[1], 0, 1, exact[0]) && !exactCase(texts[1], 0, 2, exact[0]) && !exactCase(texts[2], 1, 1, exact[0]), "U | S: no row, and no read beyond the haystack");
    expect(exactCase(texts[1], 0, 1, std::nullopt) && exactCase(texts[1], 1, 0, std::string()) && !exactCase(texts[1], 2, 0, std::string()), "no spelling keeps; the empty spelling is the empty span");
    // widths: k with exact = K keeps K and drops U+212A (len 3); with exact = U+212A the keeps and the drops swap
    const std::string kk = "K k \xE2\x84\xAA";
    const std::vector<Text> kt = {Text(reinterpret_cast<const uint8_t*>(kk.data()), 0, kk.size())};
    const std::vector<FoldStep> ks = {{0, 1, 0}, {0, 3, 0}, {0, 7, 0}};
    const ExactSpellings asK = {std::string("K")}, asKelvin = {std::string("\xE2\x84\xAA")};
    const Spans a = spansFold(ic, false, ks, kt, {1}, {1}, nullptr, &asK), b = spansFold(ic, false, ks, kt, {1}, {1}, nullptr, &asKelvin);
    expect(a.spans.size() == 1 && is(a.spans[0], 0, 1, 0) && b.spans.size() == 1 && is(b.spans[0], 4, 3, 0), "widths: K, or U+212A");
    // filter, then select: `ab c` (0) with exact = `AB C`, ab (1) without a spelling over "ab c"
    const std::string ab = "ab c";
    const std::vector<Text> at = {Text(reinterpret_cast<const uint8_t*>(ab.data()), 0, 4)};
    const ExactSpellings abx = {std::string("AB C"), std::nullopt};
    const Spans sel = spansFold(ic, true, {{0, 2, 1}, {0, 4, 0}}, at, {4, 2}, {4, 2}, nullptr, &abx);
    expect(sel.spans.size() == 1 && is(sel.spans[0], 0, 2, 1) && spansFold(ic, true, {{0, 2, 1}, {0, 4, 0}}, at, {4, 2}, {4, 2}).spans[0].len == 4, "filter, then select");
    if (g_failed) { std::printf("%d checks failed\n", g_failed); return 1; }
    std::printf("all checks passed\n");
    return 0;
}
