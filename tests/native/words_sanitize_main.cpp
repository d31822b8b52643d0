// words_sanitize_main.cpp -- a stand-alone program over the word-class code of host/spans.hpp (wholeWord, defaultWordBytes, spansFold and substitute with a class), for
// a sanitizer run of HOST code without Python:
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=undefined -I include -I alfred-margaret_amd/host tests/native/words_sanitize_main.cpp \
//       -L alfred-margaret_amd/lib -lam -Wl,-rpath,alfred-margaret_amd/lib -o words_sanitize && ./words_sanitize
// The fold steps are written out by hand (no automaton, no device): neighbours at both ends of a haystack, haystacks back to back in ONE buffer so that a read across a
// seam would see a word byte, an empty haystack, zero-length spans, a three-byte IgnoreCase match, handles beyond the table, the four classes of the tests.
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
    uint8_t dflt[256], none[256], full[256], lower[256];
    defaultWordBytes(dflt);
    std::memset(none, 0, 256);
    std::memset(full, 1, 256);
    for (unsigned b = 0; b < 256; b++) lower[b] = b >= 'a' && b <= 'z';
    int n_word = 0;
    for (unsigned b = 0; b < 256; b++) n_word += dflt[b];
    expect(n_word == 10 + 26 + 26 + 1 + 128 && dflt[(unsigned char)'_'] && !dflt[(unsigned char)'+'] && dflt[0x80] && !dflt[0x7F], "the default class");

    // one buffer, haystacks back to back: "xab" "ab" "" "abx" "a" "b" -- needles ab (0), a (1), b (2); then "ab cd" with ab (0) and `ab c` (3); then " K " with k (4)
    const std::string buf = std::string("xab") + "ab" + "" + "abx" + "a" + "b" + "ab cd" + " \xE2\x84\xAA ";
    const uint8_t* p = reinterpret_cast<const uint8_t*>(buf.data());
    const std::vector<Text> texts = {Text(p, 0, 3), Text(p, 3, 2), Text(p, 5, 0), Text(p, 5, 3), Text(p, 8, 1), Text(p, 9, 1), Text(p, 10, 5), Text(p, 15, 5)};
    const std::vector<uint32_t> lenBytes = {2, 1, 1, 4, 1, 0}, lenCps = {2, 1, 1, 4, 1, 0};
    const std::vector<FoldStep> steps = {
        {0, 2, 1}, {0, 3, 0}, {0, 3, 2},                    // xab: a, ab, b
        {1, 1, 1}, {1, 2, 0}, {1, 2, 2}, {1, 2, 5},         // ab: a, ab, b and a zero-length span at its end (after a word byte: none)
        {2, 0, 5},                                          // the empty haystack: a zero-length span without neighbours
        {3, 1, 1}, {3, 2, 0}, {3, 2, 2},                    // abx
        {4, 1, 1}, {4, 1, 99},                              // a (and a handle beyond the table: skipped)
        {5, 1, 2},                                          // b
        {6, 1, 1}, {6, 2, 0}, {6, 2, 2}, {6, 4, 3},         // ab cd: a, ab, b, `ab c`
        {7, 4, 4},                                          // U+212A matched by k: three bytes wide under IgnoreCase
    };
    for (int ic = 0; ic < 2; ic++) {
        const CaseSensitivity cs = ic ? CaseSensitivity::IgnoreCase : CaseSensitivity::CaseSensitive;
        for (int ll = 0; ll < 2; ll++) {
            const Spans s = spansFold(cs, ll != 0, steps, texts, lenBytes, lenCps, dflt);
            expect(row(s, 0).empty() && row(s, 3).empty(), "xab and abx hold no whole word");
            expect(row(s, 2).size() == (ll ? 0u : 1u) && (ll || is(row(s, 2)[0], 0, 0, 5)), "the zero-length span of the empty haystack is a row, never selected");
            expect(row(s, 1).size() == 1 && is(row(s, 1)[0], 0, 2, 0), "ab is a whole word of the haystack ab, whatever stands before and behind it in the buffer");
            expect(row(s, 4).size() == 1 && is(row(s, 4)[0], 0, 1, 1) && row(s, 5).size() == 1 && is(row(s, 5)[0], 0, 1, 2), "a and b alone");
            expect(row(s, 6).size() == 1 && is(row(s, 6)[0], 0, 2, 0), "ab cd: ab, not `ab c` -- filter, then select");
            if (ic) expect(row(s, 7).size() == 1 && is(row(s, 7)[0], 1, 3, 4), "U+212A: the left neighbour is three bytes before the end");
            const Spans e = spansFold(cs, ll != 0, steps, texts, lenBytes, lenCps, none), q = spansFold(cs, ll != 0, steps, texts, lenBytes, lenCps, nullptr);
            expect(e.offsets == q.offsets && e.spans.size() == q.spans.size() &&
                   (e.spans.empty() || std::memcmp(e.spans.data(), q.spans.data(), e.spans.size() * sizeof(am_span)) == 0), "the empty class is the plain fold");
            const Spans f = spansFold(cs, false, steps, texts, lenBytes, lenCps, full);
            for (const am_span& x : f.spans) expect(x.start == 0 && x.start + x.len == texts[x.haystack].len, "the full class keeps only a span that is its whole haystack");
            (void)spansFold(cs, ll != 0, steps, texts, lenBytes, lenCps, lower);
        }
        const std::vector<std::string> repl = {"X", "", "<seventeen bytes!>", "Y", "K", "-"};
        const std::vector<std::string> out = substitute(cs, steps, texts, lenBytes, lenCps, repl, dflt), raw = substitute(cs, steps, texts, lenBytes, lenCps, repl);
        expect(out[0] == "xab" && out[1] == "X" && out[2].empty() && out[3] == "abx" && out[4].empty() && out[5] == "<seventeen bytes!>" && out[6] == "X cd", "substitute over whole words");
        expect(raw[6] == "Yd" && raw[0] == "xX", "substitute over the plain selection");
        if (ic) expect(out[7] == " K ", "substitute removes the span's own three bytes");
    }
    expect(!wholeWord(texts[1], 1, 5, dflt) && !wholeWord(texts[1], 3, 0, dflt) && wholeWord(texts[2], 0, 0, dflt), "a span that leaves its haystack is none; the empty span of the empty haystack is one");
    std::printf(g_failed ? "%d checks failed\n" : "words_sanitize: all checks passed\n", g_failed);
    return g_failed ? 1 : 0;
}
