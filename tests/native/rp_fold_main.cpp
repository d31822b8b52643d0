// rp_fold_main.cpp -- a stand-alone program over what csrc/am_wave.h and csrc/am_rp_fold.h declare without HIP: the backward code-point walk (Utf8.hs:256-276) over
// plain bytes and over a piece list, and rp_piece_fragments, the splice of the kept matches of a Replacer pass into a piece list (Replacer.hs:163-180).  The very
// functions the kernels call, run on the CPU.  argv[1]: a file of known answers, one per line: <text in hex> <index> <n> <expected>.  Every array is a vector of
// exactly the size the device gives it, so under AddressSanitizer a read beyond one is reported.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

// the plain-data structs of csrc/am_device.h, which needs the HIP runtime (am_rp_fold.h: a program without HIP declares them first)
namespace am {
namespace dev {
struct RpPayload { int64_t priority; uint32_t len_bytes; uint32_t len_code_points; uint64_t repl_off; uint32_t repl_len; uint32_t reserved; };
struct RpStateOne { int32_t priority; uint32_t payload; };
struct RpTables { const uint64_t* vals_off; const uint32_t* vals; const RpPayload* payloads; const uint8_t* repl; int64_t min_priority; const RpStateOne* one; };
struct RpKept { uint64_t src_start, src_len, dst; };
struct RpPiece { uint64_t src; uint64_t lstart; };
constexpr uint64_t kPieceRepl = 1ull << 63;
}  // namespace dev
}  // namespace am

#include "am_rp_fold.h"

using namespace am::dev;
typedef std::vector<uint8_t> Bytes;

namespace {

int failures = 0;
uint64_t checks = 0;

void expect(bool ok, const char* what, uint64_t a = 0, uint64_t b = 0, uint64_t c = 0)
{
    checks++;
    if (ok) return;
    if (++failures <= 20) std::fprintf(stderr, "FAILED: %s (%llu, %llu, %llu)\n", what, (unsigned long long)a, (unsigned long long)b, (unsigned long long)c);
}

// the walk as the Replacer's kernels had it before there was one: (index of the match's last byte, n) -- what the shared (end_pos, n) form must agree with
uint64_t old_walk(const uint8_t* hay, uint64_t index, uint64_t n)
{
    int64_t i = (int64_t)index;
    for (;;) {
        while (i > 0 && (hay[i] & 0xC0u) == 0x80u) i--;
        if (n == 0 || i <= 0) return (uint64_t)(i < 0 ? 0 : i);
        i--; n--;
    }
}

// A text as a piece list: the parts [cuts[k], cuts[k + 1]) lie at unrelated places of two blobs (odd parts in the replacement blob, tagged), with other bytes
// between them; `empties` empty pieces before every part, their sources pointing at the blobs' ends (a read through one is out of bounds).
struct Pieced {
    Bytes text, repl;
    std::vector<RpPiece> P;                                 // the sentinel included
    uint32_t n() const { return (uint32_t)P.size() - 1; }
    Pieced(const Bytes& whole, const std::vector<uint64_t>& cuts, uint32_t empties)
    {
        for (size_t k = 0; k + 1 < cuts.size(); k++) {
            Bytes& blob = (k & 1) ? repl : text;
            blob.insert(blob.end(), 3, 0x80);              // continuation bytes beside every part: a walk that left its piece would go on through them
            blob.insert(blob.end(), whole.begin() + (long)cuts[k], whole.begin() + (long)cuts[k + 1]);
        }
        uint64_t at_text = 0, at_repl = 0;
        for (size_t k = 0; k + 1 < cuts.size(); k++) {
            uint64_t& at = (k & 1) ? at_repl : at_text;
            const uint64_t tag = (k & 1) ? kPieceRepl : 0;
            for (uint32_t e = 0; e < empties; e++) P.push_back(RpPiece{(e & 1) ? kPieceRepl | repl.size() : text.size(), cuts[k]});
            P.push_back(RpPiece{tag | (at + 3), cuts[k]});
            at += 3 + (cuts[k + 1] - cuts[k]);
        }
        P.push_back(RpPiece{0, whole.size()});
    }
    Bytes materialise() const
    {
        Bytes out;
        for (uint32_t i = 0; i < n(); i++) { const uint8_t* b = rp_piece_base(P[i].src, text.data(), repl.data()); out.insert(out.end(), b, b + (P[i + 1].lstart - P[i].lstart)); }
        return out;
    }
};

// one answer of the walk, on the plain bytes and through every piece list with up to two cuts
void check_walk(const Bytes& t, uint64_t index, uint32_t n, uint64_t want, bool every_cut)
{
    expect(skip_code_points_backwards(t.data(), index + 1, n) == want, "the walk over plain bytes", index, n, want);
    for (uint64_t c1 = 0; c1 <= t.size(); c1++) {
        for (uint64_t c2 = c1; c2 <= t.size(); c2 += every_cut ? 1 : 1 + t.size() / 3) {
            for (uint32_t empties = 0; empties < 3; empties += 2) {
                const Pieced p(t, {0, c1, c2, t.size()}, empties);
                expect(rp_skip_code_points_backwards(p.P.data(), p.n(), p.text.data(), p.repl.data(), index + 1, n) == want, "the walk through a piece list", c1, c2, index);
            }
        }
    }
}

Bytes from_hex(const std::string& h)
{
    Bytes b;
    for (size_t i = 0; i + 1 < h.size(); i += 2) b.push_back((uint8_t)std::strtoul(h.substr(i, 2).c_str(), nullptr, 16));
    return b;
}

// `replace` (Replacer.hs:163-180) on bytes: the gaps between the matches and the replacement in place of each
Bytes replace_ref(const Bytes& old_text, const std::vector<RpKept>& K, const Bytes& replacement)
{
    Bytes out;
    uint64_t x = 0;
    for (const RpKept& k : K) {
        out.insert(out.end(), old_text.begin() + (long)x, old_text.begin() + (long)k.src_start);
        out.insert(out.end(), replacement.begin(), replacement.end());
        x = k.src_start + k.src_len;
    }
    out.insert(out.end(), old_text.begin() + (long)x, old_text.end());
    return out;
}

}  // namespace

int main(int argc, char** argv)
{
    if (argc < 2) { std::fprintf(stderr, "usage: rp_fold_main <known answers>\n"); return 2; }
    // ---- the known answers of the reference's own tests
    std::FILE* f = std::fopen(argv[1], "r");
    if (!f) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    char hex[256]; unsigned long long index, n, want;
    uint64_t rows = 0;
    while (std::fscanf(f, "%255s %llu %llu %llu", hex, &index, &n, &want) == 4) { check_walk(from_hex(hex), index, (uint32_t)n, want, true); rows++; }
    std::fclose(f);
    expect(rows >= 20, "known answers were read", rows);

    // ---- random byte strings, half of their bytes continuation bytes: the (end_pos, n) form against the (index, n) form the kernels had, and through piece lists
    std::mt19937_64 rng(20260321);
    uint64_t cont_at_0 = 0, beyond = 0;
    for (int it = 0; it < 4000; it++) {
        Bytes t(1 + rng() % 24);
        for (uint8_t& b : t) { const uint64_t r = rng(); b = (r & 1) ? (uint8_t)(0x80 | ((r >> 8) & 0x3F)) : (r & 2) ? (uint8_t)(0xC0 | ((r >> 8) & 0x3F)) : (uint8_t)((r >> 8) & 0x7F); }
        const uint64_t idx = rng() % t.size();
        uint32_t starts = 0;
        for (uint64_t i = 0; i <= idx; i++) starts += (t[i] & 0xC0u) != 0x80u;
        const uint32_t nn = (uint32_t)(rng() % (it % 4 == 0 ? 40 : starts + 2));      // (beyond the text's code points among them)
        cont_at_0 += (t[0] & 0xC0u) == 0x80u;
        beyond += nn >= starts;
        const uint64_t w = old_walk(t.data(), idx, nn);
        expect(nn < starts || w == 0, "a walk beyond the text's first code point answers 0", idx, nn, w);
        check_walk(t, idx, nn, w, it < 400);
    }
    expect(cont_at_0 > 500 && beyond > 500, "the random strings hold continuation bytes at position 0 and n beyond the code points", cont_at_0, beyond);
    const Bytes one_start = {0x80, 0x80, 0x41, 0x80};
    expect(skip_code_points_backwards(one_start.data(), 0, 0) == 0 && skip_code_points_backwards(one_start.data(), 2, 0) == 0, "an empty prefix and one of continuation bytes answer 0");
    expect(skip_code_points_backwards(one_start.data(), 4, 0) == 2 && skip_code_points_backwards(one_start.data(), 4, 0xFFFFFFFFu) == 0, "n == 0 and the largest n");

    // ---- the piece fragments: random piece lists, random sorted disjoint kept matches of at least one byte (an automaton with the empty needle does not come
    // here), one replacement per pass.  The fragments taken piece by piece are a piece list again; its text is `replace` applied to the old list's text.
    uint64_t spanning = 0, at_front = 0, at_back = 0, empty_repl = 0, tagged = 0;
    for (int it = 0; it < 3000; it++) {
        Bytes whole(1 + rng() % 60);
        for (uint8_t& b : whole) b = (uint8_t)(0x61 + rng() % 26);
        std::vector<uint64_t> cuts = {0};
        while (cuts.back() < whole.size()) cuts.push_back(std::min<uint64_t>(whole.size(), cuts.back() + rng() % 9));      // (empty parts among them)
        const Pieced p(whole, cuts, (uint32_t)(rng() % 2));
        expect(p.materialise() == whole, "the piece list describes its text");
        Bytes replacement(it % 5 == 0 ? 0 : rng() % 7);
        for (uint8_t& b : replacement) b = (uint8_t)(0x41 + rng() % 26);
        Bytes repl = p.repl;                                // the replacement lies behind the list's own parts in the blob
        const uint64_t repl_off = repl.size();
        repl.insert(repl.end(), replacement.begin(), replacement.end());
        std::vector<RpKept> K;
        int64_t delta = 0;
        const uint64_t gap = rng() % 12;
        for (uint64_t x = it % 3 == 0 ? 0 : rng() % 4; x < whole.size();) {
            uint64_t len = 1 + rng() % (it % 7 == 0 ? 20 : 5);
            if (it % 11 == 0 || x + len > whole.size()) len = whole.size() - x;      // (a match that ends with the text)
            K.push_back(RpKept{x, len, (uint64_t)((int64_t)x + delta)});
            delta += (int64_t)replacement.size() - (int64_t)len;
            x += len + rng() % (gap + 1);
        }
        std::vector<RpPiece> Q;
        uint64_t counted = 0;
        for (uint32_t i = 0; i < p.n(); i++) {
            rp_piece_fragments(p.P.data(), i, K.data(), (uint32_t)K.size(), replacement.size(), kPieceRepl | repl_off, [&](uint64_t, uint64_t) { counted++; });
            rp_piece_fragments(p.P.data(), i, K.data(), (uint32_t)K.size(), replacement.size(), kPieceRepl | repl_off, [&](uint64_t src, uint64_t pos) { Q.push_back(RpPiece{src, pos}); });
        }
        expect(counted == Q.size() && Q.size() <= p.n() + 2 * K.size(), "the counting sweep and the writing sweep agree, within the bound the kernels reserve", counted, Q.size());
        const Bytes want_text = replace_ref(whole, K, replacement);
        Q.push_back(RpPiece{0, (uint64_t)((int64_t)whole.size() + delta)});
        Bytes got;
        bool ordered = Q[0].lstart == 0 || Q.size() == 1;
        for (size_t i = 0; i + 1 < Q.size() && ordered; i++) {
            ordered = Q[i].lstart < Q[i + 1].lstart;         // (no empty entry is made)
            if (!ordered) break;
            const uint8_t* b = rp_piece_base(Q[i].src, p.text.data(), repl.data());
            got.insert(got.end(), b, b + (Q[i + 1].lstart - Q[i].lstart));
        }
        expect(ordered, "the new list's starts ascend from 0", (uint64_t)it);
        expect(got == want_text, "the new list's text is replace applied to the old text", (uint64_t)it, got.size(), want_text.size());
        for (const RpKept& k : K) {
            const uint32_t a = rp_piece_at(p.P.data(), p.n(), k.src_start), b = rp_piece_at(p.P.data(), p.n(), k.src_start + k.src_len - 1);
            spanning += b > a + 1;
        }
        for (uint32_t i = 0; i < p.n(); i++) tagged += (p.P[i].src & kPieceRepl) != 0 && p.P[i + 1].lstart > p.P[i].lstart;
        at_front += !K.empty() && K[0].src_start == 0;
        at_back += !K.empty() && K.back().src_start + K.back().src_len == whole.size();
        empty_repl += replacement.empty() && !K.empty();
    }
    expect(spanning > 100 && at_front > 100 && at_back > 100 && empty_repl > 100 && tagged > 1000, "the cases hold matches over several pieces, at both ends, empty replacements and tagged pieces", spanning, at_front,
           at_back);

    if (failures) { std::fprintf(stderr, "%d checks failed\n", failures); return 1; }
    std::printf("%llu checks, all checks passed\n", (unsigned long long)checks);
    return 0;
}
