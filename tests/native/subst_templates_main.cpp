// subst_templates_main.cpp -- a stand-alone program that runs the piece plan of a table of substitution templates (csrc/am_subst_tpl.h: subst_tpl_count,
// subst_tpl_segments, subst_tpl_gap_piece / subst_tpl_seg_piece and subst_tpl_piece, the __host__ __device__ functions k_subst_tpl_count, k_subst_tpl_pieces and
// k_subst_compact call) ON THE CPU, step by step as the kernels run it -- the counts, their exclusive sum, the pieces, the exclusive sum of their lengths, the
// out_offsets, then a plain copy of every piece from its tagged source -- and holds the bytes and the offsets to the sequential definition (host/spans.hpp
// substituteTemplates), byte for byte, so that the plan is checked -- every index it forms included, under a sanitizer -- before it meets a GPU:
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=undefined -static-libasan -static-libubsan -I alfred-margaret_amd/csrc \
//       -I alfred-margaret_amd/host -I include tests/native/subst_templates_main.cpp -o subst_templates && ./subst_templates
// The piece arrays, the pool and the text are heap blocks of exactly their size: a read or write beyond one is a sanitizer report.  Inputs: random sorted disjoint
// spans over a few haystacks (touching spans, empty haystacks, matches at both ends), templates of 0, 1 and 64 segments and the sizes between, empty literals,
// adjacent MATCHes, needles that share a template shape, and a handle the table does not know.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "am_subst_tpl.h"
#include "spans.hpp"

using namespace am::dev;
namespace amh = alfred_margaret;

namespace {

int g_failed = 0;
long g_pieces = 0, g_empty = 0, g_match = 0, g_literal = 0, g_adjacent = 0, g_full = 0, g_none = 0;

// exact-size heap block: what the sanitizer watches
template <class T>
struct Block {
    T* p; size_t n;
    explicit Block(size_t count) : p(static_cast<T*>(std::calloc(count ? count : 1, sizeof(T)))), n(count) {}
    ~Block() { std::free(p); }
    Block(const Block&) = delete;
    Block& operator=(const Block&) = delete;
    T& at(size_t i) { if (i >= n) { std::printf("FAIL index %zu of %zu\n", i, n); g_failed++; std::exit(1); } return p[i]; }
};

void run(std::mt19937_64& rng, uint32_t n_needles, uint32_t n_hay, bool force_shapes)
{
    // the table: templates of handle v, as am_subst_table_create_templates lays them out
    std::vector<amh::Template> tpl(n_needles);
    std::vector<uint64_t> seg_off(n_needles + 1, 0);
    std::vector<SubstSeg> segs;
    std::string pool;
    for (uint32_t v = 0; v < n_needles; v++) {
        uint32_t nseg = (uint32_t)(rng() % 6);
        if (force_shapes) nseg = v % 4 == 0 ? 0 : v % 4 == 1 ? 1 : v % 4 == 2 ? kSubstMaxSegments : 2 + (uint32_t)(rng() % 5);
        bool prev_match = false;
        for (uint32_t s = 0; s < nseg; s++) {
            const bool match = rng() % 5 < 2;
            if (match) {
                tpl[v].push_back(amh::TemplateSegment{true, std::string()});
                segs.push_back(SubstSeg{0, 0, kSegMatch});
                if (prev_match) g_adjacent++;
            } else {
                const size_t len = rng() % 3 == 0 ? 0 : (size_t)(rng() % 20);
                std::string lit(len, 'A');
                for (auto& c : lit) c = (char)('A' + rng() % 26);
                tpl[v].push_back(amh::TemplateSegment{false, lit});
                segs.push_back(SubstSeg{(uint64_t)pool.size(), (uint32_t)len, kSegLiteral});
                pool += lit;
            }
            prev_match = match;
        }
        if (nseg == kSubstMaxSegments) g_full++;
        if (nseg == 0) g_none++;
        seg_off[v + 1] = segs.size();
    }
    Block<uint8_t> pool_b(pool.size());
    if (!pool.empty()) std::memcpy(pool_b.p, pool.data(), pool.size());
    Block<SubstSeg> segs_b(segs.size());
    for (size_t i = 0; i < segs.size(); i++) segs_b.p[i] = segs[i];
    Block<uint64_t> seg_off_b(seg_off.size());
    for (size_t i = 0; i < seg_off.size(); i++) seg_off_b.p[i] = seg_off[i];

    // the batch and its leftmost-longest spans: ascending, disjoint, len > 0
    std::vector<std::string> hays(n_hay);
    amh::Spans sp;
    sp.offsets.assign(n_hay + 1, 0);
    for (uint32_t h = 0; h < n_hay; h++) {
        sp.offsets[h] = sp.spans.size();
        const size_t len = rng() % 4 == 0 ? 0 : (size_t)(rng() % 120);
        hays[h].resize(len);
        for (auto& c : hays[h]) c = (char)('a' + rng() % 26);
        uint64_t cursor = rng() % 3 == 0 ? 0 : rng() % 4;                   // a match at the very start is common
        while (cursor < len) {
            uint64_t l = 1 + rng() % 5;
            if (cursor + l > len || rng() % 7 == 0) l = len - cursor;       // ... and one that ends the haystack
            sp.spans.push_back(am_span{cursor, l, h, (uint32_t)(rng() % n_needles)});
            cursor += l + (rng() % 3 == 0 ? 0 : rng() % 6);                 // touching spans are common
        }
    }
    sp.offsets[n_hay] = sp.spans.size();
    const uint64_t S = sp.spans.size();
    std::vector<uint64_t> src_off(n_hay + 1, 0);
    std::string text;
    for (uint32_t h = 0; h < n_hay; h++) { src_off[h] = text.size(); text += hays[h]; }
    src_off[n_hay] = text.size();
    Block<uint8_t> text_b(text.size());
    if (!text.empty()) std::memcpy(text_b.p, text.data(), text.size());

    // k_subst_tpl_count, a lane per span and the trailing zero; launch_scan: its exclusive sum
    Block<uint32_t> cnt(S + 1);
    for (uint64_t j = 0; j < S; j++) cnt.at(j) = subst_tpl_count(seg_off_b.p, n_needles, sp.spans[j].needle);
    Block<uint64_t> pbase(S + 1);
    { uint64_t run = 0; for (uint64_t j = 0; j <= S; j++) { pbase.at(j) = run; run += cnt.at(j); } }
    const uint64_t P = pbase.at(S) + n_hay;
    // k_subst_tpl_pieces: lens / src_at / live, P + 1 entries, zero before; every piece must be written exactly once
    Block<uint64_t> lens(P + 1), src_at(P + 1);
    Block<uint32_t> live(P + 1), written(P + 1);
    auto put = [&](uint64_t i, uint64_t len, uint64_t at) {
        if (i >= P) { std::printf("FAIL piece index %llu of %llu\n", (unsigned long long)i, (unsigned long long)P); g_failed++; return; }
        lens.at(i) = len; src_at.at(i) = at; live.at(i) = len != 0; written.at(i)++;
    };
    for (uint64_t j = 0; j < S; j++) {
        const am_span& s = sp.spans[j];
        const uint32_t h = s.haystack;
        const uint64_t base = src_off[h], first = sp.offsets[h];
        const uint64_t prev_end = j > first ? sp.spans[j - 1].start + sp.spans[j - 1].len : 0;
        put(subst_tpl_gap_piece(pbase.at(j), h), s.start - prev_end, base + prev_end);
        uint64_t s0;
        const uint32_t nseg = subst_tpl_segments(seg_off_b.p, n_needles, s.needle, &s0);
        if (pbase.at(j + 1) - pbase.at(j) != 1 + nseg) { std::printf("FAIL count of span %llu\n", (unsigned long long)j); g_failed++; }
        for (uint32_t k = 0; k < nseg; k++) {
            const SubstPiece pc = subst_tpl_piece(segs_b.at(s0 + k), pool.size(), base + s.start, s.len);
            put(subst_tpl_seg_piece(pbase.at(j), h, k), pc.len, pc.src);
        }
    }
    for (uint32_t h = 0; h < n_hay; h++) {
        const uint64_t e0 = sp.offsets[h], e1 = sp.offsets[h + 1], hay_len = src_off[h + 1] - src_off[h];
        const uint64_t last_end = e1 > e0 ? sp.spans[e1 - 1].start + sp.spans[e1 - 1].len : 0;
        put(subst_tpl_gap_piece(pbase.at(e1), h), hay_len - last_end, src_off[h] + last_end);
    }
    for (uint64_t i = 0; i < P; i++)
        if (written.at(i) != 1) { std::printf("FAIL piece %llu written %u times\n", (unsigned long long)i, written.at(i)); g_failed++; }
    // launch_scan64 over the lengths; k_subst_compact's out_offsets; the gather as a plain copy per piece
    Block<uint64_t> dst_at(P + 1);
    { uint64_t run = 0; for (uint64_t i = 0; i <= P; i++) { dst_at.at(i) = run; run += lens.at(i); } }
    const uint64_t total = dst_at.at(P);
    std::vector<uint64_t> out_off(n_hay + 1);
    for (uint32_t h = 0; h <= n_hay; h++) out_off[h] = dst_at.at(subst_tpl_gap_piece(pbase.at(sp.offsets[h]), h));
    Block<uint8_t> out(total);
    for (uint64_t i = 0; i < P; i++) {
        g_pieces++;
        if (!live.at(i)) { g_empty++; continue; }
        const bool repl = (src_at.at(i) & kSubstRepl) != 0;
        const uint64_t at = src_at.at(i) & ~kSubstRepl;
        if (repl) g_literal++; else g_match++;
        for (uint64_t b = 0; b < lens.at(i); b++) out.at(dst_at.at(i) + b) = repl ? pool_b.at(at + b) : text_b.at(at + b);
    }
    // the definition
    std::vector<amh::Text> texts;
    for (const std::string& s : hays) texts.emplace_back(s);
    const std::vector<std::string> exp = amh::substituteTemplates(sp, texts, tpl);
    uint64_t at = 0;
    for (uint32_t h = 0; h < n_hay; h++) {
        if (out_off[h] != at) { std::printf("FAIL out_off[%u] = %llu, expected %llu\n", h, (unsigned long long)out_off[h], (unsigned long long)at); g_failed++; }
        if (at + exp[h].size() > total || std::memcmp(out.p + at, exp[h].data(), exp[h].size()) != 0) { std::printf("FAIL bytes of haystack %u\n", h); g_failed++; }
        at += exp[h].size();
    }
    if (at != total || out_off[n_hay] != total) { std::printf("FAIL total %llu, expected %llu\n", (unsigned long long)total, (unsigned long long)at); g_failed++; }
}

}  // namespace

int main()
{
    std::mt19937_64 rng(20261);
    // the arithmetic at its edges: a handle the table does not know owns its gap only; a literal that would leave the pool and an unknown kind are empty pieces
    const uint64_t off[3] = {0, 2, 2};
    uint64_t first = 9;
    if (subst_tpl_count(off, 2, 0) != 3 || subst_tpl_count(off, 2, 1) != 1 || subst_tpl_count(off, 2, 2) != 1 || subst_tpl_segments(off, 2, 7, &first) != 0 || first != 0) { std::printf("FAIL count\n"); g_failed++; }
    const SubstPiece m = subst_tpl_piece(SubstSeg{0, 0, kSegMatch}, 10, 1234, 7), l = subst_tpl_piece(SubstSeg{3, 7, kSegLiteral}, 10, 1234, 9);
    if (m.len != 7 || m.src != 1234 || l.len != 7 || l.src != (kSubstRepl | 3)) { std::printf("FAIL piece\n"); g_failed++; }
    if (subst_tpl_piece(SubstSeg{4, 7, kSegLiteral}, 10, 0, 9).len != 0 || subst_tpl_piece(SubstSeg{11, 0, kSegLiteral}, 10, 0, 9).len != 0 || subst_tpl_piece(SubstSeg{0, 1, 5}, 10, 0, 9).len != 0) { std::printf("FAIL piece bounds\n"); g_failed++; }
    if (subst_tpl_gap_piece(10, 3) != 13 || subst_tpl_seg_piece(10, 3, 0) != 14 || subst_tpl_seg_piece(10, 3, 63) != 77) { std::printf("FAIL piece index\n"); g_failed++; }
    for (int rep = 0; rep < 300; rep++) run(rng, 1 + (uint32_t)(rng() % 9), (uint32_t)(rng() % 7), rep % 3 == 0);
    run(rng, 4, 0, true);                                                   // no haystack
    if (g_pieces == 0 || g_empty == 0 || g_match == 0 || g_literal == 0 || g_adjacent == 0 || g_full == 0 || g_none == 0) {
        std::printf("FAIL coverage: pieces %ld empty %ld match %ld literal %ld adjacent %ld full %ld none %ld\n", g_pieces, g_empty, g_match, g_literal, g_adjacent, g_full, g_none);
        g_failed++;
    }
    if (g_failed) { std::printf("%d FAILED\n", g_failed); return 1; }
    std::printf("subst_templates: all checks passed (%ld pieces, %ld empty, %ld from the text, %ld from the pool, %ld adjacent MATCHes, %ld templates of 64 segments)\n",
                g_pieces, g_empty, g_match, g_literal, g_adjacent, g_full);
    return 0;
}
