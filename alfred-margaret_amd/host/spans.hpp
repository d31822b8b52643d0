// spans.hpp -- host mirror of am_spans (include/am.h "match spans"): the sequential definition.  A fold step `Match pos v` of runWithCase (reference:
// src/Data/Text/AhoCorasick/Automaton.hs:442-553) becomes the span makeMatch gives it (src/Data/Text/AhoCorasick/Replacer.hs:264-274) with the needle's own lengths;
// all of them in fold order, or the leftmost-longest non-overlapping selection.  spansFold takes the fold steps as they are and touches no device.
#pragma once
#include <algorithm>
#include <cstring>
#include <optional>
#include <string>

#include "automaton.hpp"

namespace alfred_margaret {

struct FoldStep { uint32_t haystack; uint64_t matchPos; uint32_t value; };      // a triple of amh_run_list: fold order, haystacks ascending

struct Spans {
    std::vector<uint64_t> offsets;                          // texts.size() + 1
    std::vector<am_span> spans;                             // haystack i: [offsets[i], offsets[i + 1])
};

// makeMatch: where the match of a needle with these lengths that ends at pos starts (clamped to 0 where the reference calls `error`)
inline uint64_t spanStart(CaseSensitivity cs, const Text& hay, uint64_t pos, uint32_t lenBytes, uint32_t lenCodePoints)
{
    if (lenBytes == 0) return pos;
    if (cs == CaseSensitivity::CaseSensitive) return pos >= lenBytes ? pos - lenBytes : 0;
    if (pos == 0 || pos > hay.len) return 0;
    try { return utf8::skipCodePointsBackwards(hay, (size_t)pos - 1, lenCodePoints - 1); } catch (const std::out_of_range&) { return 0; }
}

// the whole-word rule of include/am.h "whole words": both neighbours of [start, start + len) inside THIS haystack are no word bytes (or do not exist); it does not
// look at the span's own bytes.  wordBytes: 256 flags, non-zero = word byte
inline bool wholeWord(const Text& hay, uint64_t start, uint64_t len, const uint8_t* wordBytes)
{
    if (start > hay.len || len > hay.len - start) return false;
    if (start > 0 && wordBytes[hay.begin()[start - 1]]) return false;
    if (start + len < hay.len && wordBytes[hay.begin()[start + len]]) return false;
    return true;
}

// the default class: 0-9 A-Z a-z _ and every byte from 0x80 on (am_word_bytes_default)
inline void defaultWordBytes(uint8_t out[256])
{
    for (unsigned b = 0; b < 256; b++) out[b] = ((b >= '0' && b <= '9') || (b >= 'A' && b <= 'Z') || (b >= 'a' && b <= 'z') || b == '_' || b >= 0x80) ? 1 : 0;
}

// the exact-case rule of include/am.h "exact case": a handle may carry a spelling, and a span of it is a row only where len == |spelling| and the haystack spells it
// so, byte for byte.  The definition as it stands: the span comes from spanStart, no shortcut.
using ExactSpellings = std::vector<std::optional<std::string>>;      // one entry per value handle (shorter: the handles beyond have none)

inline bool exactCase(const Text& hay, uint64_t start, uint64_t len, const std::optional<std::string>& spelling)
{
    if (!spelling) return true;
    if (start > hay.len || len > hay.len - start) return false;
    return len == spelling->size() && (len == 0 || std::memcmp(hay.begin() + start, spelling->data(), (size_t)len) == 0);
}

// wordBytes (nullable: no class): only the whole-word spans are rows, and the leftmost-longest selection runs over those -- filter, then select.  exact (nullable:
// no spelling): the exact-case rule, applied where the whole-word rule is; with both, both must hold
inline Spans spansFold(CaseSensitivity cs, bool leftmostLongest, const std::vector<FoldStep>& steps, const std::vector<Text>& texts,
                       const std::vector<uint32_t>& lenBytes, const std::vector<uint32_t>& lenCodePoints, const uint8_t* wordBytes = nullptr,
                       const ExactSpellings* exact = nullptr)
{
    if (lenBytes.size() != lenCodePoints.size()) throw AmError(AM_ERR_INVALID, "spansFold: the two length arrays differ in size");
    const size_t nValues = lenBytes.size();
    Spans out;
    out.offsets.assign(texts.size() + 1, 0);
    size_t k = 0;
    std::vector<am_span> all;
    for (size_t h = 0; h < texts.size(); h++) {
        out.offsets[h] = out.spans.size();
        all.clear();
        for (; k < steps.size() && steps[k].haystack == h; k++) {
            const uint32_t v = steps[k].value;
            if (v >= nValues) continue;                     // the am_needle_ids convention: skipped
            const uint64_t start = spanStart(cs, texts[h], steps[k].matchPos, lenBytes[v], lenCodePoints[v]);
            const uint64_t len = steps[k].matchPos >= start ? steps[k].matchPos - start : 0;
            if (exact && v < exact->size() && !exactCase(texts[h], start, len, (*exact)[v])) continue;
            if (wordBytes && !wholeWord(texts[h], start, len, wordBytes)) continue;
            all.push_back(am_span{start, len, (uint32_t)h, v});
        }
        if (!leftmostLongest) { out.spans.insert(out.spans.end(), all.begin(), all.end()); continue; }
        // smallest start >= cursor, then the largest len, then the smallest handle: in that order the first span at or after the cursor is the one to take
        std::sort(all.begin(), all.end(), [](const am_span& a, const am_span& b) {
            if (a.start != b.start) return a.start < b.start;
            if (a.len != b.len) return a.len > b.len;
            return a.needle < b.needle;
        });
        uint64_t cursor = 0;
        for (const am_span& s : all)
            if (s.len > 0 && s.start >= cursor) { out.spans.push_back(s); cursor = s.start + s.len; }
    }
    if (k != steps.size()) throw AmError(AM_ERR_INVALID, "spansFold: the fold steps are not grouped by ascending haystack below texts.size()");
    out.offsets[texts.size()] = out.spans.size();
    return out;
}

// substitute (include/am.h "substitute"): `replace` (src/Data/Text/AhoCorasick/Replacer.hs:163-180) applied to the leftmost-longest spans of spansFold, sequentially:
// out_i = hay[0, s_1) ++ repl[v_1] ++ hay[s_1 + l_1, s_2) ++ ... ++ repl[v_k] ++ hay[s_k + l_k, len_i).  Replacements are bytes and are never scanned.
inline std::vector<std::string> substitute(const Spans& spans, const std::vector<Text>& texts, const std::vector<std::string>& replacements)
{
    if (spans.offsets.size() != texts.size() + 1) throw AmError(AM_ERR_INVALID, "substitute: the spans are not those of these texts");
    std::vector<std::string> out(texts.size());
    for (size_t h = 0; h < texts.size(); h++) {
        const Text& hay = texts[h];
        std::string& o = out[h];
        uint64_t cursor = 0;
        for (uint64_t k = spans.offsets[h]; k < spans.offsets[h + 1]; k++) {
            const am_span& s = spans.spans.at((size_t)k);
            if (s.start < cursor || s.start + s.len > hay.len || s.needle >= replacements.size())
                throw AmError(AM_ERR_INVALID, "substitute: a span overlaps the one before it, leaves its haystack or has no replacement");
            if (s.start > cursor) o.append(reinterpret_cast<const char*>(hay.begin()) + cursor, (size_t)(s.start - cursor));
            o.append(replacements[s.needle]);
            cursor = s.start + s.len;
        }
        if (hay.len > cursor) o.append(reinterpret_cast<const char*>(hay.begin()) + cursor, (size_t)(hay.len - cursor));
    }
    return out;
}

// ... straight from the fold steps, with an optional word class and optional spellings: substitute over spansFold(cs, leftmost-longest, ..., wordBytes, exact)
inline std::vector<std::string> substitute(CaseSensitivity cs, const std::vector<FoldStep>& steps, const std::vector<Text>& texts, const std::vector<uint32_t>& lenBytes,
                                           const std::vector<uint32_t>& lenCodePoints, const std::vector<std::string>& replacements, const uint8_t* wordBytes = nullptr,
                                           const ExactSpellings* exact = nullptr)
{
    return substitute(spansFold(cs, true, steps, texts, lenBytes, lenCodePoints, wordBytes, exact), texts, replacements);
}
inline std::vector<std::string> substituteFold(CaseSensitivity cs, const std::vector<FoldStep>& steps, const std::vector<Text>& texts, const std::vector<uint32_t>& lenBytes,
                                               const std::vector<uint32_t>& lenCodePoints, const std::vector<std::string>& replacements, const uint8_t* wordBytes = nullptr,
                                               const ExactSpellings* exact = nullptr)
{
    return substitute(cs, steps, texts, lenBytes, lenCodePoints, replacements, wordBytes, exact);
}

// substitute templates (include/am.h "substitute templates"): the same splice with T(v, m) in the place of repl[v] -- the segments of template v in order, a literal's
// bytes or the matched bytes m themselves.  The sequential definition: a plain loop, on purpose not built on the piece arithmetic the kernels use.
struct TemplateSegment { bool match; std::string literal; };            // match: the span's own bytes (the literal is not looked at)
using Template = std::vector<TemplateSegment>;

inline std::vector<std::string> substituteTemplates(const Spans& spans, const std::vector<Text>& texts, const std::vector<Template>& templates)
{
    if (spans.offsets.size() != texts.size() + 1) throw AmError(AM_ERR_INVALID, "substituteTemplates: the spans are not those of these texts");
    std::vector<std::string> out(texts.size());
    for (size_t h = 0; h < texts.size(); h++) {
        const Text& hay = texts[h];
        const char* bytes = reinterpret_cast<const char*>(hay.begin());
        std::string& o = out[h];
        uint64_t cursor = 0;
        for (uint64_t k = spans.offsets[h]; k < spans.offsets[h + 1]; k++) {
            const am_span& s = spans.spans.at((size_t)k);
            if (s.start < cursor || s.start + s.len > hay.len || s.needle >= templates.size())
                throw AmError(AM_ERR_INVALID, "substituteTemplates: a span overlaps the one before it, leaves its haystack or has no template");
            if (s.start > cursor) o.append(bytes + cursor, (size_t)(s.start - cursor));
            for (const TemplateSegment& g : templates[s.needle]) {
                if (g.match) { if (s.len) o.append(bytes + s.start, (size_t)s.len); }
                else o.append(g.literal);
            }
            cursor = s.start + s.len;
        }
        if (hay.len > cursor) o.append(bytes + cursor, (size_t)(hay.len - cursor));
    }
    return out;
}

// extract (include/am.h "extract"): every span with up to `before` code points of its haystack in front of it and up to `after` behind it, as fragments of the
// haystack; one per span, or -- merged -- the union of the windows per haystack as disjoint ascending pieces.  The sequential definition, a byte at a time.
struct Extracted {
    std::vector<uint64_t> offsets;                          // texts.size() + 1
    std::vector<am_fragment> fragments;                     // haystack i: [offsets[i], offsets[i + 1])
};

inline bool isStartByte(uint8_t b) { return (b & 0xC0) != 0x80; }

// the window [ws, we) of the span (s, l) of hay: ws = the before-th START byte among the indices < s, counted leftwards (fewer: 0; before == 0: s), we = the
// after-th START byte among the indices > s + l, counted rightwards (fewer: hay.len; after == 0: s + l)
inline am_fragment extractWindow(const Text& hay, uint64_t s, uint64_t l, uint32_t before, uint32_t after)
{
    if (s > hay.len || l > hay.len - s) throw AmError(AM_ERR_INVALID, "extractFold: a span leaves its haystack");
    const uint8_t* p = hay.begin();
    const uint64_t e = s + l;
    uint64_t ws = s, we = e;
    if (before > 0) {
        ws = 0;
        uint32_t seen = 0;
        for (uint64_t i = s; i-- > 0;)
            if (isStartByte(p[i]) && ++seen == before) { ws = i; break; }
    }
    if (after > 0) {
        we = hay.len;
        uint32_t seen = 0;
        for (uint64_t i = e + 1; i < hay.len; i++)
            if (isStartByte(p[i]) && ++seen == after) { we = i; break; }
    }
    return am_fragment{ws, we - ws};
}

// merged: the rows of a haystack must ascend by start and must not overlap (an AM_SPANS_LEFTMOST_LONGEST result); window i joins the piece of window i - 1 of the
// same haystack iff ws_i <= we_{i-1}
inline Extracted extractFold(const Spans& spans, const std::vector<Text>& texts, uint32_t before, uint32_t after, bool merged)
{
    if (spans.offsets.size() != texts.size() + 1) throw AmError(AM_ERR_INVALID, "extractFold: the spans are not those of these texts");
    Extracted out;
    out.offsets.assign(texts.size() + 1, 0);
    for (size_t h = 0; h < texts.size(); h++) {
        out.offsets[h] = out.fragments.size();
        uint64_t cursor = 0;
        bool open = false;                                  // a piece of THIS haystack is open: the first span of a haystack always opens one
        for (uint64_t k = spans.offsets[h]; k < spans.offsets[h + 1]; k++) {
            const am_span& s = spans.spans.at((size_t)k);
            const am_fragment w = extractWindow(texts[h], s.start, s.len, before, after);
            if (!merged) { out.fragments.push_back(w); continue; }
            if (s.start < cursor) throw AmError(AM_ERR_INVALID, "extractFold: merged windows need spans that ascend and do not overlap");
            cursor = s.start + s.len;
            am_fragment* last = open ? &out.fragments.back() : nullptr;
            if (last && w.start <= last->start + last->len) last->len = w.start + w.len - last->start;      // (we is non-decreasing over such rows)
            else out.fragments.push_back(w);
            open = true;
        }
    }
    out.offsets[texts.size()] = out.fragments.size();
    return out;
}

}  // namespace alfred_margaret
