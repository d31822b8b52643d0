// spans.hpp -- host mirror of am_spans (include/am.h "match spans"): the sequential definition.  A fold step `Match pos v` of runWithCase (reference:
// src/Data/Text/AhoCorasick/Automaton.hs:442-553) becomes the span makeMatch gives it (src/Data/Text/AhoCorasick/Replacer.hs:264-274) with the needle's own lengths;
// all of them in fold order, or the leftmost-longest non-overlapping selection.  spansFold takes the fold steps as they are and touches no device.
#pragma once
#include <algorithm>
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

// wordBytes (nullable: no class): only the whole-word spans are rows, and the leftmost-longest selection runs over those -- filter, then select
inline Spans spansFold(CaseSensitivity cs, bool leftmostLongest, const std::vector<FoldStep>& steps, const std::vector<Text>& texts,
                       const std::vector<uint32_t>& lenBytes, const std::vector<uint32_t>& lenCodePoints, const uint8_t* wordBytes = nullptr)
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

// ... straight from the fold steps, with an optional word class: substitute over spansFold(cs, leftmost-longest, ..., wordBytes)
inline std::vector<std::string> substitute(CaseSensitivity cs, const std::vector<FoldStep>& steps, const std::vector<Text>& texts, const std::vector<uint32_t>& lenBytes,
                                           const std::vector<uint32_t>& lenCodePoints, const std::vector<std::string>& replacements, const uint8_t* wordBytes = nullptr)
{
    return substitute(spansFold(cs, true, steps, texts, lenBytes, lenCodePoints, wordBytes), texts, replacements);
}

}  // namespace alfred_margaret
