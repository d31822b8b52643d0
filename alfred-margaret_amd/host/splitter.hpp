// splitter.hpp -- host mirror of Data.Text.AhoCorasick.Splitter (reference:
// src/Data/Text/AhoCorasick/Splitter.hs): split on a single separator with a 1-needle automaton.
//   build :64-67, split :84-85, splitIgnoreCase :96-97, splitReverse :100-107,
//   splitReverseIgnoreCase :112-121, Accum / stepAccum / finalizeAccum :128-170.
// The match positions come from libam (GPU).  splitBatch folds the records on the host with the reference's stepAccum (the host mirror of the fold);
// splitBatchFragments / splitBatchDevice leave the fold to the device too (am_split, csrc/am_split.hip) and receive (start, length) per fragment.
#pragma once
#include <algorithm>
#include <mutex>

#include "automaton.hpp"

namespace alfred_margaret {

class Splitter {
public:
    struct Unit0 {};
    explicit Splitter(std::string sep) : separator_(std::move(sep))
    {
        std::vector<std::pair<Text, Unit0>> nv{{Text(separator_), Unit0{}}};
        automaton_ = alfred_margaret::build(nv);                     // Splitter.hs:66  Aho.build [(sep, ())]
    }
    Splitter(const Splitter&) = delete;                              // (the device handle below points at this object's automaton)
    Splitter& operator=(const Splitter&) = delete;

    // the am_splitter* behind this Splitter (made on first use): the separator's length in bytes (:105) and in code points (:117)
    const am_splitter* device() const
    {
        std::lock_guard<std::mutex> lk(mu_);
        if (!device_) {
            am_splitter* raw = nullptr;
            amCheck(am_splitter_create(automaton_.device.get(), (uint32_t)separator_.size(), (uint32_t)utf8::lengthCodePoints(Text(separator_)), &raw));
            device_.reset(raw, am_splitter_destroy);
        }
        return device_.get();
    }

    // Splitter.hs:84-85 / :96-97 with the fold on the device: the fragments of every text as (start, length) in code units, in forward order
    struct Fragments { std::vector<uint64_t> offsets; std::vector<am_fragment> fragments; };      // text i: fragments[offsets[i] .. offsets[i + 1])
    Fragments splitBatchFragments(const std::vector<Text>& ts, bool ignoreCase) const
    {
        std::vector<am_slice> slices(ts.size());
        for (size_t i = 0; i < ts.size(); i++) slices[i] = am_slice{ts[i].data, ts[i].off, ts[i].len};
        am_fragments* raw = nullptr;
        amCheck(am_split(device(), ignoreCase ? AM_IGNORE_CASE : AM_CASE_SENSITIVE, slices.data(), slices.size(), &raw));
        std::unique_ptr<am_fragments, void (*)(am_fragments*)> guard(raw, am_fragments_free);
        const uint64_t n = am_fragments_size(raw);
        const uint64_t* offs = am_fragments_offsets(raw);
        const am_fragment* data = am_fragments_data(raw);
        if (!offs || !data) throw AmError(AM_ERR_HIP, am_last_error());
        return Fragments{std::vector<uint64_t>(offs, offs + ts.size() + 1), std::vector<am_fragment>(data, data + n)};
    }
    // ... and the strings built from them: what splitBatch returns
    std::vector<std::vector<std::string>> splitBatchDevice(const std::vector<std::string>& texts, bool ignoreCase) const
    {
        std::vector<Text> ts; ts.reserve(texts.size());
        for (auto& t : texts) ts.emplace_back(t);
        const Fragments fr = splitBatchFragments(ts, ignoreCase);
        std::vector<std::vector<std::string>> out(texts.size());
        for (size_t i = 0; i < texts.size(); i++) {
            out[i].reserve((size_t)(fr.offsets[i + 1] - fr.offsets[i]));
            for (uint64_t k = fr.offsets[i]; k < fr.offsets[i + 1]; k++) out[i].emplace_back(texts[i], (size_t)fr.fragments[k].start, (size_t)fr.fragments[k].len);
        }
        return out;
    }
    const std::string& separator() const { return separator_; }

    // Splitter.hs:84-85 / :96-97, for a batch: fragments of every haystack in order
    std::vector<std::vector<std::string>> splitBatch(const std::vector<std::string>& texts, bool ignoreCase) const
    {
        struct Accum { std::vector<std::string> result; size_t fragmentStart; const std::string* hay; };   // Splitter.hs:128-136
        // case sensitive: separator length in bytes (:105); ignore case: in code points (:118)
        const size_t sepBytes = separator_.size(), sepCps = utf8::lengthCodePoints(Text(separator_));
        auto step = [&](Accum acc, const Match<Unit0>& m) {                                                   // stepAccum :158-170
            const size_t newFragmentStart = m.matchPos;
            const size_t sepStart = ignoreCase ? utf8::skipCodePointsBackwards(Text(*acc.hay), newFragmentStart - 1, sepCps - 1)
                                               : newFragmentStart - sepBytes;
            if (sepStart >= acc.fragmentStart) {
                acc.result.emplace_back(*acc.hay, acc.fragmentStart, sepStart - acc.fragmentStart);
                acc.fragmentStart = newFragmentStart;
            }
            return Next<Accum>::Step(std::move(acc));
        };
        std::vector<Text> ts; ts.reserve(texts.size());
        for (auto& t : texts) ts.emplace_back(t);
        // one accumulator per haystack: the seed cannot carry the haystack pointer, so fold per record group
        std::vector<am_slice> slices(ts.size());
        for (size_t i = 0; i < ts.size(); i++) slices[i] = am_slice{ts[i].data, ts[i].off, ts[i].len};
        am_matches* ms = nullptr;
        amCheck(am_run(automaton_.device.get(), ignoreCase ? AM_IGNORE_CASE : AM_CASE_SENSITIVE, slices.data(), slices.size(), &ms));
        std::unique_ptr<am_matches, void (*)(am_matches*)> guard(ms, am_matches_free);
        const uint64_t n = am_matches_size(ms);
        const am_match* recs = am_matches_data(ms);
        if (n && !recs) throw AmError(AM_ERR_HIP, am_last_error());
        std::vector<Accum> accs(texts.size());
        for (size_t i = 0; i < texts.size(); i++) accs[i] = Accum{{}, 0, &texts[i]};                         // zeroAccum :150-151
        for (uint64_t i = 0; i < n;) {
            uint64_t j = i;
            while (j < n && recs[j].haystack == recs[i].haystack) j++;
            foldRecords(accs[recs[i].haystack], step, automaton_, recs + i, j - i);
            i = j;
        }
        std::vector<std::vector<std::string>> out(texts.size());
        for (size_t i = 0; i < texts.size(); i++) {                                                          // finalizeAccum :141-146
            accs[i].result.emplace_back(texts[i], accs[i].fragmentStart, std::string::npos);
            out[i] = std::move(accs[i].result);
        }
        return out;
    }
    std::vector<std::string> split(const std::string& text) const { return splitBatch({text}, false)[0]; }
    std::vector<std::string> splitIgnoreCase(const std::string& text) const { return splitBatch({text}, true)[0]; }
    // Splitter.hs:100-107 / :112-121: the fragments last-first (what the fold accumulates before `split` reverses it)
    std::vector<std::string> splitReverse(const std::string& text) const { auto v = split(text); std::reverse(v.begin(), v.end()); return v; }
    std::vector<std::string> splitReverseIgnoreCase(const std::string& text) const { auto v = splitIgnoreCase(text); std::reverse(v.begin(), v.end()); return v; }
    const AcMachine<Unit0>& automaton() const { return automaton_; }       // Splitter.hs:71-72

private:
    std::string separator_;
    AcMachine<Unit0> automaton_;
    mutable std::mutex mu_;
    mutable std::shared_ptr<am_splitter> device_;
};

}  // namespace alfred_margaret
