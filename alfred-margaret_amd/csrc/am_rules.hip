// am_rules.hip -- rule sets on the device (include/am.h "rule sets"): the slot rows a scan leaves in HBM -- one bitmap row per haystack, bit v = slot v was reported
// in it -- evaluated against a program in conjunctive normal form, into rule-major bitmaps (`fired`), first-rule-wins labels and per-rule counts.
//
// k_rules_eval: ONE LANE PER HAYSTACK, 64 consecutive haystacks per wavefront, so the ballot of "rule r fires" IS the uint64 word of fired[r] that covers the
// wavefront's haystacks: one 8-byte store per wavefront and rule, no atomics and no read-modify-write on `fired`.  A workgroup is four wavefronts and handles tiles of
// kRulesTile = 256 consecutive haystacks.  The rows are haystack-major in HBM (the scans write them that way); a tile's rows are loaded coalesced -- the tile is one
// contiguous piece of tile x words dwords -- and stored TRANSPOSED into LDS, lds[w * kRulesStride + t]: the program is wave-uniform, so every lane asks for the same
// word index w and a wavefront's read is 64 consecutive dwords, conflict-free.  kRulesStride = 257 (odd) keeps the transposing STORES off one bank as well: consecutive
// elements of a row go to consecutive banks.  Rows wider than kRulesLdsSlotWords words do not fit the budget and are read from HBM in place (STAGED = false): a lane
// reads its own row, the L1 / L2 absorb the repeated words.
// The program is read through wave-uniform indices (rule_fires, am_rules.h: its loops end on ballots), so the compiler is free to use scalar loads for it; a program of
// any size is read where it lies in HBM, never staged.  Everything is written with plain vector stores.
// labels: a running "first rule that fired" in a register, one coalesced 4-byte store per lane.  counts: popcount(ballot) per wavefront and rule, added into an LDS
// table of kRulesLdsRules 64-bit counters while the workgroup walks its tiles and flushed with one 64-bit global atomic per non-zero counter at the end; rules beyond
// the table add to HBM per wavefront.  Integer adds commute: the counts are exact and the same from run to run.
// LDS: at most 8 KiB of counters + 48 x 257 x 4 B = 48.2 KiB of rows = 56.2 KiB per workgroup, so two workgroups fit the 160 KiB of a CU with room to spare, and
// narrow rows (the common case: one word per 32 slots) leave room for eight and more.
//
// k_rule_flags: one rule's row of `fired` (or labels == rule) as the n_hay byte flags the select's compaction takes (am_select.cpp compact).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "am_bounds.h"
#include "am_device.h"
#include "am_rules.h"
#include "am_wave.h"

AM_BOUNDS_TU("am_rules.hip")

namespace am {
namespace dev {

namespace {

constexpr uint32_t kRulesTile = 256;                        // haystacks per workgroup step = threads per workgroup
constexpr uint32_t kRulesStride = kRulesTile + 1;           // dwords between two words of the transposed tile
constexpr uint32_t kRulesLdsSlotWords = 48;                 // widest row (in 32-slot words) that is staged in LDS
constexpr uint32_t kRulesLdsRules = 1024;                   // rules whose counts a workgroup keeps in LDS
constexpr uint32_t kRulesWave = 64;

template <bool STAGED>
__global__ void __launch_bounds__(kRulesTile) k_rules_eval(RulesEvalIn in)
{
    extern __shared__ __attribute__((aligned(16))) uint64_t rules_lds[];
    uint64_t* const cnt = rules_lds;                                     // [in.lds_rules]
    uint32_t* const tile_rows = (uint32_t*)(rules_lds + in.lds_rules);   // [in.words * kRulesStride] (STAGED)
    const uint32_t t = threadIdx.x, lane = t & (kRulesWave - 1);
    const uint32_t wv = (uint32_t)__builtin_amdgcn_readfirstlane((int)(t / kRulesWave));
    AM_BOUNDS(in.lds_rules <= kRulesLdsRules && in.lds_rules <= in.p.n_rules && (!STAGED || in.words <= kRulesLdsSlotWords));
    for (uint32_t r = t; r < in.lds_rules; r += kRulesTile) cnt[r] = 0;
    __syncthreads();
    for (uint64_t tile = blockIdx.x; tile < in.n_tiles; tile += gridDim.x) {
        const uint64_t tile_h0 = tile * kRulesTile;
        AM_BOUNDS(tile_h0 < in.n_hay);
        if (STAGED) {
            const uint32_t tile_n = (uint32_t)(in.n_hay - tile_h0 < kRulesTile ? in.n_hay - tile_h0 : kRulesTile);
            const uint32_t n_e = tile_n * in.words;
            const uint32_t* __restrict__ src = in.rows + tile_h0 * in.words;
            __syncthreads();                                             // (the last tile's readers have finished)
            for (uint32_t e = t; e < n_e; e += kRulesTile) {
                const uint32_t hh = e / in.words, w = e - hh * in.words;
                AM_BOUNDS(tile_h0 * in.words + e < in.n_hay * in.words && hh < kRulesTile && w < in.words);
                tile_rows[w * kRulesStride + hh] = src[e];
            }
            __syncthreads();
        }
        const uint64_t wave_h0 = tile_h0 + (uint64_t)wv * kRulesWave;
        if (wave_h0 >= in.n_hay) continue;                               // (wave-uniform; every wavefront of the workgroup walks the same tiles)
        const uint64_t h = wave_h0 + lane;
        const bool active = h < in.n_hay;
        const uint32_t* __restrict__ row = in.rows + h * in.words;       // (looked at by active lanes only)
        auto word = [&](uint32_t w) -> uint32_t {
            AM_BOUNDS(w < in.words);
            if (STAGED) return tile_rows[w * kRulesStride + t];          // (an idle lane reads a stale word of the tile: in bounds, never used)
            return active ? row[w] : 0u;
        };
        auto any = [](bool x) -> bool { return __ballot(x) != 0; };
        const uint64_t fw = in.word0 + wave_h0 / kRulesWave;
        AM_BOUNDS(fw < in.hay_words);
        uint32_t label = kRuleNone;
        for (uint32_t r = 0; r < in.p.n_rules; r++) {
            const bool f = rule_fires(in.p, r, active, word, any);
            const uint64_t m = __ballot(f);                              // (idle lanes are false: the bits beyond the batch are zero)
            if (lane == 0) in.fired[(uint64_t)r * in.hay_words + fw] = m;
            if (f && label == kRuleNone) label = r;
            if (m != 0 && lane == 0) {
                const unsigned long long k = (unsigned long long)__popcll(m);
                if (r < in.lds_rules) atomicAdd((unsigned long long*)&cnt[r], k);
                else atomicAdd((unsigned long long*)&in.counts[r], k);
            }
        }
        if (active) in.labels[h] = label;
    }
    __syncthreads();
    for (uint32_t r = t; r < in.lds_rules; r += kRulesTile) {
        const uint64_t k = cnt[r];
        if (k != 0) atomicAdd((unsigned long long*)&in.counts[r], (unsigned long long)k);
    }
}

// one lane per haystack
__global__ void __launch_bounds__(kRowThreads) k_rule_flags(const uint64_t* __restrict__ fired_row, const uint32_t* __restrict__ labels, uint32_t rule, uint64_t n_hay,
                                                           uint64_t hay_words, uint8_t* __restrict__ flags)
{
    const uint64_t h = global_row();
    if (h >= n_hay) return;
    AM_BOUNDS(h / 64 < hay_words);
    flags[h] = fired_row ? (uint8_t)((fired_row[h / 64] >> (h % 64)) & 1u) : (uint8_t)(labels[h] == rule ? 1 : 0);
}

}  // namespace

void rules_geometry(uint32_t* tile_haystacks, uint32_t* lds_slot_words, uint32_t* lds_rules)
{
    if (tile_haystacks) *tile_haystacks = kRulesTile;
    if (lds_slot_words) *lds_slot_words = kRulesLdsSlotWords;
    if (lds_rules) *lds_rules = kRulesLdsRules;
}

hipError_t launch_rules_eval(const RulesEvalIn& call, int n_cu, hipStream_t st)
{
    RulesEvalIn in = call;
    if (in.n_hay == 0) return hipSuccess;
    in.n_tiles = (in.n_hay + kRulesTile - 1) / kRulesTile;
    in.lds_rules = std::min(in.p.n_rules, kRulesLdsRules);
    const bool staged = in.words != 0 && in.words <= kRulesLdsSlotWords;
    const size_t lds = (size_t)in.lds_rules * 8 + (staged ? (size_t)in.words * kRulesStride * 4 : 0);
    const uint32_t grid = (uint32_t)std::min<uint64_t>(in.n_tiles, (uint64_t)std::max(n_cu, 1) * 8);
    if (staged) hipLaunchKernelGGL(k_rules_eval<true>, dim3(grid), dim3(kRulesTile), lds, st, in);
    else hipLaunchKernelGGL(k_rules_eval<false>, dim3(grid), dim3(kRulesTile), lds, st, in);
    return hipGetLastError();
}

hipError_t launch_rule_flags(const uint64_t* fired_row, const uint32_t* labels, uint32_t rule, uint64_t n_hay, uint64_t hay_words, uint8_t* flags, hipStream_t st)
{
    return launch_rows(k_rule_flags, n_hay, st, fired_row, labels, rule, n_hay, hay_words, flags);
}

}  // namespace dev
}  // namespace am
