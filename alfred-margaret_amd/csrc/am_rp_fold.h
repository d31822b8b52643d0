// am_rp_fold.h -- what the Replacer's kernels (am_replace.hip, am_rploop.hip, am_rplds.hip) share.  The reference's fold is stated HERE, once:
//   prependMatch   Replacer.hs:252-260   rp_best_in_values / rp_pick_in_values: a state's value list, first and second half
//   makeMatch      Replacer.hs:268-274   rp_skip_code_points_backwards: Utf8.hs:256-276 (am_wave.h) on the text a piece list describes
//   removeOverlap  Replacer.hs:191-198   rp_remove_overlap: one block of 64 matches in position order; rp_keep_block: the kept ones as RpKept entries
//   replace        Replacer.hs:163-180   rp_piece_fragments: what an old piece becomes; rp_splice_pieces: the next piece list; rp_gather: bytes of a list
// AM_HD marks what is free of lanes and runs on the host as well (tests/native/rp_fold_main.cpp, a plain g++ program).  am_device.h needs HIP, so such a program
// declares RpPayload, RpStateOne, RpTables, RpKept, RpPiece and kPieceRepl as am_device.h has them before it includes this header.
#pragma once
#include "am_wave.h"
#if defined(__HIPCC__)
#include "am_device.h"
#endif

namespace am {
namespace dev {

// ---- prependMatch over the value list of a state that carries several values
// first half (:255-258): the best priority below the threshold
AM_HD void rp_best_in_values(const RpTables& t, uint32_t state, int64_t threshold, int64_t& best)
{
    for (uint64_t k = t.vals_off[state], ke = t.vals_off[state + 1]; k < ke; k++) {
        const int64_t p = t.payloads[t.vals[k]].priority;
        if (p < threshold && p > best) best = p;
    }
}
// second half: the value of the list that carries `best` (priorities are distinct: at most one does)
AM_HD void rp_pick_in_values(const RpTables& t, uint32_t state, int64_t best, bool& sel, uint32_t& payload)
{
    for (uint64_t k = t.vals_off[state], ke = t.vals_off[state + 1]; k < ke; k++) {
        const uint32_t v = t.vals[k];
        if (t.payloads[v].priority == best) { sel = true; payload = v; }
    }
}

// ---- piece lists: P[0 .. n) = {source, logical start}, P[n] = the sentinel (logical start = the text's length)
AM_HD const uint8_t* rp_piece_base(uint64_t src, const uint8_t* text, const uint8_t* repl) { return (src & kPieceRepl) ? repl + (src & ~kPieceRepl) : text + src; }

// the last piece that starts at or before pos (n >= 1; piece 0 starts at 0)
AM_HD uint32_t rp_piece_at(const RpPiece* P, uint32_t n, uint64_t pos)
{
    uint32_t lo = 0, hi = n;
    while (hi - lo > 1) { const uint32_t mid = (lo + hi) >> 1; if (P[mid].lstart <= pos) lo = mid; else hi = mid; }
    return lo;
}

// makeMatch of an IgnoreCase replacer on the text a piece list describes (end_pos >= 1; n = the match's code points - 1): the walk's byte source is a cursor
// into the list that only moves backwards (the bytes of a match almost always lie in one piece)
AM_HD uint64_t rp_skip_code_points_backwards(const RpPiece* P, uint32_t np, const uint8_t* text, const uint8_t* repl, uint64_t end_pos, uint32_t n)
{
    uint32_t pi = rp_piece_at(P, np, end_pos - 1);
    uint64_t ls = P[pi].lstart, src = P[pi].src;
    return skip_code_points_backwards_by([&](uint64_t pos) -> uint32_t {
        while (pos < ls) { pi--; ls = P[pi].lstart; src = P[pi].src; }      // (pieces may be empty: a loop)
        return rp_piece_base(src, text, repl)[pos - ls];
    }, end_pos, n);
}

// replace on a piece list.  Old piece i = old text [ls, le).  The kept matches K[0 .. nk) (sorted, disjoint) cut it into fragments; a fragment that starts at old
// position x lies, in the new text, at x + (sum of the length changes of the matches before it) = K[j].dst + repl_len + (x - end of K[j]) for the last match j
// before x.  The replacement of match j (repl_src: its tagged source; every kept match of a pass has the same one) is emitted by the piece that contains the
// match's first byte.  f(src, new_pos) for every entry piece i becomes, in order.
template <class F>
AM_HD void rp_piece_fragments(const RpPiece* P, uint32_t i, const RpKept* K, uint32_t nk, uint64_t repl_len, uint64_t repl_src, F&& f)
{
    const uint64_t ls = P[i].lstart, le = P[i + 1].lstart;
    if (le == ls) return;
    uint32_t ja = 0, jb = nk;                             // span: the matches j in [ja, jb) are those that end after the piece's start and start before its end
    while (ja < jb) { const uint32_t mid = (ja + jb) >> 1; if (K[mid].src_start + K[mid].src_len <= ls) ja = mid + 1; else jb = mid; }
    while (jb < nk && K[jb].src_start < le) jb++;
    // new position of old position x when it is not inside a match: after the last match that ends at or before x
    auto new_pos = [&](uint64_t xx, uint32_t jprev_plus1) -> uint64_t {
        if (jprev_plus1 == 0) return xx;
        const RpKept k = K[jprev_plus1 - 1];
        return k.dst + repl_len + (xx - (k.src_start + k.src_len));
    };
    uint64_t x = ls;                                      // old position where the next fragment would start
    uint32_t jp = ja;                                     // matches [0, jp) end at or before x
    for (uint32_t j = ja; j < jb; j++) {
        const RpKept k = K[j];
        if (k.src_start > x) f(P[i].src + (x - ls), new_pos(x, jp));                              // fragment before the match
        if (k.src_start >= ls && repl_len) f(repl_src, k.dst);                                     // the match starts in this piece: its replacement
        x = k.src_start + k.src_len;
        jp = j + 1;
        if (x >= le) break;
    }
    if (x < le) f(P[i].src + (x - ls), new_pos(x, jp));
}

#if defined(__HIPCC__)
// ---- removeOverlap over one block of 64 matches in position order (lane = match, sel: the lane holds one): keep a match iff it starts at or after the end of
// the last kept one.  last_end is uniform and carried from block to block.  Pos: uint64_t, or uint32_t in k_rp_lds.
template <class Pos>
__device__ __forceinline__ bool rp_remove_overlap(bool sel, Pos start, Pos len, Pos& last_end, int lane)
{
    uint64_t pending = __ballot(sel);
    bool keep = false;
    while (pending) {
        const uint64_t ok = __ballot(sel && start >= last_end) & pending;
        if (!ok) break;
        const int l = __ffsll((unsigned long long)ok) - 1;
        if (lane == l) keep = true;
        last_end = wave_read_lane((Pos)(start + len), l);
        pending &= l == 63 ? 0ull : ~((2ull << l) - 1ull);
    }
    return keep;
}

// the kept matches of a block go to K[nkept ..) with where their replacement starts in the new text (delta: replacement - match of the lane's match; delta_kept:
// the sum over the matches kept so far); nkept and delta_kept are uniform
__device__ __forceinline__ void rp_keep_block(bool keep, uint64_t start, uint64_t len, int64_t delta, RpKept* __restrict__ K, uint32_t& nkept, int64_t& delta_kept, int lane)
{
    const uint64_t keepmask = __ballot(keep);
    if (!keepmask) return;
    const int64_t kd = keep ? delta : 0;
    const int64_t incl = (int64_t)wave_inclusive_sum_u64((uint64_t)kd, (uint32_t)lane);
    if (keep) {
        const uint32_t rank = __popcll(keepmask & ((1ull << lane) - 1ull));
        RpKept e; e.src_start = start; e.src_len = len; e.dst = (uint64_t)((int64_t)start + delta_kept + (incl - kd));
        K[nkept + rank] = e;
    }
    delta_kept += (int64_t)wave_read_lane((uint64_t)incl, 63);
    nkept += __popcll(keepmask);
}

// the next piece list Q of a haystack from P[0 .. n) and the pass's kept matches, one wavefront: 64 pieces per round, lane = piece within the round -- count,
// prefix over the lanes, write; rounds follow each other in order.  Returns the entries written (the caller adds the sentinel).  go_on(): asked before every
// round, false ends the sweep (k_rp_loop's watchdog).
template <class GoOn>
__device__ __forceinline__ uint32_t rp_splice_pieces(const RpPiece* __restrict__ P, uint32_t n, const RpKept* __restrict__ K, uint32_t nk, uint64_t repl_len, uint64_t repl_src,
                                                     RpPiece* __restrict__ Q, int lane, GoOn go_on)
{
    uint32_t nq = 0;
    for (uint32_t r0 = 0; r0 < n && go_on(); r0 += 64) {
        const uint32_t i = r0 + lane;
        uint32_t c = 0;
        if (i < n) rp_piece_fragments(P, i, K, nk, repl_len, repl_src, [&](uint64_t, uint64_t) { c++; });
        const uint32_t incl = wave_inclusive_sum(c, (uint32_t)lane);
        uint32_t at = nq + incl - c;
        if (i < n) rp_piece_fragments(P, i, K, nk, repl_len, repl_src, [&](uint64_t src, uint64_t pos) { Q[at++] = RpPiece{src, pos}; });
        nq += wave_last_lane(incl);
    }
    return nq;
}

// bytes [lo, lo + len) of a piece list into dst, one wavefront.  first(): the index of a piece that starts at or before lo, found the caller's way; go_on(): asked
// before every piece that holds bytes, false ends the copy (k_rp_loop's watchdog).
template <class First, class GoOn>
__device__ __forceinline__ void rp_gather(const RpPiece* __restrict__ P, uint32_t n, const uint8_t* __restrict__ text, const uint8_t* __restrict__ repl,
                                          uint64_t lo, uint64_t len, uint8_t* __restrict__ dst, int lane, First first, GoOn go_on)
{
    if (len == 0) return;
    uint64_t pos = lo;
    const uint64_t end = lo + len;
    for (uint64_t i = first(); pos < end && i < n; i++) {
        const uint64_t ps = P[i].lstart, pn = P[i + 1].lstart, pe = pn < end ? pn : end;
        if (pe <= pos) continue;                                         // (an empty piece)
        if (!go_on()) return;
        const uint8_t* from = rp_piece_base(P[i].src, text, repl) + (pos - ps);
        uint8_t* to = dst + (pos - lo);
        for (uint64_t x = lane; x < pe - pos; x += 64) to[x] = from[x];
        pos = pe;
    }
}
#endif  // __HIPCC__

}  // namespace dev
}  // namespace am
