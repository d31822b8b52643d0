// am_device.h -- interface between the host-side translation units (am_host.h) and the kernels: the launchers of every .hip file and the structs they take
#pragma once
#include <hip/hip_runtime.h>

#include "am_chain.h"
#include "am_image.h"
#include "am_subst_tpl.h"

namespace am {
namespace dev {

constexpr int kModeCount = 0;   // unit_counts[u] = records of unit u; optional per-haystack value counts; total values
constexpr int kModeEmit = 1;    // write records at unit_offsets[u]
constexpr int kModeAny = 2;     // flags[haystack] = 1 if anything matches
constexpr int kModeIds = 3;     // Searcher.containsAll: the needle ids of everything that matches into the haystack's bitmap row; flags[haystack] = 1 when the row is full
                                // (k_sf only: a flag mode like kModeAny -- a flagged haystack is not looked at any further)

// (Record, the 16-byte match record in HBM: am_rows.h)
struct ScanOut {
    // general (AC) kernel, two passes: count pass fills unit_counts[u], emit pass writes at unit_offsets[u]
    uint32_t* unit_counts;
    const uint64_t* unit_offsets;
    Record* records;
    // suffix-filter kernel, single pass: records go to 64-record blocks taken from a pool with one
    // atomic per block; the blocks of a unit form a linked list (block_next); k_permute then copies
    // every unit's list to its final place (unit_offsets = exclusive scan of unit_counts)
    Record* pool;
    uint32_t* block_next;
    uint32_t* pool_ctrl;          // [0] next free block (keeps counting past n_blocks = blocks needed), [1] overflow flag
    uint32_t* unit_first;         // first block of each unit (kNone: none)
    uint32_t* unit_slots;         // record SLOTS in each unit's chain: its records (unit_counts) + the slots of parked walkers that found nothing
                                  // (state == kNone; k_permute drops them)
    uint32_t wq_iters;            // set by launch_sf: trie steps a resolve batch takes before it parks the walkers that are not done (2)
    uint32_t wq_cap;              // set by launch_sf: walker-queue entries per wavefront in LDS (0: the filter leaves no room)
    uint32_t n_blocks;
    uint32_t unit_chunks;         // 1-KiB chunks per unit
    uint32_t* next_unit;          // zeroed before the launch: wavefronts draw their second and later units from it (null: fixed stride)
    // all kernels
    uint64_t* hay_counts;         // count mode, may be null
    uint64_t* total_values;       // count mode
    uint8_t* flags;               // any mode; ids mode: the haystack's row is full
    // ids mode (containsAll): machineValues in flat form = the needle ids a state reports; one row of ids_words 32-bit words per haystack;
    // ids_missing[h] = ids of haystack h not seen yet (starts at the number of needles: the bit that brings it to 0 raises flags[h])
    const uint64_t* ids_vals_off; const uint32_t* ids_vals; uint32_t* ids_bits; uint32_t* ids_missing; uint32_t ids_words, ids_n;
    uint32_t two_always;          // set by launch_sf: 0.  k_sf<ILP = 1> reads it (non-zero: every probe round takes two candidates per lane).  Like wq_iters a constant
                                  // that stays an argument: folding it into the kernel changes the code of those instantiations (registers, spills), which is a kernel change to measure
    uint64_t* dbg;                // AM_SF_TRACE only: per-phase cycle sums
};

constexpr uint32_t kPoolBlock = 64;   // records per pool block (1 KiB)
constexpr uint32_t kSfBlockGrant = 32; // pool blocks a k_sf wavefront takes per atomic
// blocks that may stay unused in the wavefronts' grants: one grant per wavefront that can be resident (<= 32 per CU), never more than units
// (wavefronts launched = 16 per workgroup, one workgroup per CU -- two when the filter is small -- and never more workgroups than 16-unit groups)
inline uint64_t pool_grant_slack(int n_cu, uint64_t n_units, bool two_per_cu)
{
    uint64_t w = (uint64_t)n_cu * (two_per_cu ? 32u : 16u);
    const uint64_t need = (n_units + 15u) / 16u * 16u;
    if (w > need) w = need;
    return w * kSfBlockGrant;
}

// z0 / z1 (nullable): up to two arrays of n0 / n1 dwords that the same launch clears
hipError_t launch_hidx(const BatchView& b, uint32_t* hidx, uint64_t n_entries, hipStream_t st, uint32_t* z0 = nullptr, uint64_t n0 = 0, uint32_t* z1 = nullptr, uint64_t n1 = 0);
uint64_t sf_chunks(const BatchView& b);
uint32_t sf_unit_chunks(const BatchView& b, int n_cu);
hipError_t launch_permute(const ScanOut& o, const uint64_t* unit_offsets, Record* out, uint64_t n_units, hipStream_t st);
uint64_t ac_units(const AcView& a, const BatchView& b);
size_t sf_lds_bytes(const SfView& s);
// scan2: the image's derived two-word filter on the device (am_image.h scan2_mask), or null; the launches that can filter with it get it as their SfView::scan_bloom
hipError_t launch_sf(bool ic, int mode, const SfView& s, const BatchView& b, const ScanOut& o, int n_cu, hipStream_t st, const uint32_t* scan2 = nullptr);
uint32_t take_sf_last_variant();      // the k_sf instantiation launch_sf launched last in this process (am_debug_sf_last_variant's word), cleared by the read; 0: none since
hipError_t launch_ac(bool ic, int mode, const AcView& a, const BatchView& b, const ScanOut& o, hipStream_t st);
// table-walk kernel (am_dfa.hip): same two-pass protocol as the general kernel (count -> scan -> emit), unit = one lane's DfaView::chunk bytes
uint64_t dfa_units(const DfaView& d, const BatchView& b);
bool dfa_usable(const DfaView& d);      // on the current device: offsets fit, the LDS attribute could be raised (checked once per device)
// k_dfa's launch geometry, decided ONCE per entry-point call (dfa_launch_shape, on the current device) and handed to every launch of that call: the walk, its retries
// and k_dfa_place agree on it whatever AM_DFA_TUNE or the device's probe (am_dfa.hip dfa_resident_sets) would say a moment later
struct DfaLaunch {
    int n_cu; uint32_t workgroups, per_cu;        // the grid; workgroups per CU (2, or 1 with all of the LDS)
    uint32_t lds_rows, hot_rows, lds_n1, lds_n2;  // what a workgroup keeps in LDS: rows (room for / read from LDS: AM_DFA_TUNE bits 8-23 cap the latter), single-entry and two-entry records (bit 24: none)
    uint32_t walk; bool place_wide;               // AM_DFA_TUNE bits 0-3 (the walk variant) and 25 (k_dfa_place's table of seen states with 8-byte entries)
};
DfaLaunch dfa_launch_shape(const DfaView& d, const BatchView& b, int n_cu);
hipError_t launch_dfa(int mode, const DfaView& d, const BatchView& b, const ScanOut& o, const DfaLaunch& s, hipStream_t st);
// records in ONE walk: 8-byte tokens into ScanOut::pool (superblocks; ScanOut::block_next = 2 x n_blocks words: their fill counts, zeroed before the launch, then their
// first groups; pool_ctrl[0] superblocks drawn, [1] pool exhausted; n_blocks = superblocks in the pool), unit_counts as in count mode; then scan(unit_counts) and launch_dfa_place
// an estimate of the needle ends per byte of a batch: n_samples lanes spread over the text walk len bytes each and add their count to *out (zeroed by the caller)
hipError_t launch_dfa_sample(const DfaView& d, const uint8_t* text, uint64_t total, uint32_t n_samples, uint32_t len, uint32_t* out, hipStream_t st);
bool dfa_tokens_ok(const DfaView& d);
uint64_t dfa_token_superblocks(uint64_t records, uint32_t n_waves /* 16 x DfaLaunch::workgroups */, uint64_t n_units);
uint64_t dfa_superblock_bytes();
hipError_t launch_dfa_tokens(const DfaView& d, const BatchView& b, const ScanOut& o, const DfaLaunch& s, hipStream_t st);
hipError_t launch_dfa_place(const DfaView& d, const BatchView& b, const ScanOut& o, uint32_t n_super, const uint64_t* unit_offsets, const DfaLaunch& s, uint32_t n_ref_states, Record* out, hipStream_t st);
hipError_t read_sf_phase_cycles(uint64_t* out5);
hipError_t read_sf_wave_records(uint64_t* out, size_t n_waves);
hipError_t scan_temp_bytes(uint64_t n, size_t* bytes);
hipError_t launch_scan(void* temp, size_t temp_bytes, const uint32_t* counts, uint64_t* offsets, uint64_t n, hipStream_t st);
hipError_t launch_offsets_rebase(const uint64_t* local /* nullable: zeros */, uint64_t n, uint64_t base, uint64_t* out, hipStream_t st);      // out[i] = base + local[i], i < n (am_scan.hip)

// ---- automata with the empty needle: dense pass over the suffix-filter kernel's records (am_dense.hip)
hipError_t launch_dense(bool ic, bool write, const AcView& a, const BatchView& b, const Record* sparse, const uint64_t* sparse_offsets, uint32_t unit_chunks,
                        uint64_t n_units, uint32_t* unit_totals, const uint64_t* out_offsets, Record* out, hipStream_t st);
hipError_t launch_records_reduce(const Record* recs, uint64_t n, const uint32_t* vlen, uint64_t* hay_counts, uint64_t* total, uint8_t* flags, hipStream_t st);
// one haystack scanned in ranges (am_run_range): out2 = {records with end_pos <= x0, records with end_pos <= x1}; end_pos += add
hipError_t launch_range_bounds(const Record* recs, uint64_t n, uint64_t x0, uint64_t x1, uint64_t* out2, hipStream_t st);
hipError_t launch_range_rebase(Record* recs, uint64_t n, uint64_t add, hipStream_t st);
hipError_t launch_hay_rebase(Record* recs, uint64_t n, uint32_t add, hipStream_t st);
hipError_t launch_spin(uint32_t workgroups, uint32_t threads, uint64_t cycles, uint32_t* out, hipStream_t st);      // am_debug_resident_waves

// ---- Replacer pass (am_replace.hip) ----------------------------------------------------------
// same layout as am_payload in include/am.h (Replacer.hs:59-70 Payload, replacement text as a slice of one blob)
struct RpPayload { int64_t priority; uint32_t len_bytes; uint32_t len_code_points; uint64_t repl_off; uint32_t repl_len; uint32_t reserved; };
// machineValues of the Replacer's automaton in CSR form: the list of state s is payloads[vals[vals_off[s] .. vals_off[s+1])]
// per state, 8 bytes: for the states that carry exactly ONE value (almost all of them) that value's priority and payload index, so that the fold
// reads one small entry -- the table of a 50k-needle automaton stays in L2 -- instead of walking state -> value list -> payload (three dependent
// loads); payload == kRpWalkList: several values (or a priority beyond 32 bits): walk the list
struct RpStateOne { int32_t priority; uint32_t payload; };
constexpr uint32_t kRpWalkList = 0xFFFFFFFFu;
struct RpTables { const uint64_t* vals_off; const uint32_t* vals; const RpPayload* payloads; const uint8_t* repl; int64_t min_priority; const RpStateOne* one; };
struct RpKept { uint64_t src_start, src_len, dst; };     // a match that survives removeOverlap; dst = where its replacement starts in the new text
constexpr uint32_t kRpActive = 0, kRpFinished = 1, kRpNothing = 2;
struct RpHay { uint64_t newlen; int64_t best; uint32_t status, nkept, payload, pad; };
struct RpFin { uint64_t off, len; uint32_t orig, status; };
struct RpRoute { uint64_t* len_next; uint64_t* len_fin; uint32_t* tiles; uint32_t* act; uint32_t* fin; };                       // per haystack, written by k_rp_pass
struct RpRouted { const uint64_t* off_next; const uint64_t* off_fin; const uint64_t* tile_off; const uint64_t* act_idx; const uint64_t* fin_idx; };   // their exclusive sums
constexpr uint64_t kRpTile = 16384;                      // bytes of new text per k_rp_splice workgroup

hipError_t launch_rp_ranges(const Record* recs, uint64_t n_rec, uint64_t* rec_first, const RpRoute& route, uint32_t n_act, hipStream_t st);
hipError_t launch_rp_ranges_dev(const Record* recs, const uint64_t* n_rec_dev, uint64_t* rec_first, const RpRoute& route, uint32_t n_act, hipStream_t st);
hipError_t launch_rp_totals(const RpRouted& rt, uint32_t n_act, const uint64_t* win_off, const uint64_t* woffs, uint64_t woffs_last, uint64_t* out10, hipStream_t st,
                            const uint64_t* extra8 = nullptr, const uint64_t* extra9 = nullptr, uint64_t seq = 0);      // out10[8], out10[9] = *extra8, *extra9 (0 when null); seq != 0: out10 is pinned host memory, out10[15] = seq last
// what k_rp_ranges (before the fold) and k_pt_count (after it) would write, done by k_rp_pass itself: one dispatch instead of three in the
// chain of a Replacer pass.  rec_first_w == nullptr: not fused (rec_first is read).
struct RpFused { uint64_t* rec_first_w; uint64_t n_rec; const uint64_t* n_rec_dev; const uint32_t* pc_cnt; uint32_t* need; uint32_t* nwin; };
hipError_t launch_rp_pass(bool ic, const RpTables& t, const uint8_t* text, const uint64_t* offsets, const Record* recs, const uint64_t* rec_first,
                          const int64_t* thr, uint64_t max_len, RpKept* kept, RpHay* hs, const RpRoute& route, uint32_t n_act, uint32_t keep_all, hipStream_t st,
                          const RpFused* fused = nullptr);
struct RpSelected { uint64_t start, len; uint32_t haystack, payload; };     // = am_prio_match in include/am.h
hipError_t launch_rp_gather(const RpHay* hs, const uint64_t* rec_first, const RpKept* kept, const uint64_t* out_off, RpSelected* out, int64_t* best_out,
                            uint32_t n_act, hipStream_t st);
hipError_t launch_rp_route(const RpHay* hs, const RpRouted& rt, const uint32_t* orig, uint32_t n_act, uint64_t* next_offsets, uint32_t* next_orig,
                           int64_t* next_thr, RpFin* fin, hipStream_t st);
hipError_t launch_rp_splice(const RpTables& t, const uint8_t* text, const uint64_t* offsets, const uint64_t* rec_first, const RpKept* kept,
                            const RpHay* hs, const RpRouted& rt, uint32_t n_act, uint64_t n_tiles, uint32_t* tile_hay /* n_tiles entries, scratch */,
                            uint8_t* text_next, uint8_t* text_fin, hipStream_t st);
// ---- folds over the records of a scan.  What every one of them reads: the sorted records and machineValues in flat form (am_needle_ids; host: records_in, am_host.h);
// the value list of a record is read through value_range / load_records (am_records.h), by k_mx_values (am_matrix.hip) alone with a loop of its own.
struct RecordsIn {
    const Record* recs; uint64_t n_rec;                     // the sorted records
    const uint64_t* vals_off; const uint32_t* vals; uint64_t n_states, n_values;      // entries of vals_off - 1 / of vals (index checks)
    uint32_t n_needles, n_hay;                              // handles >= n_needles are skipped by the folds that keep a table; n_hay bounds the records' haystack fields
};
// Searcher.containsAll on the records and the fold checksum (am_records.hip).  launch_idset: bit id of row (haystack - hay0) of `bits` (in.n_hay rows of `words` words)
// for every value id < in.n_needles of in.recs.  launch_fold_hash: per haystack h < in.n_hay the checksum and the count of EVERY value of records [rec_first[h], rec_first[h + 1])
hipError_t launch_idset(const RecordsIn& in, uint32_t hay0, uint32_t words, uint32_t* bits, hipStream_t st);
hipError_t launch_fold_hash(const RecordsIn& in, const uint64_t* rec_first, uint64_t* hash_out, uint64_t* count_out, hipStream_t st);
hipError_t launch_idset_all(const uint32_t* bits, uint32_t words, uint32_t n_needles, uint32_t n_hay, uint8_t* flags, hipStream_t st);
// per-needle match counts (am_hist.hip): counts[id] += occurrences of id < in.n_needles in the value lists of in.recs; a persistent grid sized from n_cu.
// trace (nullable; the instrumented instantiation): [0] adds the workgroups' LDS tables absorbed, [1] adds that went to HBM one by one (slot conflicts), [2] the flushes' adds
hipError_t launch_needle_hist(const RecordsIn& in, uint64_t* counts, uint64_t* trace, uint32_t flush_tiles /* 0: the kernel's own interval */, int n_cu, hipStream_t st);
// the term-document matrix (am_matrix.hip): per-haystack needle counts of a group of n_rows = in.n_hay haystacks whose sorted records are in.recs, haystack indices
// relative to the group.  In the order of the calls: *total += lengths of the records' value lists; the (haystack, needle) keys combined into the open-addressing table keys / cnts
// (cap slots, keys all ones and cnts zero before; cap > the group's distinct keys) with row_entries[h] = entries of row h (n_rows + 1, zero before); then, with
// offsets = exclusive sum of row_entries and n_entries = offsets[n_rows], the live slots into tmp in arrival order (haystack = hay0 + h; row_entries ends at zero again);
// rows of up to kMxWaveRow entries ordered by needle into `out`, the longer ones listed (list: n_rows words, ctr: two words, zero before) and ordered by launch_mx_rows_lds
// (up to kMxLdsRow entries) and launch_mx_rows_wide (beyond: grid = mx_wide_grid(...) workgroups, each with ceil(n_needles / 32) words of `bits`, zero before, and of `pre`).
struct alignas(16) NeedleCount { uint64_t count; uint32_t needle; uint32_t haystack; };      // = am_needle_count in include/am.h
constexpr uint32_t kMxWaveRow = 64, kMxLdsRow = 2048;
void mx_limits(uint32_t* out4);                             // wavefront row limit, LDS row capacity, slots of a workgroup's LDS table, records between two of its flushes
hipError_t launch_mx_values(const RecordsIn& in, uint64_t* total, int n_cu, hipStream_t st);
hipError_t launch_mx_combine(const RecordsIn& in, uint64_t* keys, uint64_t* cnts, uint64_t cap, uint32_t* row_entries, int n_cu, hipStream_t st);
hipError_t launch_mx_scatter(const uint64_t* keys, const uint64_t* cnts, uint64_t cap, const uint64_t* offsets, uint32_t* row_entries, uint32_t n_rows, uint32_t hay0,
                             NeedleCount* tmp, uint64_t n_entries, int n_cu, hipStream_t st);
hipError_t launch_mx_rows(const NeedleCount* tmp, const uint64_t* offsets, uint32_t n_rows, uint64_t n_entries, NeedleCount* out, uint32_t* list, uint32_t* ctr, hipStream_t st);
hipError_t launch_mx_rows_lds(const NeedleCount* tmp, const uint64_t* offsets, uint32_t n_rows, uint64_t n_entries, const uint32_t* list, const uint32_t* ctr,
                              NeedleCount* out, int n_cu, hipStream_t st);
uint32_t mx_wide_grid(uint32_t n_rows, uint64_t n_entries, uint32_t n_needles, int n_cu);      // 0: no row can be that long
hipError_t launch_mx_rows_wide(const NeedleCount* tmp, const uint64_t* offsets, uint32_t n_rows, uint64_t n_entries, const uint32_t* list, const uint32_t* ctr,
                               uint32_t n_needles, uint32_t* bits, uint32_t* pre, uint32_t grid, NeedleCount* out, hipStream_t st);
// Splitter's fold over the sorted records of a one-needle automaton, and the gather of the fragments into a batch (am_split.hip)
struct Fragment { uint64_t start, len; };                   // = am_fragment in include/am.h: code units, relative to the haystack
struct SplitIn { const Record* recs; uint64_t n_rec; const uint8_t* text; const uint64_t* offsets; uint64_t total; uint32_t n_hay, sep_bytes, sep_cps; };
// start[i] = sepStart of record i (Splitter.hs:105-107 / :117-121), head[i] = first of its haystack or starting at or after the end of record i - 1, kept = head;
// kept has n_rec + 1 entries (the last one 0: the scan's trailing element)
hipError_t launch_split_start(bool ic, const SplitIn& in, uint64_t* start, uint8_t* head, uint32_t* kept, hipStream_t st);
// the greedy selection inside the chains between heads: select_chains (am_fold.h) over a SplitChain (am_chain.h).  With kidx = exclusive sum of kept (n_rec + 1), rec_first = first record of every haystack (n_hay + 1): frag_off (n_hay + 1) and the n_frag = kidx[n_rec] + n_hay fragments
hipError_t launch_split_emit(const SplitIn& in, const uint64_t* start, const uint32_t* kept, const uint64_t* kidx, const uint64_t* rec_first, uint64_t* frag_off,
                             Fragment* frags, uint64_t n_frag, hipStream_t st);
// am_batch_from_fragments: lens (n_frag + 1, the last one 0) and the source position of every fragment; then, with dst_off = exclusive sum of lens, the bytes
hipError_t launch_split_sources(const Fragment* frags, uint64_t n_frag, const uint64_t* frag_off, const uint64_t* src_offsets, uint64_t n_hay, uint64_t src_total,
                                uint64_t* lens, uint64_t* src_at, hipStream_t st);
hipError_t launch_split_gather(const uint8_t* src, uint64_t src_total, const uint64_t* src_at, const uint64_t* dst_off, uint64_t n_frag, uint64_t total, uint8_t* dst,
                               int n_cu, hipStream_t st);
// match spans (am_spans.hip): every fold step `Match pos v` with v < n_needles as (start, len, haystack, needle), all of them or the leftmost-longest selection
struct Span { uint64_t start, len; uint32_t haystack, needle; };      // = am_span in include/am.h
constexpr uint32_t kWordClassWords = 8;                     // a word class: 256 flags, bit b & 31 of word b >> 5
struct ExactRef { uint32_t at16, len; };                    // the spelling of a handle: `len` bytes at 16 * at16 of the pool (am_cased.h); len == 0: none
struct SpansIn : RecordsIn {                             // the sorted records of the batch and machineValues, and what only spans need:
    const uint32_t* len_bytes; const uint32_t* len_cps;     // the needles' own lengths (am_span_table)
    const uint8_t* text; const uint64_t* offsets; uint64_t total;
    const uint32_t* words;                                  // the table's word class: 256 flags in 8 dwords (am_words.h); null: no class, every span is kept
    const ExactRef* exact; const uint8_t* exact_pool;       // the table's spellings (include/am.h "exact case"): one ExactRef per handle and the pool; null: no spelling
};
constexpr uint64_t kSpansMaxTile = 2048;                    // candidates per workgroup of the prefix maximum
constexpr uint32_t kSpThreads = 256;                        // lanes per workgroup of the prefix maximum; k_spans_tiles_max takes the tile maxima in sweeps of as many
// cnt[i] = values < n_needles of record i (n_rec + 1 entries, the last one 0); then, with voff = exclusive sum of cnt and n_span = voff[n_rec], the spans in fold order.
// With in.words both passes keep the whole-word spans only (ic decides the starts, so the count pass needs it as well)
hipError_t launch_spans_count(bool ic, const SpansIn& in, uint32_t* cnt, hipStream_t st);
hipError_t launch_spans_write(bool ic, const SpansIn& in, const uint64_t* voff, Span* spans, uint64_t n_span, hipStream_t st);
// AM_SPANS_ALL: span_off[h] = voff[rec_first[h]] (n_hay + 1)
hipError_t launch_spans_offsets(const uint64_t* rec_first, const uint64_t* voff, uint64_t n_rec, uint32_t n_hay, uint64_t* span_off, hipStream_t st);
// AM_SPANS_LEFTMOST_LONGEST, in global byte positions g = offsets[haystack] + start.  In the order of the calls: bit g of `bits` (n_words = ceil(total / 32) words, zero
// before) for every span with len > 0, pc[w] = popcount(bits[w]) (n_words + 1, the last one 0); with rank = exclusive sum of pc and n_cand = rank[n_words]:
// best[rank of g] = max(len << 32 | ~needle) (zero before); cand_g[k] = the k-th set bit; head / kept (kept: n_cand + 1, the last one 0) from the exclusive prefix
// maximum of the candidates' ends (tile_max: ceil((n_cand + 1) / kSpansMaxTile) words); select_chains (am_fold.h) over a SpansChain (am_chain.h) finishes kept; with
// kidx = exclusive sum of kept and n_out = kidx[n_cand]: the spans kept and span_off (n_hay + 1)
hipError_t launch_spans_mark(const Span* spans, uint64_t n_span, const SpansIn& in, uint32_t* bits, uint64_t n_words, hipStream_t st);
hipError_t launch_spans_popcount(const uint32_t* bits, uint64_t n_words, uint32_t* pc, hipStream_t st);
hipError_t launch_spans_best(const Span* spans, uint64_t n_span, const SpansIn& in, const uint32_t* bits, const uint64_t* rank, uint64_t n_words, uint64_t* best, uint64_t n_cand, hipStream_t st);
hipError_t launch_spans_candidates(const uint32_t* bits, const uint64_t* rank, uint64_t n_words, uint64_t* cand_g, uint64_t n_cand, hipStream_t st);
hipError_t launch_spans_heads(const uint64_t* cand_g, const uint64_t* best, uint64_t n_cand, uint64_t* tile_max, uint8_t* head, uint32_t* kept, hipStream_t st);
hipError_t launch_spans_emit(const uint64_t* cand_g, const uint64_t* best, const uint32_t* kept, const uint64_t* kidx, uint64_t n_cand, const SpansIn& in, Span* out, uint64_t n_out,
                             uint64_t* span_off, hipStream_t st);
// per-needle counts over the whole-word spans only (am_hist.hip, am_count_spans_by_needle*): counts[id] += the values id < in.n_needles of in.recs whose span the class
// in.words (not null) keeps: the bincount of the AM_SPANS_ALL rows of that table.  trace / flush_tiles / n_cu as launch_needle_hist
hipError_t launch_needle_hist_words(bool ic, const SpansIn& in, uint64_t* counts, uint64_t* trace, uint32_t flush_tiles, int n_cu, hipStream_t st);
// substitute (am_subst.hip): the leftmost-longest spans of a batch spliced into a new text.  P = 2 * n_span + n_hay pieces: span j of haystack h owns 2j + h (the gap
// before it) and 2j + h + 1 (its replacement), 2 * span_off[h + 1] + h is the tail of h.  kSubstRepl (am_subst_tpl.h) tags a piece's source as an offset into the
// replacement pool instead of the batch text
struct SubstIn {
    const Span* spans; uint64_t n_span; const uint64_t* span_off;       // an AM_SPANS_LEFTMOST_LONGEST result of the batch below
    const uint64_t* src_off; uint64_t src_total; uint32_t n_hay, n_needles;
    const uint64_t* repl_off; uint64_t pool_bytes;           // replacement of handle v: pool[repl_off[v], repl_off[v + 1])
};
void subst_geometry(uint32_t* group_bytes, uint32_t* tile_bytes);      // k_subst_gather's store group and tile
// lens / src_at / live: P + 1 entries each, zero before (the last ones stay 0: the scans' trailing element); then, with dst_at = exclusive sum of lens (total = dst_at[P])
// and cidx = exclusive sum of live (n_live = cidx[P]): the live pieces as cdst / csrc (n_live + 1 entries, the last one the sentinel `total`) and out_off (n_hay + 1);
// then the bytes (dst: readable and writable to round_up(total, 16))
hipError_t launch_subst_pieces(const SubstIn& in, uint64_t* lens, uint64_t* src_at, uint32_t* live, hipStream_t st);
hipError_t launch_subst_compact(const uint64_t* src_at, const uint32_t* live, const uint64_t* dst_at, const uint64_t* cidx, uint64_t n_pieces, uint64_t* cdst, uint64_t* csrc,
                                uint64_t n_live, const uint64_t* span_off, const uint64_t* pbase, uint64_t n_span, uint64_t n_hay, uint64_t* out_off, hipStream_t st);
// a table of templates (am_subst_tpl.h): cnt[j] = 1 + the segments of span j's template (n_span + 1 entries, the last one 0); with pbase = exclusive sum of cnt
// (launch_scan) there are P = pbase[n_span] + n_hay pieces, and launch_subst_tpl_pieces writes lens / src_at / live as launch_subst_pieces does for 2 * n_span + n_hay.
// launch_subst_compact takes pbase for out_off (null: the fixed plan)
struct SubstTpl { const uint64_t* seg_off; const SubstSeg* segs; uint64_t n_seg; };      // template of handle v: segs[seg_off[v], seg_off[v + 1])
hipError_t launch_subst_tpl_count(const SubstIn& in, const SubstTpl& tpl, uint32_t* cnt, hipStream_t st);
hipError_t launch_subst_tpl_pieces(const SubstIn& in, const SubstTpl& tpl, const uint64_t* pbase, uint64_t n_pieces, uint64_t* lens, uint64_t* src_at, uint32_t* live,
                                   hipStream_t st);
hipError_t launch_subst_gather(const uint8_t* text, uint64_t src_total, const uint8_t* pool, uint64_t pool_bytes, const uint64_t* cdst, const uint64_t* csrc, uint64_t n_live,
                               uint64_t total, uint8_t* dst, int n_cu, hipStream_t st);
// a select's predicate over the records (am_records.hip): flags[h] = 1 for every haystack that owns a (record, value < n_needles) pair whose span the table keeps
// (span_of, am_words.h): row h of AM_SPANS_ALL is not empty.  flags: in.n_hay bytes, zero before; in.words null: no class, IC is not looked at
hipError_t launch_hay_flags_spans(bool ic, const SpansIn& in, uint8_t* flags, hipStream_t st);
// select (am_select.hip): the haystacks of a batch that a predicate keeps, compacted by RUNS (maximal sequences of consecutive kept haystacks: contiguous in the source)
// n + 1 entries each, the last ones 0 (the scans' trailing element): keep[i] = (flags[i] != 0) != (invert != 0) (flags null: every flag is `constant`),
// run_head[i] = keep[i] && !(i > 0 && keep[i - 1]), klen[i] = keep[i] ? length of haystack i : 0
hipError_t launch_select_plan(const uint8_t* flags, uint32_t constant, uint32_t invert, const uint64_t* src_offsets, uint64_t n, uint64_t src_total, uint32_t* keep,
                              uint32_t* run_head, uint64_t* klen, hipStream_t st);
// with rank / run_rank / koff = the exclusive sums of keep / run_head / klen (n_kept = rank[n], n_runs = run_rank[n], total = koff[n]): indices[rank] = i and
// new_off[rank] = koff[i] for every kept haystack (new_off[n_kept] = total); per run its source position run_src = src_offsets[first] and its destination run_dst =
// koff[first] (run_dst[n_runs] = total: the closing entry launch_split_gather wants)
hipError_t launch_select_emit(const uint32_t* keep, const uint32_t* run_head, const uint64_t* rank, const uint64_t* run_rank, const uint64_t* koff, const uint64_t* src_offsets,
                              uint64_t n, uint64_t n_kept, uint64_t n_runs, uint32_t* indices, uint64_t* new_off, uint64_t* run_src, uint64_t* run_dst, hipStream_t st);
// extract (am_extract.hip): the window of every span -- the span with up to `before` / `after` code points of its own haystack around it -- relative to the haystack.
// frags given: AM_EXTRACT_EACH, frags[i] = the window of span i (ws / we unused).  frags null: ws[i] / we[i] for the two kernels below.
hipError_t launch_extract_windows(const Span* spans, uint64_t n_span, const uint8_t* text, const uint64_t* src_offsets, uint32_t n_hay, uint64_t total, uint32_t before,
                                  uint32_t after, Fragment* frags, uint64_t* ws, uint64_t* we, hipStream_t st);
// head[i] = span i opens a piece (the first of its haystack, or ws[i] > we[i - 1]); head has n_span + 1 entries (the last one 0: the sum's trailing element)
hipError_t launch_extract_heads(const Span* spans, uint64_t n_span, const uint64_t* ws, const uint64_t* we, uint32_t* head, hipStream_t st);
// with rank = the exclusive sum of head (n_pieces = rank[n_span]): frags[p] = [ws of the head of piece p, we of its last span), out_off[h] = rank[span_off[h]]
hipError_t launch_extract_emit(const uint32_t* head, const uint64_t* rank, const uint64_t* ws, const uint64_t* we, uint64_t n_span, uint64_t n_pieces, const uint64_t* span_off,
                               uint64_t n_hay, Fragment* frags, uint64_t* out_off, hipStream_t st);
// am_select_geometry: bytes of new text per workgroup of launch_split_gather (am_split.hip), elements per workgroup of launch_scan / a sweep of launch_scan_jobs (am_scan.hip)
uint32_t split_gather_tile_bytes();
uint32_t scan_tile_items();
// rule sets (am_rules.hip; the program view, the launch struct and the evaluator of one (row, program) pair: am_rules.h).  k_rules_eval: the slot rows of in.n_hay
// consecutive haystacks against the program, into their words of in.fired, their labels and in.counts (accumulating: cleared by the caller).  in.n_hay is a whole batch
// or a group that begins at a multiple of 64 haystacks (in.word0), so no word of `fired` is written twice.  A persistent grid sized from n_cu.
struct RulesEvalIn;
hipError_t launch_rules_eval(const RulesEvalIn& in, int n_cu, hipStream_t st);
// flags[h] = bit h of fired_row (one rule's row of `fired`), or -- fired_row null -- labels[h] == rule: the n_hay byte flags launch_select_plan takes
hipError_t launch_rule_flags(const uint64_t* fired_row, const uint32_t* labels, uint32_t rule, uint64_t n_hay, uint64_t hay_words, uint8_t* flags, hipStream_t st);
// am_rules_geometry: haystacks per workgroup step of k_rules_eval, the widest slot row (32-bit words) it stages in LDS, the rules whose counts it keeps in LDS
void rules_geometry(uint32_t* tile_haystacks, uint32_t* lds_slot_words, uint32_t* lds_rules);
// scores (am_score.hip; score_key / topk_pick, the select's state and k_score's output struct: am_score.h).  k_score: score[c][h] += the weights of column c of the
// values id < in.n_needles of in.recs, per haystack h of the records -- a segmented sum over the sorted records, at most one 64-bit add per column and run of equal
// haystacks a wavefront holds; out.scores is accumulating (cleared by the caller) and out.stride >= in.n_hay.  in.words given: only the values whose span the class
// keeps (ic decides the starts), otherwise only the RecordsIn part of `in` is looked at (and handed to the kernel).  A persistent grid sized from n_cu.
struct ScoreOut;
struct TopkState;
struct alignas(8) Scored { int64_t score; uint32_t haystack; uint32_t reserved; };      // = am_scored in include/am.h
hipError_t launch_score(bool ic, const SpansIn& in, const ScoreOut& out, int n_cu, hipStream_t st);
// the workspace of a top-k selection over n keys: the select's state, 256 words of histogram, tie / tie_rank of n + 1 entries each, and the exclusive sum's temporary
struct TopkWork { TopkState* state; uint64_t* hist; uint32_t* tie; uint64_t* tie_rank; void* scan_tmp; size_t scan_tmp_bytes; };
// the min(k, n) best scores of col[0, n) -- largest: (score descending, index ascending), else (score ascending, index ascending) -- for 1 <= k <= n: flags[i] (n
// bytes, nullable) and keep[i] (n + 1 words, the last one 0, nullable) = 1 for the winners.  Eight histogram passes and their picks, all on the device
hipError_t launch_topk_flags(const int64_t* col, uint64_t n, uint64_t k, bool largest, const TopkWork& w, uint8_t* flags, uint32_t* keep, hipStream_t st);
hipError_t launch_score_range(const int64_t* col, uint64_t n, int64_t lo, int64_t hi, uint8_t* flags, hipStream_t st);      // flags[i] = lo <= col[i] <= hi
// with pos = the exclusive sum of keep (n + 1): out[pos[i]] = {col[i], i} for every kept i; n_out = pos[n]
hipError_t launch_topk_gather(const int64_t* col, uint64_t n, const uint32_t* keep, const uint64_t* pos, Scored* out, uint64_t n_out, hipStream_t st);
// am_score_geometry: records per workgroup step of k_score (a wavefront owns a quarter of them, consecutive), keys per workgroup of the top-k histogram
void score_geometry(uint32_t* tile_records, uint32_t* topk_block_items);
// proximity (am_near.hip; the pick, the bitmap arithmetic and the launch struct: am_near.h) over the n_span rows of an AM_SPANS_LEFTMOST_LONGEST result, in this order:
// the group bitmaps in.bits (every word written), their word links in.prev_nz / in.next_nz, then per span the mask and the number of the queries that hit (in.hit_mask,
// in.hit_count; in.fired is accumulating: cleared by the caller), and -- with in.pos = the exclusive sum of in.hit_count over n_span + 1 entries -- the pairs at their
// places, in.out_off and in.counts (accumulating).  launch_near_emit runs for n_span == 0 too (it writes out_off).  Persistent grids sized from n_cu.
struct NearIn;
hipError_t launch_near_bits(const NearIn& in, int n_cu, hipStream_t st);
hipError_t launch_near_words(const NearIn& in, hipStream_t st);
hipError_t launch_near_count(const NearIn& in, int n_cu, hipStream_t st);
hipError_t launch_near_emit(const NearIn& in, int n_cu, hipStream_t st);
// am_near_geometry: spans per workgroup step of the three span kernels (a sweep of k_near_words covers 4 x as many WORDS), spans per bitmap word
void near_geometry(uint32_t* tile_spans, uint32_t* word_spans);
// incremental re-scan between Replacer passes (am_replace.hip)
struct RpWin { uint64_t src_abs; uint64_t ws; uint32_t len; uint32_t own_lo; };   // window: bytes src_abs.. of the next text; ws = its start inside the haystack; records with end > own_lo are its own
hipError_t launch_rp_win_count(const RpHay* hs, uint32_t n_act, uint32_t* nwin, hipStream_t st);
hipError_t launch_rp_win_meta(const RpTables& t, const RpRouted& rt, const RpHay* hs, const uint64_t* rec_first,
                              const RpKept* kept, const uint64_t* win_off, uint32_t ov, RpWin* wins, uint32_t* wlen, uint32_t n_act, hipStream_t st, bool pt = false);
// piece table (am_replace.hip): the text of a haystack between passes as (source, logical start) pairs + a sentinel
struct RpPiece { uint64_t src; uint64_t lstart; };
constexpr uint64_t kPieceRepl = 1ull << 63;             // RpPiece::src: offset into the replacement blob instead of the batch text
// all passes of a haystack in one kernel (am_rploop.hip): every haystack owns two record lists, two piece lists, a kept list and a window scratch
struct RpLoopOut { uint64_t len; uint64_t pieces_at; uint32_t n_pieces, status, passes, pad; };      // pieces_at: index of the final list in pc_buf
struct RpLoop {
    RpTables t; SfView s;
    const uint8_t* text; const uint64_t* offsets; uint32_t n_hay, ov;
    const Record* recs0; const uint64_t* rec_first0;        // the first scan's sorted records and their range per haystack
    Record* rec_buf; const uint64_t* rec_base;              // haystack h: records [rec_base[h], rec_base[h + 1]), two halves
    RpPiece* pc_buf; const uint64_t* pc_base;               // the same for its piece lists
    RpKept* kept_buf;                                       // haystack h: from rec_base[h] / 2, half a record region long
    uint8_t* wtext; uint32_t wcap, pad;                     // haystack h: wcap bytes of window scratch; pad != 0: the instrumented instantiation
    uint64_t max_len;
    RpLoopOut* out;
    uint32_t* ctrl;                                         // [0] overflow, [1] passes (max), [2..3] window bytes scanned, [5] watchdog: the loop that ran out of time (100 +: in k_rp_lds), [6] the longest record list of the batch (k_rp_loop_caps), [7] haystacks k_rp_lds finished, [8..23] eight 64-bit phase sums of the instrumented instantiation
    uint32_t* redo;                                         // per haystack: 1 = k_rp_lds (LDS-resident lists, am_rplds.hip) gave it up, k_rp_loop runs it; null: k_rp_loop runs every haystack
    uint32_t h_first, pl_implicit;                          // the launch covers haystacks h_first + blockIdx.x (groups of a batch, one launch each); pl_implicit: every payload's
                                                            // priority is minus its index (Replacer.hs:100-104): k_rp_lds needs no payload column (am_rplds.hip, PLI)
};
hipError_t launch_rp_loop_caps(const uint64_t* rec_first, uint32_t n_hay, uint32_t* cap_r2, uint32_t* cap_p2, uint32_t* max_records /* atomic max, cleared by the caller */, hipStream_t st);
hipError_t launch_rp_loop(bool ic, const RpLoop& a, uint32_t n /* haystacks from a.h_first */, hipStream_t st);
hipError_t launch_rp_lds(bool ic, const RpLoop& a, uint32_t n /* haystacks from a.h_first */, hipStream_t st);
hipError_t launch_pt_init(const uint64_t* offsets, uint32_t n_act, RpPiece* pieces, uint64_t* pc_start, uint32_t* pc_cnt, hipStream_t st);
hipError_t launch_pt_count(const RpHay* hs, const uint32_t* pc_cnt, uint32_t n_act, uint32_t* need, uint32_t* nwin, hipStream_t st);
hipError_t launch_pt_build(const RpTables& t, const RpHay* hs, const uint64_t* rec_first, const RpKept* kept, const RpPiece* pieces, const uint64_t* pc_start,
                           const uint32_t* pc_cnt, const uint64_t* need_off, const RpRouted& rt, uint32_t n_act, RpPiece* out, uint64_t* next_start, uint32_t* next_cnt,
                           uint64_t* fin_start, uint32_t* fin_cnt, hipStream_t st);
hipError_t launch_pt_materialise(const RpPiece* pieces, const uint64_t* fin_start, const uint32_t* fin_cnt, const RpFin* fin, uint32_t n_fin, const uint8_t* text,
                                 const uint8_t* repl, uint8_t* text_fin, hipStream_t st);
hipError_t launch_pt_materialise_next(const RpPiece* pieces, const uint64_t* next_start, const uint32_t* next_cnt, const uint64_t* next_offsets, uint32_t n_next,
                                      const uint8_t* text, const uint8_t* repl, uint8_t* out, hipStream_t st);
hipError_t launch_pt_win_copy(const RpWin* wins, const uint64_t* woffs, const RpPiece* pieces, const uint64_t* next_start, const uint32_t* next_cnt, const uint8_t* text,
                              const uint8_t* repl, uint8_t* wtext, uint64_t n_win, uint64_t total_w, uint64_t padded, hipStream_t st);
hipError_t launch_rp_win_copy(const RpWin* wins, const uint64_t* woffs, const uint8_t* text_next, uint8_t* wtext, uint64_t n_win, hipStream_t st);
hipError_t launch_rp_merge(bool write, const Record* recs, const uint64_t* rec_first, const RpKept* kept, const RpHay* hs, const uint64_t* offsets, const RpRouted& rt,
                           const uint64_t* win_off, const RpWin* wins, const Record* wrecs, const uint64_t* wrec_first, uint32_t ov, uint32_t n_act,
                           uint32_t* mcount, const uint64_t* moff, Record* out, hipStream_t st);
// the record-parallel variant of the fold (few haystacks with very many matches), same outputs as launch_rp_pass
struct RpSel { uint64_t start, len; uint32_t haystack, pad; };
hipError_t launch_rpp_best(const RpTables& t, const Record* recs, uint64_t n_rec, const int64_t* thr, int64_t* best /* n_act + 1 */, uint32_t n_act, hipStream_t st);
hipError_t launch_rpp_select(bool ic, const RpTables& t, const uint8_t* text, const uint64_t* offsets, const Record* recs, uint64_t n_rec, const int64_t* best,
                             uint32_t* selflag, RpSel* cand, int64_t* delta_all, uint32_t* payload_of, hipStream_t st);
hipError_t launch_rpp_compact(const uint32_t* selflag, const uint64_t* sidx, const RpSel* cand, uint64_t n_rec, RpSel* sel, hipStream_t st);
hipError_t launch_rpp_overlaps(const RpSel* sel, const uint64_t* n_sel_dev, uint64_t bound, uint32_t* keep, hipStream_t st);
hipError_t launch_rpp_kflags(const RpSel* sel, const uint64_t* n_sel_dev, uint64_t bound, const uint32_t* keep, const RpTables& t, const uint32_t* payload_of,
                             uint32_t* kflag, uint64_t* kdelta, hipStream_t st);
hipError_t launch_rpp_finish(const RpTables& t, const RpSel* sel, const uint64_t* n_sel_dev, uint64_t bound, const uint32_t* kflag, const uint64_t* kidx,
                             const uint64_t* kdpre, const uint64_t* sidx, const uint64_t* offsets, const uint64_t* rec_first, const int64_t* best,
                             const int64_t* delta_all, const uint32_t* payload_of, uint64_t max_len, RpKept* kept, RpHay* hs, const RpRoute& route, uint32_t n_act,
                             hipStream_t st);
// several small exclusive sums in one launch (am_scan.hip): out[i] = sum of in[0..i), for i < n (+ *n_dev when given)
struct ScanJob { const uint32_t* in32; const uint64_t* in64; uint64_t* out; uint64_t n; const uint64_t* n_dev; };
struct ScanJobs { ScanJob j[6]; uint32_t n_jobs; };
hipError_t launch_scan_jobs(const ScanJobs& jobs, hipStream_t st);
hipError_t scan64_temp_bytes(uint64_t n, size_t* bytes);
hipError_t launch_scan64(void* temp, size_t temp_bytes, const uint64_t* in, uint64_t* out, uint64_t n, hipStream_t st);

}  // namespace dev
}  // namespace am
