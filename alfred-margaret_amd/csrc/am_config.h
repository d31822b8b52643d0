// am_config.h -- the library's test / measurement switches in ONE place.  None of them changes a result; they select between
// equivalent code paths (A/B measurements, tests that force a rarely taken path).  (That holds for every switch listed here, AM_SF_TRACE included: it only times.)
// Every switch is read from its environment
// variable ONCE, when the library first looks at any of them, and can be set afterwards with am_debug_set(name, value) (exported for
// the tests, not part of include/am.h).  A read is one relaxed atomic load: no getenv on any call path.
#pragma once
#include <atomic>
#include <cstdlib>
#include <cstring>
#include <mutex>

namespace am {
namespace cfg {

enum Key {
    kSfTrace,             // AM_SF_TRACE: the instrumented instantiation of k_sf sums its wavefronts' cycles per phase into a debug buffer (am_debug_sf_phase_cycles, tools/phase_timing.py)
    kSfPoolBlocks,        // AM_SF_POOL_BLOCKS: size of the record-block pool of the first attempt (tests force overflow + retry)
    kSfNoChildren,        // AM_SF_NO_CHILDREN: the flattener gives heavy depth-4 nodes no five-byte child entries (A/B; read when an image is flattened)
    kDfa,                 // AM_DFA: 0 = no automaton gets a DFA section / none is used; 1 = every automaton whose table fits gets one (read when an image is flattened); unset: dictionaries with heavy suffix nodes
    kDfaChunk,            // AM_DFA_CHUNK: bytes of the batch one lane of k_dfa owns (read when an image is flattened; default 2048)
    kDfaRarePermille,     // AM_DFA_RARE_PERMILLE: share of the edges (in thousandths; default 1) whose bytes may go without a column of the DFA table (tests: 300 makes most bytes rare)
    kDfaMinKiB,           // AM_DFA_MIN_KIB: batch size from which a dictionary's scans take the table walk by themselves (default 32 768: below, a unit's walk costs more than the filter's whole scan)
    kDfaTune,             // AM_DFA_TUNE: launch parameters of k_dfa for A/B measurements (am_dfa.hip dfa_launch_shape)
    kDfaNoChains,         // AM_DFA_NO_CHAINS: every state of the DFA section gets a dense row (A/B against the chain records; read when an image is flattened)
    kFlattenTrace,        // AM_FLATTEN_TRACE: the flattener prints its phases with their wall time on stderr
    kFlattenSerial,       // AM_FLATTEN_SERIAL: the flattener starts no task (tests: the images are the same byte for byte; am_automaton_create flattens IgnoreCase on first use)
    kNoIdsScan,           // AM_NO_IDS_SCAN: containsAll folds the records of a full scan (k_idset) instead of setting the id bits inside k_sf
    kRpFullScans, kRpPieces, kRpParallelFold, kRpGroups, kRpNoFuse, kRpNoSpin, kRpMatMain, kRpNoRangeReuse, kRpTrace,
    kRpLds,               // AM_RP_LDS: 0 = the one-kernel loop never keeps a haystack's lists in LDS (k_rp_loop alone, round 4's kernel); unset / 1: k_rp_lds first, k_rp_loop for what it gives up
    kRpLoop,              // AM_RP_LOOP: all passes of a haystack in one kernel (am_rploop.hip): 0 = never, 1 = whenever the replacer allows it; unset: many documents
    kRunSegments,         // AM_RUN_SEGMENTS: am_run on host slices in segments whose records come back while the next segment goes up: 0 = never (the call in one piece), k > 0 = always, in segments of k KiB (tests); unset: from 1 GiB on, 256-MiB segments
    kHistRecordsMiB,      // AM_HIST_RECORDS_MIB: MiB of match records am_count_by_needle* keeps in HBM at a time (tests: 1 = many groups of haystacks); unset: 1024
    kHistTrace,           // AM_HIST_TRACE: the instrumented instantiation of k_needle_hist counts the adds its LDS tables absorbed and the adds that went to HBM (am_debug_hist_adds, tests/measure/needle_counts.py)
    kHistFlushTiles,      // AM_HIST_FLUSH_TILES: tiles after which a workgroup of k_needle_hist flushes and clears its LDS counts (tests: 1 = after every tile); unset: 2048, the most that cannot wrap a counter
    kSplitChainLimit,     // AM_SPLIT_CHAIN_LIMIT: records the lane of a chain's head looks at in k_chain_walk (am_chain.h) before the chain is left to the pointer-doubling rounds (tests: 1 = the head looks at one record: chains of three records and more go to the rounds); unset: 32
    kSpansChainLimit,     // AM_SPANS_CHAIN_LIMIT: the same for the candidates of am_spans* in leftmost-longest mode; unset: 32
    kRulesRowsMiB,        // AM_RULES_ROWS_MIB: MiB of slot rows am_rules_eval_batch keeps in HBM at a time (tests: 0 = the smallest group, 64 haystacks); unset: 1024
    kCount
};

struct Table {
    std::atomic<long> v[kCount];
    std::once_flag once;
};
inline Table& table() { static Table t; return t; }
inline const char* name_of(int k)
{
    static const char* const names[kCount] = {"AM_SF_TRACE", "AM_SF_POOL_BLOCKS", "AM_SF_NO_CHILDREN", "AM_DFA", "AM_DFA_CHUNK", "AM_DFA_RARE_PERMILLE", "AM_DFA_MIN_KIB", "AM_DFA_TUNE", "AM_DFA_NO_CHAINS", "AM_FLATTEN_TRACE", "AM_FLATTEN_SERIAL", "AM_NO_IDS_SCAN",
                                              "AM_RP_FULL_SCANS", "AM_RP_PIECES", "AM_RP_PARALLEL_FOLD", "AM_RP_GROUPS", "AM_RP_NO_FUSE", "AM_RP_NO_SPIN",
                                              "AM_RP_MAT_MAIN", "AM_RP_NO_RANGE_REUSE", "AM_RP_TRACE", "AM_RP_LDS", "AM_RP_LOOP", "AM_RUN_SEGMENTS", "AM_HIST_RECORDS_MIB", "AM_HIST_TRACE", "AM_HIST_FLUSH_TILES", "AM_SPLIT_CHAIN_LIMIT", "AM_SPANS_CHAIN_LIMIT", "AM_RULES_ROWS_MIB"};
    return names[k];
}
constexpr long kUnset = -1;
inline void init()
{
    Table& t = table();
    std::call_once(t.once, [&t] {
        for (int k = 0; k < kCount; k++) {
            const char* e = std::getenv(name_of(k));
            t.v[k].store(e ? (*e ? std::atol(e) : 1L) : kUnset, std::memory_order_relaxed);
        }
    });
}
// the switch's value, or kUnset (-1)
inline long get(Key k) { init(); return table().v[k].load(std::memory_order_relaxed); }
inline bool on(Key k) { const long v = get(k); return v != kUnset && v != 0; }
inline bool set(const char* name, long value)
{
    init();
    for (int k = 0; k < kCount; k++) if (std::strcmp(name, name_of(k)) == 0) { table().v[k].store(value, std::memory_order_relaxed); return true; }
    return false;
}

}  // namespace cfg
}  // namespace am
