/*
 * am.h -- C ABI of libam.so, the MI355X-native drop-in for the hot path of
 * channable/alfred-margaret's Data.Text.AhoCorasick.Automaton.
 *
 * The reference is a pure Haskell library with no FFI layer of its own on this path; its only
 * precedent for a C boundary is benchmark/rust-ffi (app/Main.hs:28-52: `foreign import ccall
 * unsafe "perform_ac"`, slices passed as {ptr, off, len}, pinned byte arrays, callee borrows).
 * This header keeps that slice convention.  Each entry point names the reference function whose
 * body it replaces (paths relative to the reference repository root); INTEGRATION.md shows the
 * `foreign import ccall` stubs a maintainer would add.
 *
 * Division of labour (unchanged semantics):
 *   Haskell keeps   build (Automaton.hs:176-200)  -> state numbering, value lists, value order
 *                   the fold function f, Done/Step (Automaton.hs:398,522-534)
 *   libam replaces  the body of runWithCase (Automaton.hs:442-534): decode, lower-case,
 *                   transition lookup and the "is there anything to report here" test,
 *                   for a whole batch of haystacks at once on the GPU.
 *
 * Result format: one am_match per (haystack, end position) at which the reference would call
 * the fold function at least once.  `state` is a reference state id such that
 * `machineValues ! state` (Automaton.hs:109) is exactly the list of values the reference folds
 * at that position, in the reference's order.  Records are sorted by (haystack, end_pos), which
 * is the order of the reference's left fold.  So
 *     runWithCase cs seed f machine text
 *  == foldl over records r, then over (machineValues ! r.state), of f acc (Match r.end_pos v),
 *     stopping at the first Done.
 *
 * Conventions: every function returns AM_OK (0) or a negative AM_ERR_* code and never throws or
 * aborts; am_last_error() gives a thread-local message.  Inputs are borrowed for the duration of
 * the call only.  Handles are immutable after creation and may be shared between threads; every
 * calling thread launches on its own HIP stream (am_set_stream replaces it for that thread), so
 * calls from different threads run concurrently; two calls on the SAME am_batch serialise on its
 * workspaces.  There is no CPU execution path: without a usable MI355X every run entry point
 * returns AM_ERR_NO_DEVICE.
 */
#ifndef AM_H
#define AM_H

#include <stddef.h>
#include <stdint.h>

/* libam.so is built with -fvisibility=hidden: the functions below (and include/am_debug.h's, for tests and measurements) are
 * everything it exports. */
#ifndef AM_API
#define AM_API __attribute__((visibility("default")))
#endif

#ifdef __cplusplus
extern "C" {
#endif

/* Data.Text.CaseSensitivity (src/Data/Text/CaseSensitivity.hs:14-22) */
#define AM_CASE_SENSITIVE 0
#define AM_IGNORE_CASE 1

#define AM_OK 0
#define AM_ERR_INVALID (-1)      /* malformed arguments / automaton arrays */
#define AM_ERR_NO_DEVICE (-2)    /* no usable HIP device */
#define AM_ERR_HIP (-3)          /* HIP runtime error, see am_last_error() */
#define AM_ERR_OOM (-4)
#define AM_ERR_UNSUPPORTED (-5)

typedef struct am_automaton am_automaton;
typedef struct am_replacer am_replacer;
typedef struct am_needle_ids am_needle_ids;
typedef struct am_replaced am_replaced;
typedef struct am_batch am_batch;
typedef struct am_matches am_matches;
typedef struct am_splitter am_splitter;
typedef struct am_fragments am_fragments;

/* A Text slice: bytes ptr[off .. off+len).  Same shape as U8Slice in
 * benchmark/rust-ffi/app/Main.hs:34-45 (= Data.Text.Internal.Text array/offset/length). */
typedef struct am_slice {
    const uint8_t* ptr;
    size_t off;
    size_t len;
} am_slice;

/* One reportable position.  end_pos = matchPos (Automaton.hs:99-102): code unit index one past the
 * match, relative to the START OF THE SLICE (Automaton.hs:452,530), not to the array. */
typedef struct am_match {
    uint64_t end_pos;
    uint32_t haystack;   /* index into the batch */
    uint32_t state;      /* fold (machineValues ! state) here */
} am_match;

AM_API const char* am_last_error(void);

/* ---- automaton ------------------------------------------------------------------------------
 * am_automaton_create: second half of `build` (Automaton.hs:176-200).  Takes the AcMachine fields
 * exactly as the reference packs them (Automaton.hs:108-123, bit layout :75-94):
 *   transitions   machineTransitions, n_transitions entries
 *   offsets       machineOffsets, n_states + 1 entries (scanl, :170)
 *   root_ascii    machineRootAsciiTransitions, 128 entries
 *   values_len    length (machineValues ! s) for every state (the values themselves stay in Haskell)
 * and flattens them into the device image (LDS filter, cuckoo fingerprint table and Patricia trie of
 * the reversed needles, goto hash of the general path).  The image for each case mode
 * is built and uploaded on first use. */
AM_API int am_automaton_create(const uint64_t* transitions, size_t n_transitions,
                        const uint32_t* offsets, size_t n_states,
                        const uint64_t* root_ascii,
                        const uint32_t* values_len,
                        am_automaton** out);
/* The same with the caller's lower-casing.  The reference lowers non-ASCII code points with GHC base's Data.Char.toLower
 * (src/Data/Text/Utf8.hs:145-151 lowerCodePoint, :138-140 lowerUtf8; inverse src/Data/Text/Utf8/Unlower.hs:26-40), whose table
 * follows the Unicode version of the compiler that builds it (alfred-margaret.cabal:69 `base >= 4.7 && < 5`; 9.6-9.10 = Unicode 15,
 * 9.12+ = 16).  So that IgnoreCase is bit-exact against ANY such build, the table crosses the boundary as data:
 *   lower_from[i] -> lower_to[i], n_lower_pairs pairs = [(c, toLower c) | c <- [minBound ..], toLower c /= c]
 * in any order (pairs with lower_from < 128 are ignored: ASCII is toLowerAscii, :131-135; identity pairs are ignored; one code point
 * with two different images is AM_ERR_INVALID).  NULL, NULL, 0 = the built-in Unicode 14.0 table (am_unicode_version()).
 * The IgnoreCase image bakes the table in (byte edges of every x with toLower x == c; the general kernel's delta table) and
 * records a hash of it: am_automaton_lower_hash(a) == am_lower_table_hash(pairs). */
AM_API int am_automaton_create_ex(const uint64_t* transitions, size_t n_transitions,
                           const uint32_t* offsets, size_t n_states,
                           const uint64_t* root_ascii,
                           const uint32_t* values_len,
                           const uint32_t* lower_from, const uint32_t* lower_to, size_t n_lower_pairs,
                           am_automaton** out);
AM_API uint32_t am_automaton_lower_hash(const am_automaton* a);
AM_API uint32_t am_lower_table_hash(const uint32_t* lower_from, const uint32_t* lower_to, size_t n_pairs);   /* NULL: the built-in table's; 0 on error */
AM_API void am_automaton_destroy(am_automaton* a);
/* Route k: 0 = automatic (the suffix-filter kernel; the table-walk kernel k_dfa for automata whose image carries a DFA section -- dictionaries with
 * heavy suffix nodes -- on batches of 32 MiB and more, from 64 MiB on only where a sample walk finds a needle end every few bytes), 1 = force the general AC kernel (test infrastructure: AM_ERR_UNSUPPORTED unless libam_check.so
 * is loaded), 2 = force the suffix-filter kernel, 3 = force the table-walk kernel (AM_ERR_UNSUPPORTED at run time when the image has no DFA section).
 * All routes report the same matches. */
AM_API int am_automaton_set_kernel(am_automaton* a, int k);

/* ---- one-shot entry points on host slices (what the Haskell shim binds) ----------------------
 * am_count:        runWithCase cs 0 (\n _ -> Step (n+1))  per haystack
 *                  (benchmark/haskell/app/Main.hs:67-76 countMatches; counts VALUES, i.e. fold calls)
 * am_contains_any: Searcher.containsAny (Searcher.hs:156-164) per haystack
 * am_run:          runWithCase / runText / runLower (Automaton.hs:442-553): all records.  A batch of 1 GiB and more against an automaton that may meet
 *                  match-dense text (a dictionary, a small automaton) goes up in segments of whole haystacks, and a segment's records travel to the host
 *                  while the next one is uploaded and scanned; such a result lives on the host only (am_matches_data is immediate,
 *                  am_matches_device_data is NULL, am_matches_fold_hash is not available).  Use am_batch_upload + am_run_batch to keep records in HBM. */
AM_API int am_count(const am_automaton* a, int case_mode, const am_slice* hay, size_t n_hay, uint64_t* counts_out);
AM_API int am_contains_any(const am_automaton* a, int case_mode, const am_slice* hay, size_t n_hay, uint8_t* flags_out);
AM_API int am_run(const am_automaton* a, int case_mode, const am_slice* hay, size_t n_hay, am_matches** out);

/* ---- ONE haystack in ranges (the reference folds one Text of any size, Automaton.hs:468-480) --
 * am_run_range:   the records of runWithCase on `hay` whose end position lies in (lo, hi], 0 <= lo <= hi <= hay->len; end_pos relative to the
 *                 whole slice, haystack = 0.  Only a window of the text is uploaded and scanned: the range plus, before it, 4 bytes per code
 *                 point of the longest needle (whether a needle ends at a position depends only on one maximal match before it), both ends on
 *                 code point boundaries.  Ranges that partition (0, len] give, concatenated, exactly the records of am_run on the whole
 *                 haystack: that is how am_multi_run_single spreads one document over several GPUs, and how a caller scans a document
 *                 larger than device memory.
 * am_count_range: countMatches (benchmark/haskell/app/Main.hs:67-76) over the same positions. */
AM_API int am_run_range(const am_automaton* a, int case_mode, const am_slice* hay, uint64_t lo, uint64_t hi, am_matches** out);
AM_API int am_count_range(const am_automaton* a, int case_mode, const am_slice* hay, uint64_t lo, uint64_t hi, uint64_t* count_out);

/* ---- device-resident batches (bulk callers; what bench.py times) ----------------------------- */
AM_API int am_batch_upload(const am_slice* hay, size_t n_hay, am_batch** out);
/* Borrow a batch that already lives in HBM: d_bytes = concatenated haystacks (16-byte aligned,
 * readable up to round_up(total, 16) bytes), d_offsets = n_hay + 1 ascending uint64 byte offsets
 * with d_offsets[0] == 0 and d_offsets[n_hay] == total_bytes.  The offsets must not change while the batch
 * exists (the text may). */
AM_API int am_batch_from_device(const void* d_bytes, const void* d_offsets, size_t n_hay, uint64_t total_bytes, am_batch** out);
AM_API void am_batch_destroy(am_batch* b);
AM_API uint64_t am_batch_total_bytes(const am_batch* b);

AM_API int am_count_batch(const am_automaton* a, int case_mode, const am_batch* b, uint64_t* counts_out /* n_hay, nullable */, uint64_t* total_out /* nullable */);
AM_API int am_contains_any_batch(const am_automaton* a, int case_mode, const am_batch* b, uint8_t* flags_out);
AM_API int am_run_batch(const am_automaton* a, int case_mode, const am_batch* b, am_matches** out);

/* ---- results ----------------------------------------------------------------------------------
 * Records are produced in HBM; am_matches_data copies them to the host on first use. */
AM_API uint64_t am_matches_size(const am_matches* m);
AM_API const am_match* am_matches_data(am_matches* m);           /* host pointer, owned by m; NULL on error */
AM_API const void* am_matches_device_data(const am_matches* m);  /* am_match[size] in HBM, owned by m; NULL for a result assembled on the host (am_run on a large host batch) */
/* One haystack's records of a large result, without copying all of it: the records are sorted by (haystack, end_pos), so they are the contiguous run
 * [*first_out, *first_out + *count_out) (count 0: no match in that haystack); am_matches_copy brings records [first, first + count) to caller memory.
 * What a lazy fold over one document of a big batch consumes (Automaton.hs:522-534 folds a haystack's matches in order). */
AM_API int am_matches_haystack_range(const am_matches* m, uint32_t haystack, uint64_t* first_out, uint64_t* count_out);
AM_API int am_matches_copy(const am_matches* m, uint64_t first, uint64_t count, am_match* out);
AM_API void am_matches_free(am_matches* m);

/* ---- Searcher.containsAll (src/Data/Text/AhoCorasick/Searcher.hs:167-187) ------------------------
 * For a `Searcher Int` made by buildNeedleIdSearcher (:167-169): machineValues in flat form (the list
 * of state s is values[values_offsets[s] .. values_offsets[s+1]), needle ids 0 .. n_needles-1).  The
 * IntSet fold (:175-183) becomes one bitmap row per haystack in HBM; flags_out[i] = 1 iff every id was
 * reported in haystack i (IS.null of the final set; all ones when n_needles == 0).  `a` must outlive ids. */
AM_API int am_needle_ids_create(const am_automaton* a, const uint64_t* values_offsets, const uint32_t* values, uint32_t n_needles, am_needle_ids** out);
AM_API void am_needle_ids_destroy(am_needle_ids* ids);
AM_API int am_contains_all(const am_needle_ids* ids, int case_mode, const am_slice* hay, size_t n_hay, uint8_t* flags_out);
AM_API int am_contains_all_batch(const am_needle_ids* ids, int case_mode, const am_batch* b, uint8_t* flags_out);

/* ---- per-needle match counts (term frequencies of a dictionary over a corpus) ---------------------
 * The fold  runWithCase cs Map.empty (\m (Match _ v) -> Step (Map.insertWith (+) v 1 m))  (Automaton.hs:442-553: runWithCase / runText / runLower), summed over all
 * haystacks of the batch, as a dense vector: counts_out[v] for v < n_needles = how often the reference would call the fold function with `Match _ v`, i.e. the sum over
 * the records r of the number of k in [values_offsets[r.state], values_offsets[r.state + 1]) with values[k] == v.  Overlapping occurrences count; a needle given twice
 * with two handles counts under both; a state reached through suffix outputs counts every value of its list; the empty needle counts once per position, as the
 * reference reports it.  Handles >= n_needles are SKIPPED (the convention of am_needle_ids: containsAll ignores them likewise); when every handle is < n_needles,
 * the sum of counts_out equals am_count_batch's total (countMatches, benchmark/haskell/app/Main.hs:67-76).  `ids` carries machineValues in flat form
 * (am_needle_ids_create).  counts_out: n_needles entries of host memory; with n_needles == 0 nothing is written (AM_OK); with no haystacks every count is 0.
 * The records are produced and folded in HBM (csrc/am_hist.hip) and never cross the wire; what comes back is n_needles counts.
 *   am_count_by_needle_batch    a device-resident batch, on whatever route the automaton takes.  Record memory is bounded: a batch whose records would exceed 1 GiB is
 *                               counted first (am_count_batch) and then scanned in groups of whole consecutive haystacks, each group folded before the next is scanned;
 *                               the counts are the same (integer adds commute).  A single haystack whose records alone exceed the bound is scanned whole, and for an automaton with the
 *                               empty needle (a record at almost every position) the count pass itself goes through the records of the whole batch: no bound there.
 *   am_count_by_needle          the one-shot form on host slices.  A batch of 1 GiB and more goes up in segments of whole haystacks (like am_run's), and a segment's
 *                               records are folded in HBM while the next segment is uploaded.
 *   am_matches_count_by_needle  the same fold over a result the caller holds (am_run_batch, am_run).  AM_ERR_UNSUPPORTED when the result was assembled on the host
 *                               (am_run on a large host batch: no records in HBM), AM_ERR_INVALID when result and table live on different devices.
 * Arguments are checked before any device work: AM_ERR_INVALID for null ids / batch / result, a null counts_out with n_needles > 0, slices without memory. */
AM_API int am_count_by_needle_batch(const am_needle_ids* ids, int case_mode, const am_batch* b, uint64_t* counts_out /* n_needles, host */);
AM_API int am_count_by_needle(const am_needle_ids* ids, int case_mode, const am_slice* hay, size_t n_hay, uint64_t* counts_out /* n_needles, host */);
AM_API int am_matches_count_by_needle(const am_matches* m, const am_needle_ids* ids, uint64_t* counts_out /* n_needles, host */);

/* ---- per-haystack needle counts: the term-document matrix of a dictionary over a batch --------------
 * The same fold,  runWithCase cs Map.empty (\m (Match _ v) -> Step (Map.insertWith (+) v 1 m))  (Automaton.hs:442-553), run once PER HAYSTACK: which needles occur in
 * which haystack, and how often.  The result is a CSR matrix with one row per haystack: row i is [offsets[i], offsets[i + 1]) of data, and holds one entry per value
 * v < n_needles that the reference's fold would meet at least once in haystack i; count = how often it meets it, i.e. the sum over the haystack's records r of the number
 * of k in [values_offsets[r.state], values_offsets[r.state + 1]) with values[k] == v.  Entries are SORTED BY (haystack, needle) ASCENDING -- a row reads like Map.toAscList
 * of the reference's fold -- and the result is bit-identical from run to run.  No entry has count 0; a haystack without a match has an empty row
 * (offsets[i] == offsets[i + 1]).  Everything am_count_by_needle says about handles holds per row: handles >= n_needles are SKIPPED, a needle given twice with two handles
 * counts under both, two needles under one handle add into one entry, a state reached through suffix outputs counts every value of its list, the empty needle counts once
 * per position.  Counts are 64-bit.  Two identities follow: summing the matrix over its rows gives am_count_by_needle_batch's vector, and when every handle is
 * < n_needles, row i sums to am_count_batch's counts_out[i].  n_needles == 0 gives n_hay empty rows; n_hay == 0 gives offsets = [0] and size 0.
 * The records are produced and folded in HBM (csrc/am_matrix.hip) and never cross the wire; the result stays in HBM until asked for.
 *   am_count_matrix_batch    a device-resident batch, on whatever route the automaton takes.  Record memory is bounded as in am_count_by_needle_batch (the same 1 GiB,
 *                            the same groups of whole consecutive haystacks, a haystack that alone exceeds the bound scanned whole): a group's rows are built before the
 *                            next group is scanned and appended, haystack index and offsets rebased.  Workspace of the fold while a group is in HBM, next to its records:
 *                            16 bytes per slot of the group's table, which has 1.5 x min(values of the group's records, haystacks of the group x n_needles) + 64 slots
 *                            (values = the sum of the records' value-list lengths: 24 bytes per value at most, and a few hundred bytes for `a, aa, aaa` over one
 *                            document), 16 bytes per haystack of the group, 32 per entry of the group (its rows before and after they are ordered; 16 stay in the result,
 *                            and 16 more per entry while the groups of a call that needed several are appended), and for rows of more than 2 048 entries up to 256 MiB of
 *                            n_needles-bit maps.  The library's device buffers are allocated an eighth larger than asked.
 *   am_count_matrix          the one-shot form on host slices.  A batch of 1 GiB and more goes up in segments of whole haystacks, as in am_count_by_needle; a segment's
 *                            rows are built in HBM while the next segment is uploaded, and appended in order.
 *   am_matches_count_matrix  the same fold over a result the caller holds (am_run_batch, am_run), for haystacks 0 .. n_hay - 1.  AM_ERR_UNSUPPORTED when the result was
 *                            assembled on the host (no records in HBM), AM_ERR_INVALID when result and table live on different devices or when n_hay is not greater than
 *                            the largest haystack index in the result (the records are sorted: the last one tells).
 *   am_needle_matrix_*       size = entries of the whole matrix.  offsets (n_hay + 1) / data are host copies made on first use and owned by the result (NULL on error);
 *                            the device_ forms are the arrays in HBM (NULL where there is nothing: no haystack, no entry).  All indices are 64-bit.
 * Arguments are checked before any device work: AM_ERR_INVALID for null ids / batch / result / out, a case_mode that is neither AM_CASE_SENSITIVE nor AM_IGNORE_CASE,
 * slices without memory, n_hay >= 0xFFFFFFFF.  *out is NULL after every failure. */
typedef struct am_needle_count { uint64_t count; uint32_t needle; uint32_t haystack; } am_needle_count;   /* 16 bytes: offsets 0, 8, 12 */
typedef struct am_needle_matrix am_needle_matrix;
AM_API int am_count_matrix_batch(const am_needle_ids* ids, int case_mode, const am_batch* b, am_needle_matrix** out);
AM_API int am_count_matrix(const am_needle_ids* ids, int case_mode, const am_slice* hay, size_t n_hay, am_needle_matrix** out);
AM_API int am_matches_count_matrix(const am_matches* m, const am_needle_ids* ids, size_t n_hay, am_needle_matrix** out);
AM_API uint64_t am_needle_matrix_size(const am_needle_matrix* x);
AM_API uint64_t am_needle_matrix_haystacks(const am_needle_matrix* x);
AM_API const uint64_t* am_needle_matrix_offsets(am_needle_matrix* x);
AM_API const am_needle_count* am_needle_matrix_data(am_needle_matrix* x);
AM_API const void* am_needle_matrix_device_offsets(const am_needle_matrix* x);
AM_API const void* am_needle_matrix_device_data(const am_needle_matrix* x);
AM_API void am_needle_matrix_free(am_needle_matrix* x);

/* ---- Splitter: split every haystack of a batch on one separator, in HBM (src/Data/Text/AhoCorasick/Splitter.hs) ---------------
 * A Splitter is a one-needle automaton, `Aho.build [(sep, ())]` (Splitter.hs:64-67), plus the separator's length.  The scan leaves its sorted records in HBM and the
 * fold stepAccum / finalizeAccum (Splitter.hs:141-170) runs there too (csrc/am_split.hip); no record crosses the wire.  For haystack i the fragments are exactly
 * `split` (Splitter.hs:84-85) in forward order, with AM_IGNORE_CASE exactly `splitIgnoreCase` (Splitter.hs:96-97): a match that starts before the current fragment
 * start is ignored (Splitter.hs:163-164), empty fragments are kept, and every haystack has at least one fragment (finalizeAccum, Splitter.hs:141-147; an empty haystack
 * gives one empty fragment).  The start of a separator that ends at end_pos is end_pos - sep_len_bytes when case sensitive (Splitter.hs:105-107) and
 * skipCodePointsBackwards text (end_pos - 1) (sep_len_code_points - 1) when ignoring case (Splitter.hs:117-121, Utf8.hs:256-276: a K matched by U+212A is three bytes
 * long); that walk never leaves the haystack: one that would is clamped to 0 where the reference calls `error`, which no match the automaton reports can cause.
 *   am_splitter_create       `a`: the automaton of the separator (it must outlive the splitter), given in the case the caller will split in (Splitter.hs:92-93: a
 *                            lower-case needle for splitIgnoreCase).  Checked before any device work: AM_ERR_INVALID for null arguments, sep_len_bytes == 0,
 *                            sep_len_code_points == 0 or > sep_len_bytes (the empty separator is refused: the reference's own arithmetic is meaningless for it) and for
 *                            an automaton that is not a one-needle automaton (exactly one state with values, and one value there, by the values_len given to
 *                            am_automaton_create); AM_ERR_UNSUPPORTED for a handle made from an image, which does not keep values_len.
 *   am_split_batch           a device-resident batch; the result stays in HBM.  AM_ERR_INVALID for null arguments and for splitter and batch on different devices.
 *                            Record memory is NOT bounded here: the whole batch is scanned once and all its records are in HBM while they are folded (one record
 *                            per separator occurrence, 16 bytes each, plus 21 bytes of workspace per record, 37 when a chain of overlapping matches needs the doubling rounds; the
 *                            library's device buffers are allocated an eighth larger than asked: count 48 / 66 bytes per occurrence, and 16 per fragment of the result).
 *   am_split                 the one-shot form on host slices.  n_hay == 0 gives zero fragments and AM_OK.
 *   am_fragments_*           size = fragments of the whole batch; the fragments of haystack i are [offsets[i], offsets[i + 1]) of data, start and len in code units relative
 *                            to the start of the haystack's slice.  offsets / data are host copies made on first use and owned by the result (NULL on error); the device_
 *                            forms are the arrays in HBM (NULL when there is no haystack).  All indices are 64-bit.
 *   am_batch_from_fragments  gathers the fragments' bytes into a NEW batch that the library owns (am_batch_destroy), on src's device: one haystack per fragment, in
 *                            order, offsets = the running sum of the lengths, text 16-byte aligned and readable to round_up(total, 16): usable by every *_batch entry
 *                            point.  am_fragments_offsets maps a line back to its document.  `src` must be the batch the fragments were cut from: AM_ERR_INVALID when its
 *                            haystack count or total bytes differ; AM_ERR_UNSUPPORTED for 0xFFFFFFFF fragments and more (the limit of am_batch_from_device). */
typedef struct am_fragment { uint64_t start; uint64_t len; } am_fragment;
AM_API int am_splitter_create(const am_automaton* a, uint32_t sep_len_bytes, uint32_t sep_len_code_points, am_splitter** out);
AM_API void am_splitter_destroy(am_splitter* s);
AM_API int am_split_batch(const am_splitter* s, int case_mode, const am_batch* b, am_fragments** out);
AM_API int am_split(const am_splitter* s, int case_mode, const am_slice* hay, size_t n_hay, am_fragments** out);
AM_API uint64_t am_fragments_size(const am_fragments* f);
AM_API uint64_t am_fragments_haystacks(const am_fragments* f);
AM_API const uint64_t* am_fragments_offsets(am_fragments* f);
AM_API const am_fragment* am_fragments_data(am_fragments* f);
AM_API const void* am_fragments_device_offsets(const am_fragments* f);
AM_API const void* am_fragments_device_data(const am_fragments* f);
AM_API void am_fragments_free(am_fragments* f);
AM_API int am_batch_from_fragments(const am_batch* src, const am_fragments* f, am_batch** out);

/* ---- match spans: where every match starts, in HBM; all of them, or the leftmost-longest non-overlapping selection ---------------
 * A FOLD STEP is `Match pos v` of runWithCase (Automaton.hs:442-553).  Its SPAN is makeMatch (Replacer.hs:264-274) with the needle's own lengths:
 *   AM_CASE_SENSITIVE   start = pos - len_bytes[v]
 *   AM_IGNORE_CASE      start = skipCodePointsBackwards hay (pos - 1) (len_code_points[v] - 1)   (Utf8.hs:256-276: a k matched by U+212A is three bytes long)
 *   len = pos - start; a needle of length 0 gives start = pos, len = 0.  The walk never leaves the haystack: one that would is clamped to 0 where the reference
 *   calls `error`, as in am_split.  start and len are code units relative to the start of the haystack's slice.
 * AM_SPANS_ALL: one span per fold step whose value handle is < n_needles; handles >= n_needles are SKIPPED (the convention of am_needle_ids).  ORDER: the reference's
 *   fold order -- records ascend by (haystack, end_pos), the values of a record come in list order -- so start + len is non-decreasing per haystack, and the size
 *   equals the sum of am_count_by_needle_batch's vector.
 * AM_SPANS_LEFTMOST_LONGEST: per haystack, over the ALL spans with len > 0 (ZERO-LENGTH spans are never selected): cursor = 0; take the span with the smallest
 *   start >= cursor; TIE-BREAK: among equal starts the largest len, among equal (start, len) the smallest handle; emit it, cursor = start + len, repeat.  The output
 *   ascends by (haystack, start) and is bit-identical from run to run.  For b, abc, abcd over "abcd": ALL = (1,1,0) (0,3,1) (0,4,2), leftmost-longest = (0,4,2).
 * The records are produced, expanded and selected in HBM (csrc/am_spans.hip: no sort -- a bitmap of the distinct starts ranks them, a 64-bit atomic maximum picks the
 * longest span of a start, an exclusive prefix maximum finds the candidates no earlier one reaches, chains of overlapping candidates are walked or pointer-doubled);
 * the result stays in HBM until asked for.  It is CSR like am_fragments: the spans of haystack i are [offsets[i], offsets[i + 1]) of data.
 *   am_span_table_create     the needles' lengths beside machineValues: len_bytes / len_code_points, n_needles entries of host memory each (n_needles is ids'), copied to
 *                            ids' device; `ids` must outlive the table.  AM_ERR_INVALID, before any device work, for null arguments (the arrays may be null when
 *                            n_needles == 0), len_code_points[v] > len_bytes[v], exactly one of the two lengths being 0, len_code_points[v] >= 2^30 (a span length
 *                            fits 32 bits: at most 4 bytes per code point).
 *   am_spans_batch           a device-resident batch, on whatever route the automaton takes.  Record memory is NOT bounded here, as in am_split_batch: the whole batch
 *                            is scanned once and all its records are in HBM while they are folded.  WORKSPACE next to the 16 bytes of a record: 12 bytes per record
 *                            and 16 per haystack; 24 bytes per span (in AM_SPANS_ALL this is the result); in AM_SPANS_LEFTMOST_LONGEST also half a byte per byte of
 *                            text (bitmap, word counts, ranks), 29 bytes per distinct start (45 when a chain needs the doubling rounds) and 24 per span of the result.
 *                            The library's device buffers are allocated an eighth larger than asked.
 *   am_spans                 the one-shot form on host slices (the calling thread's one-shot batch).  n_hay == 0 gives offsets = [0], no span and AM_OK;
 *                            n_needles == 0 gives n_hay empty rows.
 *   am_spans_*               size = spans of the whole batch.  offsets (n_hay + 1) / data are host copies made on first use and owned by the result (NULL on error);
 *                            the device_ forms are the arrays in HBM (NULL where there is nothing: no haystack, no span).  am_spans_rounds = pointer-doubling rounds the
 *                            call ran: 0 in AM_SPANS_ALL and wherever no chain of overlapping candidates was longer than AM_SPANS_CHAIN_LIMIT (csrc/am_config.h) looks.
 * Arguments are checked before any device work: AM_ERR_INVALID for null table / batch / out, a case_mode that is neither AM_CASE_SENSITIVE nor AM_IGNORE_CASE, a mode
 * that is neither AM_SPANS_ALL nor AM_SPANS_LEFTMOST_LONGEST, n_hay >= 0xFFFFFFFF, slices without memory, table and batch on different devices.  *out is NULL after
 * every failure. */
typedef struct am_span { uint64_t start; uint64_t len; uint32_t haystack; uint32_t needle; } am_span;   /* 24 bytes: offsets 0, 8, 16, 20 -- am_prio_match's shape */
typedef struct am_span_table am_span_table;
struct am_spans;                 /* the result.  No typedef: the one-shot entry point has the name, so the type is always written `struct am_spans` */
#define AM_SPANS_ALL 0
#define AM_SPANS_LEFTMOST_LONGEST 1
AM_API int am_span_table_create(const am_needle_ids* ids, const uint32_t* len_bytes, const uint32_t* len_code_points /* n_needles each, host */, am_span_table** out);
AM_API void am_span_table_destroy(am_span_table* t);
AM_API int am_spans_batch(const am_span_table* t, int case_mode, int mode, const am_batch* b, struct am_spans** out);
AM_API int am_spans(const am_span_table* t, int case_mode, int mode, const am_slice* hay, size_t n_hay, struct am_spans** out);
AM_API uint64_t am_spans_size(const struct am_spans* s);
AM_API uint64_t am_spans_haystacks(const struct am_spans* s);
AM_API const uint64_t* am_spans_offsets(struct am_spans* s);
AM_API const am_span* am_spans_data(struct am_spans* s);
AM_API const void* am_spans_device_offsets(const struct am_spans* s);
AM_API const void* am_spans_device_data(const struct am_spans* s);
AM_API uint32_t am_spans_rounds(const struct am_spans* s);
AM_API void am_spans_free(struct am_spans* s);

/* ---- substitute: every leftmost-longest match replaced once, in HBM; the rewritten texts are a batch of their own ---------------
 * For haystack i of the batch, with the rows (s_1, l_1, v_1) ... (s_k, l_k, v_k) of am_spans* in AM_SPANS_LEFTMOST_LONGEST mode:
 *   out_i = hay[0, s_1) ++ repl[v_1] ++ hay[s_1 + l_1, s_2) ++ repl[v_2] ++ ... ++ repl[v_k] ++ hay[s_k + l_k, len_i)
 * which is `replace` (Replacer.hs:163-180) applied to those matches: what Rust's aho-corasick calls replace_all under LeftmostLongest.  It is NOT Replacer.run
 * (am_replacer_*: priorities, repeated passes).  Replacements are bytes and are NEVER SCANNED.  ZERO-LENGTH spans are never selected, so an empty needle inserts
 * nothing.  Handles >= n_needles are SKIPPED (the convention of am_needle_ids).  Under AM_IGNORE_CASE the bytes removed are the SPAN'S OWN len: a k matched by
 * U+212A removes three bytes.  A haystack without a match comes back BYTE FOR BYTE, an empty haystack stays empty, and the output batch has as many haystacks as the
 * input, IN ORDER.  Every index and total is 64-bit: the output may exceed 4 GiB while the input does not.  The bytes do not depend on the order of any atomic: two
 * runs give identical batches.  For b -> X, abc -> Y, abcd -> Z over "abcd b": "Z X"; for a -> "" over "banana": "bnn".
 * The splice runs in HBM (csrc/am_subst.hip): a haystack with k spans is 2k + 1 pieces (gaps of the text, replacements from the pool); an exclusive sum of their
 * lengths places them, the pieces of length 0 are dropped, and a gather over tiles of the new text keeps the tile's slice of the piece table in LDS and writes aligned
 * 16-byte groups.  WORKSPACE of the splice, freed when it returns: 36 bytes per piece (2 x spans + haystacks pieces) and 16 per piece of non-zero length; the result
 * holds its text and 8 bytes per haystack.  The library's device buffers are allocated an eighth larger than asked.
 *   am_subst_table_create   the replacements beside a span table: replacement of handle v = repl_bytes[repl_off[v], repl_off[v + 1]), repl_off has n_needles + 1 entries
 *                           of host memory (n_needles is the span table's); the pool is copied to the table's device, padded so that a 16-byte group read from any
 *                           offset stays inside.  `t` must outlive the table.  AM_ERR_INVALID, before any device work, for null arguments (repl_bytes may be null
 *                           when the pool is empty), repl_off[0] != 0, descending offsets, one replacement of 2^32 bytes and more.
 *   am_batch_substitute     the splice alone: to am_spans what am_batch_from_fragments is to am_fragments.  `s` must be an AM_SPANS_LEFTMOST_LONGEST result of `src`:
 *                           AM_ERR_INVALID for an AM_SPANS_ALL result, for a batch whose haystack count or total bytes differ, for batch, spans and table on different
 *                           devices and for a table whose n_needles differs from that of the span table the spans were made with.  The new batch is owned by the
 *                           library (am_batch_destroy); its text is 16-byte aligned, zero-filled and readable to round_up(total, 16): usable by every *_batch
 *                           entry point.
 *   am_substitute_batch     am_spans_batch in AM_SPANS_LEFTMOST_LONGEST mode followed by the splice.  spans_out (nullable): the spans, in SOURCE coordinates
 *                           (am_spans_free).  Record memory is NOT bounded here, as in am_spans_batch.
 *   am_substitute           the one-shot form on host slices (the calling thread's one-shot batch).  The result is a batch of its own and stays valid after the
 *                           one-shot batch is reused.  n_hay == 0 gives a batch without haystacks and AM_OK.
 *   am_substitute_geometry  the gather's store group and tile in bytes (tests place piece ends on the real seams).
 * Batch accessors -- what a device stage that produces text hands back: am_batch_haystacks; am_batch_device_text / am_batch_device_offsets (the arrays in HBM, owned by
 * the batch or borrowed by it); am_batch_read_offsets copies the n_hay + 1 offsets, am_batch_read_text any byte range [first_byte, first_byte + n_bytes) of the
 * concatenated text to host memory (AM_ERR_INVALID beyond total; a range of 0 bytes is AM_OK).
 * Arguments are checked before any device work: AM_ERR_INVALID for null table / batch / spans / out, a case_mode that is neither AM_CASE_SENSITIVE nor
 * AM_IGNORE_CASE, n_hay >= 0xFFFFFFFF, slices without memory.  *out (and *spans_out) is NULL after every failure. */
typedef struct am_subst_table am_subst_table;
AM_API int am_subst_table_create(const am_span_table* t, const uint64_t* repl_off /* n_needles + 1, host */, const uint8_t* repl_bytes, am_subst_table** out);
AM_API void am_subst_table_destroy(am_subst_table* r);
AM_API int am_batch_substitute(const am_batch* src, const struct am_spans* s, const am_subst_table* r, am_batch** out);
AM_API int am_substitute_batch(const am_subst_table* r, int case_mode, const am_batch* b, am_batch** out, struct am_spans** spans_out /* nullable */);
AM_API int am_substitute(const am_subst_table* r, int case_mode, const am_slice* hay, size_t n_hay, am_batch** out);
AM_API void am_substitute_geometry(uint32_t* group_bytes, uint32_t* tile_bytes);
AM_API uint64_t am_batch_haystacks(const am_batch* b);
AM_API const void* am_batch_device_text(const am_batch* b);
AM_API const void* am_batch_device_offsets(const am_batch* b);
AM_API int am_batch_read_offsets(const am_batch* b, uint64_t* out /* n_hay + 1, host */);
AM_API int am_batch_read_text(const am_batch* b, uint64_t first_byte, uint64_t n_bytes, uint8_t* dst);

/* ---- substitute templates: the replacement may keep, wrap or repeat the MATCHED TEXT itself, in HBM ---------------
 * What sed writes as &, re.sub as \g<0> and others as $0.  A TEMPLATE is a sequence of 0 .. AM_SUBST_MAX_SEGMENTS segments, each AM_SEG_LITERAL (bytes) or
 * AM_SEG_MATCH (the bytes of the span itself, as they stand in the haystack).  For haystack i with the AM_SPANS_LEFTMOST_LONGEST rows (s_1, l_1, v_1) ... (s_k, l_k, v_k):
 *   out_i = hay[0, s_1) ++ T(v_1, hay[s_1, s_1 + l_1)) ++ hay[s_1 + l_1, s_2) ++ ... ++ T(v_k, hay[s_k, s_k + l_k)) ++ hay[s_k + l_k, len_i)
 *   T(v, m) = the segments of template v in order: a literal's bytes, or m for AM_SEG_MATCH
 * Everything "substitute" says above holds: nothing of the output is scanned again, zero-length spans are never selected, handles >= n_needles never appear, every
 * index is 64-bit and the bytes depend on no order.  A template of NO segments deletes the match; [MATCH] is the identity (bytes and offsets of the input); [literal]
 * is am_subst_table_create's replacement; MATCH may occur several times.  Under AM_IGNORE_CASE the match keeps THE TEXT'S OWN SPELLING and width, which no fixed
 * replacement can: a k matched by U+212A puts three bytes where MATCH stands.  A span table with a word class gives whole-word templates (the splice reads spans and
 * needs no class of its own).
 *   nike -> [<b>, MATCH, </b>] under AM_IGNORE_CASE over "NIKE nike":  "<b>NIKE</b> <b>nike</b>"
 *   ab   -> [MATCH, MATCH]  (sed's &&)                  over "xabx":       "xababx"
 * The table is the same am_subst_table: am_batch_substitute, am_substitute_batch, am_substitute and am_subst_table_destroy take it unchanged, and the result is a
 * batch as theirs.  On the device only the PIECE PLAN differs (csrc/am_subst_tpl.h, one definition for the kernels and the CPU): span j of haystack h owns
 * 1 + nseg[v_j] pieces -- its gap, then one piece per segment, a literal read from the pool, a MATCH read from the text -- numbered through the exclusive sum of
 * those counts; the two piece scans, the compaction and the gather are those of "substitute".  WORKSPACE as there, per piece, plus 12 bytes per span.  A table made
 * by am_subst_table_create keeps its fixed plan of two pieces per span and its kernel.
 *   am_subst_table_create_templates  template of handle v = segments [seg_off[v], seg_off[v + 1]) (seg_off: n_needles + 1 entries); segment s has kind seg_kind[s]
 *                           and, as a literal, the bytes lit_bytes[lit_off[s], lit_off[s + 1]) (lit_off: n_seg + 1 entries, a MATCH segment has an empty range).
 *                           Host memory, copied; the pool keeps its padding.  `t` must outlive the table.  AM_ERR_INVALID and *out NULL, before any device work, for
 *                           a null pointer where bytes are needed (seg_kind and lit_off may be null without segments, lit_bytes without literal bytes), seg_off[0] != 0
 *                           or a descending seg_off, more than AM_SUBST_MAX_SEGMENTS segments in one template, an unknown kind, lit_off[0] != 0, a descending lit_off,
 *                           a non-empty range on a MATCH segment, a literal of 2^32 bytes and more. */
#define AM_SUBST_MAX_SEGMENTS 64
#define AM_SEG_LITERAL 0
#define AM_SEG_MATCH 1
AM_API int am_subst_table_create_templates(const am_span_table* t, const uint64_t* seg_off /* n_needles + 1, host */, const uint8_t* seg_kind /* n_seg */,
                                           const uint64_t* lit_off /* n_seg + 1 */, const uint8_t* lit_bytes, am_subst_table** out);

/* ---- whole words: a span table with a word class -- spans, substitute and term counts over the whole-word matches only, in HBM ---------------
 * A WORD CLASS W is a set of byte values, given as 256 flags (non-zero = word byte).  A span (start, len) of a haystack of L bytes is a WHOLE WORD iff both hold:
 *   start == 0        or  hay[start - 1]    is not in W
 *   start + len == L  or  hay[start + len]  is not in W
 * This is the look-around form (?<!\w)needle(?!\w), not \b: it does not look at the needle's own bytes, so c++ is a whole word in "c++ is".  The neighbours are bytes
 * of the SAME haystack only: a batch stores its haystacks back to back, and the last byte of haystack h - 1, the first byte of haystack h + 1 and the zero padding
 * behind the text are never neighbours.  Under AM_IGNORE_CASE `start` is the span's own start from the backwards walk: a k matched by U+212A has its left neighbour
 * three bytes before its end.  A zero-length span follows the same rule with len = 0.  The DEFAULT class (word_bytes == NULL) is 0-9 A-Z a-z _ and every byte
 * 0x80-0xFF, so any non-ASCII code point is a word character; a caller who wants something else passes a table of their own.
 * A span table made with a word class changes what EVERY consumer of that table sees:
 *   AM_SPANS_ALL                       the whole-word rows only, in fold order.  For he, the over "the he she": (0,3,the) (4,2,he) -- not the he inside the and she.
 *   AM_SPANS_LEFTMOST_LONGEST          the same selection rule, over the whole-word rows with len > 0: FILTER, THEN SELECT.  For ab, `ab c` over "ab cd" the plain table
 *                                      selects (0,4,`ab c`), which is followed by d and is no whole word -- filtering afterwards would leave nothing; the table with a
 *                                      class gives (0,2,ab).
 *   am_substitute*, am_batch_substitute  the splice over that selection (the splice reads spans: it needs no class of its own).
 *   am_count_spans_by_needle*          counts[v] = the number of AM_SPANS_ALL rows with needle v: the term frequencies of whole words.
 * A table made by am_span_table_create has no class and behaves byte for byte as before.
 * The predicate sits between the expansion and the selection (csrc/am_words.h, one device function for the expansion and the histogram): the records, the needles'
 * lengths and the text are in HBM already, the class is 32 bytes beside the lengths, no span that is dropped is ever written, and everything after the expansion runs
 * on a compact span array.  Nothing about the scans, the record format or the image changes.
 *   am_word_bytes_default            the default class as 256 flags of 0 / 1.  Needs no device.
 *   am_span_table_create_words       am_span_table_create (the same checks, the same messages) with a class: word_bytes = 256 flags of host memory, NULL for the default.
 *   am_span_table_word_bytes         1 and the class as 256 flags of 0 / 1 in out256 (nullable) for a table with a class, 0 for one without (or a null table).
 *   am_count_spans_by_needle_batch   a device-resident batch; counts_out = n_needles counts of host memory.  Record memory is BOUNDED as in am_count_by_needle_batch
 *                                    (groups of whole haystacks, each scanned and folded before the next; the predicate reads the group's own text).  For a table
 *                                    without a class it is am_count_by_needle_batch's vector.  Integer adds commute: two runs give identical counts.
 *   am_count_spans_by_needle         the one-shot form on host slices (the calling thread's one-shot batch).
 * Arguments are checked before any device work: AM_ERR_INVALID for null table / batch / counts_out (with n_needles > 0), a case_mode that is neither AM_CASE_SENSITIVE
 * nor AM_IGNORE_CASE, n_hay >= 0xFFFFFFFF, slices without memory, table and batch on different devices. */
AM_API void am_word_bytes_default(uint8_t out[256]);
AM_API int am_span_table_create_words(const am_needle_ids* ids, const uint32_t* len_bytes, const uint32_t* len_code_points,
                                      const uint8_t* word_bytes /* 256 flags, host, non-zero = word byte; NULL: the default class */, am_span_table** out);
AM_API int am_span_table_word_bytes(const am_span_table* t, uint8_t* out256 /* nullable */);   /* 1: has a class (copied to out256), 0: none */
AM_API int am_count_spans_by_needle_batch(const am_span_table* t, int case_mode, const am_batch* b, uint64_t* counts_out /* n_needles, host */);
AM_API int am_count_spans_by_needle(const am_span_table* t, int case_mode, const am_slice* hay, size_t n_hay, uint64_t* counts_out /* n_needles, host */);

/* ---- exact case: a span table with a spelling per needle -- most needles match in any casing, some only as spelled, in ONE scan ---------------
 * A dictionary mixes terms that should match in any casing (nike) with terms that mean something only as spelled (US, WHO, Apple).  The automaton holds the
 * lower-cased needles and the scan runs under AM_IGNORE_CASE, as ever; the span table says, per needle handle, how the text must spell it:
 *   exact[v]       the spelling of handle v: a byte string, or absent.
 *   (start, len)   the span makeMatch gives a fold step `Match pos v` -- the span of "match spans", untouched.
 *   The table KEEPS the span iff exact[v] is absent, or both hold:  len == |exact[v]|  and  hay[start, start + len) == exact[v], byte for byte.
 * The rule is the same in both case modes; under AM_CASE_SENSITIVE it is a constant per needle (the needle is its own spelling, or no span of it is a row).  With
 * a word class too, both predicates must hold.  This is still FILTER, THEN SELECT: AM_SPANS_LEFTMOST_LONGEST, substitute, extract, coordinates, near and postings see
 * only the kept rows.  A handle without a spelling behaves exactly as before, and a table with no spelling at all IS the table of am_span_table_create /
 * am_span_table_create_words: the same kernels, the same bytes.
 *   Plain filtering.    us, apple, nike with exact = [US, Apple, -] over "us, US and NIKE's apple" under AM_IGNORE_CASE: AM_SPANS_ALL gives (4,2,us) (11,4,nike).
 *   Width.              k with exact = K: the text K is kept, k is dropped, and so is U+212A (Kelvin sign): its len is 3, not 1.  With exact = U+212A the keeps
 *                       and the drops swap.
 *   Filter, then select. `ab c` with exact = `AB C` and ab without a spelling over "ab c": the plain table selects (0,4); filtering afterwards would leave nothing.
 *                       The cased table gives (0,2,ab).
 *   Duplicate needles.  us twice with exact = [US, -]: two handles of one state.  Over "US" both rows appear, over "us" only the second.
 * The predicate sits where the whole-word predicate sits (csrc/am_words.h, one device function for the expansion, the histogram, the scores and the select's
 * flags); the byte comparison is csrc/am_cased.h's.  Record memory stays bounded wherever it is bounded for a table with a class.  Nothing about the scans, the
 * record format or the image changes.
 *   am_span_table_create_cased   am_span_table_create (the same checks, the same messages) with flags (AM_SPAN_TABLE_WORDS: word_bytes applies, NULL for the default
 *                                class; otherwise word_bytes is not looked at) and spellings: the spelling of v is exact_bytes[exact_off[v], exact_off[v + 1]), an
 *                                empty range means none.  exact_off == NULL: no spelling -- with flags == 0 exactly am_span_table_create, with AM_SPAN_TABLE_WORDS
 *                                exactly am_span_table_create_words.  AM_ERR_INVALID, before any device work and with *out == NULL, for unknown flag bits,
 *                                exact_off[0] != 0 or descending offsets, a spelling of 2^32 bytes or more, and a non-empty spelling that begins with a continuation
 *                                byte, whose number of START bytes ((b & 0xC0) != 0x80) differs from len_code_points[v] (which catches a list that is off by one
 *                                handle), or that belongs to a needle of length 0.  The spellings are copied: the table keeps a host copy and a padded pool on its device.
 *   am_span_table_check_exact    the checks am_span_table_create_cased makes on its spellings, alone: AM_OK or AM_ERR_INVALID with the same message.  Needs no device.
 *   am_span_table_exact          1 and the spelling of `needle` (bytes / len nullable; the host copy, owned by the table) where it has one; 0 otherwise.
 * RuleSet, count_matrix, contains_any / contains_all and the Replacer do not go through a span table: they stay single-mode. */
#define AM_SPAN_TABLE_WORDS 1u   /* word_bytes (NULL: the default class) applies */
AM_API int am_span_table_create_cased(const am_needle_ids* ids, const uint32_t* len_bytes, const uint32_t* len_code_points,
                                      uint32_t flags, const uint8_t* word_bytes,
                                      const uint64_t* exact_off /* n_needles + 1, host; NULL: no spelling */, const uint8_t* exact_bytes,
                                      am_span_table** out);
AM_API int am_span_table_check_exact(const uint32_t* len_bytes, const uint32_t* len_code_points, uint32_t n_needles, const uint64_t* exact_off, const uint8_t* exact_bytes);
AM_API int am_span_table_exact(const am_span_table* t, uint32_t needle, const uint8_t** bytes, uint64_t* len);   /* 1: has a spelling (host copy owned by the table), 0: none */

/* ---- select: keep the haystacks that match and drop the rest, in HBM; the kept haystacks are a batch of their own ---------------
 * `grep -F -f needles` (am_select_any*), `grep -v` (invert), `grep -w` (am_select_spans_batch with a table that carries a word class) and "the lines that mention all of
 * these terms" (am_select_all*) over a batch, without the flags, the texts or the kept texts crossing the wire.  A SELECTION says which haystacks of a batch were kept:
 * ascending uint32 source indices in HBM, copied to the host on first use.  keep[i] = predicate(haystack i) != (invert != 0):
 *   am_select_any_batch     the predicate is byte for byte what am_contains_any_batch reports (Searcher.containsAny).
 *   am_select_all_batch     ... what am_contains_all_batch reports (Searcher.containsAll), with the reference's quirks: [""] is never contained, zero needles is true.
 *   am_select_spans_batch   row i of am_spans_batch(t, case_mode, AM_SPANS_ALL, b) is not empty.  With a table made by am_span_table_create_words that is
 *                           (?<!\w)(n1|n2|...)(?!\w) per haystack, filter then select as above; a zero-length span is a span.  Record memory is BOUNDED as in
 *                           am_count_spans_by_needle_batch (groups of whole haystacks).
 *   am_select_flags         the caller's own predicate: n_hay flags of host memory, non-zero = true.
 *   am_select_any, am_select_all   the one-shot forms on host slices: the indices only (the texts are the caller's already).
 * An empty haystack contains nothing: it is kept under `invert`.  During a *_batch select only scalars cross to the host (the kept count, the kept bytes, the run count
 * and what the scans read back anyway); the bounded-memory grouping of am_select_spans_batch, where it runs, reads what am_count_spans_by_needle_batch reads.
 *   am_batch_from_selection  a NEW batch that the library owns, on src's device: one haystack per kept index, in order, offsets = the running sum of their lengths, the
 *                           text 16-byte aligned, readable to round_up(total, 16) and zero beyond total.  Every *_batch entry point takes it, another select too: a
 *                           selection of a selection composes through the two index arrays.  Consecutive kept haystacks are contiguous in the source, so the bytes
 *                           move in RUNS (maximal sequences of consecutive kept haystacks): keeping everything is one straight copy.  src must be the batch the
 *                           selection was made from: AM_ERR_INVALID when the haystack count, the total bytes or the device differ.  A selection that keeps nothing
 *                           gives a valid batch of 0 haystacks and 0 bytes.
 *   am_selection_indices    host, ascending, never NULL on success (a placeholder element for an empty selection); am_selection_device_indices: the same in HBM.
 *   am_select_geometry      for tests: the gather's tile in bytes, and the haystacks one workgroup of the compaction's exclusive sums handles.
 * Arguments are checked before any device work: AM_ERR_INVALID for null handles or a null out, a case_mode that is neither of the two, null flags with n_hay > 0, slices
 * without memory, handles on different devices.  *out is NULL after every failure. */
typedef struct am_selection am_selection;
AM_API int am_select_any_batch(const am_automaton* a, int case_mode, int invert, const am_batch* b, am_selection** out);
AM_API int am_select_all_batch(const am_needle_ids* ids, int case_mode, int invert, const am_batch* b, am_selection** out);
AM_API int am_select_spans_batch(const am_span_table* t, int case_mode, int invert, const am_batch* b, am_selection** out);
AM_API int am_select_flags(const am_batch* b, const uint8_t* flags /* n_hay, host; nonzero = true */, int invert, am_selection** out);
AM_API int am_select_any(const am_automaton* a, int case_mode, int invert, const am_slice* hay, size_t n_hay, am_selection** out);
AM_API int am_select_all(const am_needle_ids* ids, int case_mode, int invert, const am_slice* hay, size_t n_hay, am_selection** out);
AM_API uint64_t am_selection_size(const am_selection* s);                 /* haystacks kept */
AM_API uint64_t am_selection_source_haystacks(const am_selection* s);
AM_API uint64_t am_selection_total_bytes(const am_selection* s);          /* bytes of the kept haystacks */
AM_API const uint32_t* am_selection_indices(am_selection* s);
AM_API const void* am_selection_device_indices(const am_selection* s);
AM_API void am_selection_free(am_selection* s);
AM_API int am_batch_from_selection(const am_batch* src, const am_selection* s, am_batch** out);
AM_API void am_select_geometry(uint32_t* tile_bytes, uint32_t* scan_block_items);

/* ---- rule sets: many boolean rules over needle groups, evaluated from ONE scan of a batch, in HBM ---------------
 * A rule is "the title mentions nike and shoe, any word of this 5 000-word list, and none of these three".  Categorising a product feed, multi-label tagging and
 * first-rule-wins routing evaluate hundreds of such rules over the same lines; all a rule needs to know is, per haystack, WHICH needles occurred at all -- the set
 * the containsAll scan computes without writing a record.  So one scan with the union dictionary answers every rule of a rule set; Searcher.containsAny (one clause),
 * Searcher.containsAll (unit clauses) and `grep -v` (a negated literal) are special cases of the one operator.
 * SLOTS.  `slots` is an am_needle_ids whose values are slot numbers 0 .. n_slots-1 (its n_needles argument is n_slots).  Several needles may carry the same slot; a
 * needle may appear several times with different slots.  P(h) = { v < n_slots : the fold of runWithCase (Automaton.hs:442-553) over haystack h meets Match _ v } --
 * the complement of containsAll's final IntSet (Searcher.hs:173-187).  Values >= n_slots are SKIPPED (the convention of am_needle_ids).  The empty needle does here
 * what it does in the reference's fold.
 * PROGRAM, in conjunctive normal form over slot literals:
 *   rule_off    uint64[n_rules + 1]    offsets into the clauses; n_clauses = rule_off[n_rules]
 *   clause_off  uint64[n_clauses + 1]  offsets into the literals; n_literals = clause_off[n_clauses]
 *   literals    uint32[n_literals]     bits 0..30: the slot; bit 31 (AM_RULE_NEGATE) set: negated
 * A literal is true iff (slot in P(h)) != negated.  A clause is the OR of its literals; an EMPTY CLAUSE IS FALSE.  A rule is the AND of its clauses; A RULE WITH NO
 * CLAUSE IS TRUE.  So a rule of negative literals only fires on the empty haystack, `x AND NOT x` never fires, `x OR NOT x` always fires.  Duplicate literals are
 * allowed.  The arrays are copied: the caller's may go after am_rules_create; `slots` (and its automaton) must outlive the rules.
 * RESULT (am_rule_hits) for a batch of n_hay haystacks, in HBM until asked for (the accessors make host copies on first use; never NULL on success):
 *   fired   uint64[n_rules][hay_words], hay_words = ceil(n_hay / 64): bit h % 64 of word h / 64 of row r is set iff rule r fires on haystack h; bits beyond n_hay are ZERO
 *   labels  uint32[n_hay]: the smallest rule that fires (first rule wins), 0xFFFFFFFF when none fires
 *   counts  uint64[n_rules]: the haystacks on which the rule fires = the popcount of its row
 * Everything is bit-identical from run to run.  n_rules == 0 is valid (empty rows, every label 0xFFFFFFFF); n_hay == 0 gives an empty result.
 *   am_rules_eval_batch  on a device-resident batch.  The slot rows are bounded workspace (1 GiB): a batch whose rows exceed it is scanned and evaluated in groups of
 *                        whole consecutive haystacks, each a multiple of 64.  Only what the scans read back themselves crosses to the host (with groups: one offset a group).
 *   am_rules_eval        the one-shot form on host slices: the slices go up as ONE batch -- no segments of the upload, unlike am_count_by_needle.
 *   am_select_rule       the haystacks of rule `rule` as a selection of `src` (am_batch_from_selection makes them a batch): which = AM_RULE_FIRED, the rule's bit;
 *                        AM_RULE_FIRST, label == rule -- over all rules these and "no rule" (the inverted union) are a partition of the batch.  src must be the batch
 *                        the hits were made from: AM_ERR_INVALID when the haystack count, the total bytes or the device differ.
 *   am_rules_geometry    for tests: the haystacks one workgroup step of the evaluation handles, the widest slot row (in 32-slot words) it keeps in LDS (wider rows are
 *                        read in HBM), and the rules whose counts a workgroup keeps in LDS (the counts of the rules beyond go to HBM per wavefront).
 * Arguments are checked before any device work: AM_ERR_INVALID for null handles or a null out, offsets that do not start at 0 or that decrease, a literal whose slot is
 * >= n_slots, n_rules == 0xFFFFFFFF, a case_mode or `which` that is neither of the two, rule >= n_rules, handles on different devices, slices without memory,
 * n_hay >= 0xFFFFFFFF.  *out is NULL after every failure. */
#define AM_RULE_NEGATE 0x80000000u
#define AM_RULE_FIRED 0   /* the rule's bit */
#define AM_RULE_FIRST 1   /* label == rule */
typedef struct am_rules am_rules;
typedef struct am_rule_hits am_rule_hits;
AM_API int am_rules_create(const am_needle_ids* slots, const uint64_t* rule_off, const uint64_t* clause_off, const uint32_t* literals, uint32_t n_rules, am_rules** out);
AM_API void am_rules_destroy(am_rules* r);
AM_API int am_rules_eval_batch(const am_rules* r, int case_mode, const am_batch* b, am_rule_hits** out);
AM_API int am_rules_eval(const am_rules* r, int case_mode, const am_slice* hay, size_t n_hay, am_rule_hits** out);
AM_API uint64_t am_rule_hits_haystacks(const am_rule_hits* x);
AM_API uint64_t am_rule_hits_rules(const am_rule_hits* x);
AM_API uint64_t am_rule_hits_hay_words(const am_rule_hits* x);
AM_API const uint64_t* am_rule_hits_fired(am_rule_hits* x);
AM_API const uint32_t* am_rule_hits_labels(am_rule_hits* x);
AM_API const uint64_t* am_rule_hits_counts(am_rule_hits* x);
AM_API const void* am_rule_hits_device_fired(const am_rule_hits* x);
AM_API const void* am_rule_hits_device_labels(const am_rule_hits* x);
AM_API const void* am_rule_hits_device_counts(const am_rule_hits* x);
AM_API void am_rule_hits_free(am_rule_hits* x);
AM_API int am_select_rule(const am_rule_hits* x, uint32_t rule, int which, int invert, const am_batch* src, am_selection** out);
AM_API void am_rules_geometry(uint32_t* tile_haystacks, uint32_t* lds_slot_words, uint32_t* lds_rules);

/* ---- scores: a number per match, added up per haystack, in HBM; top-k and range select over the result ---------------
 * The most common fold after counting:  runText 0 (\acc (Match _ v) -> Step (acc + weight v))  -- sentiment and spam lexicons, keyword relevance, "rank these product
 * titles against this weighted dictionary" -- for every haystack of a batch and up to AM_SCORE_MAX_COLUMNS weight columns from ONE scan.
 * WEIGHTS.  int64 W[n_cols][n_needles], column after column, over the value handles of an am_needle_ids; 1 <= n_cols <= AM_SCORE_MAX_COLUMNS.  The array is copied:
 * the caller's may go after am_weights_create; `ids` (and its automaton) must outlive the weights.
 * SCORE.  For haystack i and column c, score[c][i] = the sum of W[c][v] over every fold step `Match _ v` that runWithCase (Automaton.hs:442-553) makes on haystack i
 * with v < n_needles, i.e. over the haystack's records r and the k in [values_offsets[r.state], values_offsets[r.state + 1]) with values[k] < n_needles.  The sum is
 * taken MODULO 2^64 -- two's complement, what the reference's Int does.  Everything am_count_by_needle says about handles holds per haystack: overlapping occurrences
 * count, handles >= n_needles are SKIPPED, a needle given twice with two handles adds under both, two needles under one handle both add its weight, a state reached
 * through suffix outputs adds every value of its list, the empty needle adds once per position.  Three identities follow, all modulo 2^64:
 *   score[c][i] = sum over v of matrix[i][v] * W[c][v]                      (am_count_matrix's row i)
 *   a column of ones, with every handle < n_needles, is am_count_batch's counts_out
 *   sum over i of score[c][i] = sum over v of count_by_needle[v] * W[c][v]   (am_count_by_needle_batch's vector)
 * WHOLE WORDS.  am_score_spans_batch over a span table with a word class adds only those (record, value) pairs whose span the class keeps -- exactly the rows
 * am_count_spans_by_needle* counts; a table without a class is the plain form.
 * RESULT (am_scores): int64[n_cols][n_hay] in HBM, COLUMN-MAJOR as the weights are, so that a column is contiguous; the host copy is made on first use and owned by
 * the result (never NULL on success: a placeholder element for an empty result).  Integer adds commute: the scores are bit-identical from run to run and whether or
 * not the batch went through in groups or segments.  n_needles == 0 gives all-zero scores; n_hay == 0 gives an empty result.
 *   am_score_batch        a device-resident batch, on whatever route the automaton takes.  The records are produced and summed in HBM (csrc/am_score.hip: a segmented
 *                         sum over the sorted records, no atomic per value or record) and never cross the wire.  Record memory is bounded exactly as in
 *                         am_count_by_needle_batch: the same 1 GiB, the same groups of whole consecutive haystacks.
 *   am_score              the one-shot form on host slices; a batch of 1 GiB and more goes up in segments of whole haystacks, as in am_count_by_needle.
 *   am_score_spans_batch  the whole-word form; t and w must have been made over the same am_needle_ids.
 *   am_matches_score      the same fold over a result the caller holds (am_run_batch, am_run), for haystacks 0 .. n_hay - 1.  AM_ERR_UNSUPPORTED when the result was
 *                         assembled on the host (no records in HBM), AM_ERR_INVALID when n_hay is not greater than the largest haystack index in the result.  Such
 *                         scores do not know the bytes of their batch: the selects below hold them to the haystack count and the device only.
 * TOP-K of a column.  Largest: order the haystacks by (score descending, haystack ascending) and take the first min(k, n_hay); smallest: by (score ascending, haystack
 * ascending).  Ties at the cut go to the lower haystack index; k == 0 gives nothing.  The cut is found on the device (eight passes of an 8-bit radix select over
 * order-preserving keys); nothing of size n_hay crosses to the host.
 *   am_scores_top_k       the winners as {score, haystack} in that order, in host memory: out has room for min(k, n_hay) entries, *n_out = how many were written.
 *   am_select_top_k       the winners as a selection of `src` -- ascending haystack indices, as every selection -- so that am_batch_from_selection makes them a batch.
 *   am_select_score       the haystacks with lo <= score <= hi (lo > hi keeps nothing), or -- invert -- the others.
 * For both selects src must be the batch the scores were made from: AM_ERR_INVALID when the haystack count, the total bytes or the device differ.  Selections compose
 * with am_batch_from_selection and with each other.
 *   am_score_geometry     for tests, known without a device: the records one workgroup step of the fold handles (a wavefront owns a quarter of them, consecutive, 64
 *                         at a time), and the keys one workgroup of the top-k histogram handles.
 * Arguments are checked before any device work: AM_ERR_INVALID for null handles or null outputs, n_cols of 0 or above the maximum, column >= n_cols, a case_mode that
 * is neither of the two, a span table whose ids is not the weights' ids, handles on different devices, slices without memory, n_hay >= 0xFFFFFFFF.  *out is NULL
 * after every failure. */
#define AM_SCORE_MAX_COLUMNS 8
typedef struct am_weights am_weights;
typedef struct am_scores am_scores;
typedef struct am_scored { int64_t score; uint32_t haystack; uint32_t reserved; } am_scored;   /* 16 bytes: offsets 0, 8, 12 */
AM_API int am_weights_create(const am_needle_ids* ids, const int64_t* weights /* n_cols * n_needles, host */, uint32_t n_cols, am_weights** out);
AM_API void am_weights_destroy(am_weights* w);
AM_API int am_score_batch(const am_weights* w, int case_mode, const am_batch* b, am_scores** out);
AM_API int am_score(const am_weights* w, int case_mode, const am_slice* hay, size_t n_hay, am_scores** out);
AM_API int am_score_spans_batch(const am_span_table* t, const am_weights* w, int case_mode, const am_batch* b, am_scores** out);
AM_API int am_matches_score(const am_matches* m, const am_weights* w, size_t n_hay, am_scores** out);
AM_API uint64_t am_scores_haystacks(const am_scores* x);
AM_API uint64_t am_scores_columns(const am_scores* x);
AM_API const int64_t* am_scores_data(am_scores* x);            /* host copy on first use: [n_cols][n_hay] */
AM_API const void* am_scores_device_data(const am_scores* x);  /* the same in HBM */
AM_API void am_scores_free(am_scores* x);
AM_API int am_scores_top_k(am_scores* x, uint32_t column, uint64_t k, int largest, am_scored* out /* min(k, n_hay), host */, uint64_t* n_out);
AM_API int am_select_top_k(const am_scores* x, uint32_t column, uint64_t k, int largest, const am_batch* src, am_selection** out);
AM_API int am_select_score(const am_scores* x, uint32_t column, int64_t lo, int64_t hi, int invert, const am_batch* src, am_selection** out);
AM_API void am_score_geometry(uint32_t* tile_records, uint32_t* topk_block_items);

/* ---- proximity: which matches lie near which, from one scan, in HBM; per query a haystack bitmap for the select ---------------
 * `nike w/20 shoe`, a currency word next to an amount, a negation right before a sentiment word, a drug next to a dosage unit, relation candidates for an extraction
 * model: did a match of one group occur within D bytes of a match of another, and where.  A stage over an AM_SPANS_LEFTMOST_LONGEST result (rows ascending by
 * (haystack, start), disjoint, len > 0); up to AM_NEAR_MAX_QUERIES queries over up to AM_NEAR_MAX_GROUPS groups are answered from one scan and one spans call.
 * GROUPS.  group_mask[v] is a uint32 per needle handle of the span table: bit g set = needle v belongs to group g.  A needle may belong to several groups or to none.
 * QUERY.  am_near_query { group_a, group_b, flags, reserved, max_gap }, 24 bytes at offsets 0, 4, 8, 12, 16; flags is 0 or AM_NEAR_ORDERED, reserved must be 0.
 * For haystack h with leftmost-longest rows s_0 .. s_{k-1} and e_i = start_i + len_i, span i is in group g iff group_mask[needle_i] has bit g.  For query q and every
 * i in group group_a, taken as ANCHOR, the candidates are
 *   p = the largest j < i in group group_b,  gap_p = start_i - e_p
 *   n = the smallest j > i in group group_b, gap_n = start_n - e_i        (under AM_NEAR_ORDERED only n is a candidate)
 * The anchor is NEVER ITS OWN PARTNER, even when it is in both groups: group_a == group_b means "a repeated mention".  The partner is the candidate with the smaller
 * gap; a TIE goes to p, the lower index.  A pair is emitted iff the partner's gap is <= max_gap, compared in 64 bits: max_gap = 2^64 - 1 is valid and means
 * "anywhere in the haystack".  Partners never come from another haystack; touching spans have gap 0.  Because the rows are disjoint and ascending, this partner IS
 * the nearest span of the group on each side.
 * With A = {nike}, B = {shoe} and kids in no group, over "nike kids shoe, shoe nike" the rows are nike[0,4) kids[5,9) shoe[10,14) shoe[16,20) nike[21,25):
 *   query (A, B, max_gap 1)                       the one pair (a=4, b=3, gap=1)
 *   max_gap 6                                     (0,2,6) and (4,3,1)
 *   max_gap 6 with AM_NEAR_ORDERED                (0,2,6) only
 * Over "shoe nike shoe" both gaps are 1 and b = 0.
 * RESULT (am_near_hits), in HBM until asked for (the accessors make host copies on first use; never NULL on success):
 *   pairs   am_near_pair { a, b, gap, haystack, query }, 32 bytes: a and b are indices into the DATA ARRAY of the spans result the hits were made from (global, not
 *           per row); CSR per haystack, offsets[n_hay + 1], as for am_spans; rows ascend by (haystack, a, query)
 *   fired   uint64[n_queries][hay_words], hay_words = ceil(n_hay / 64): bit h % 64 of word h / 64 of row q is set iff query q has at least one pair in haystack h; bits
 *           beyond n_hay are ZERO (am_rule_hits' layout)
 *   counts  uint64[n_queries]: the pairs of query q
 * Everything is bit-identical from run to run.  n_queries == 0, no haystacks and no spans are all valid and give empty shapes.
 *   am_near_create    compiles the groups and queries for a span table; the arrays are copied, the table must outlive the handle.
 *   am_near_spans     the stage alone over a spans result the caller holds: AM_ERR_INVALID for an AM_SPANS_ALL result (as am_batch_substitute), for spans whose
 *                     n_needles differs from the table's, for handles on different devices.  The join (csrc/am_near.hip) needs no sort, no atomic per pair and no
 *                     lane loop whose trip count depends on the text: one bitmap row over the span indices per group, per 64-span word the nearest non-zero word
 *                     on either side, then a lane per span finds both candidates by bit arithmetic.  WORKSPACE, freed when the call returns: 20 bytes per span and
 *                     0.25 bytes per span and group a query names (8 at the most); the result holds 32 bytes per pair, 8 per haystack and 8 per query and 64
 *                     haystacks.  Only the pair count crosses to the host.  The library's device buffers are allocated an eighth larger than asked.
 *   am_near_batch     am_spans_batch(t, case_mode, AM_SPANS_LEFTMOST_LONGEST, b) and the stage; spans_out (nullable): the spans a and b index (am_spans_free).
 *                     Record memory is NOT bounded here, as in am_spans_batch.  A span table with a word class gives whole-word proximity (the stage reads spans).
 *   am_near           the one-shot form on host slices (the calling thread's one-shot batch).
 *   am_select_near    the haystacks of query `query`'s row of fired as a selection of `src` -- to these hits what am_select_rule(..., AM_RULE_FIRED, ...) is to rule
 *                     hits; src must be the batch the spans were made from: AM_ERR_INVALID when the haystack count, the total bytes or the device differ.
 *   am_near_geometry  for tests, known without a device: the spans one workgroup step handles (a sweep of the word links covers four times as many WORDS), and the
 *                     spans of one bitmap word.
 * Arguments are checked before any device work (a null group_mask alone is seen after the runtime is up: whether it is needed is the table's needle count):
 * AM_ERR_INVALID for null handles or a null out, n_queries > AM_NEAR_MAX_QUERIES, a group index >= 32, unknown flag
 * bits or reserved != 0, query >= n_queries, a case_mode that is neither of the two, slices without memory, n_hay >= 0xFFFFFFFF.  *out and *spans_out are NULL after
 * every failure. */
#define AM_NEAR_MAX_GROUPS 32
#define AM_NEAR_MAX_QUERIES 64
#define AM_NEAR_ORDERED 1u
struct am_near;                                         /* (no typedef: am_near alone names the one-shot entry point, as am_spans does) */
typedef struct am_near_hits am_near_hits;
typedef struct am_near_query { uint32_t group_a, group_b, flags, reserved; uint64_t max_gap; } am_near_query;   /* 24 bytes: offsets 0, 4, 8, 12, 16 */
typedef struct am_near_pair { uint64_t a, b, gap; uint32_t haystack, query; } am_near_pair;                     /* 32 bytes: offsets 0, 8, 16, 24, 28 */
AM_API int am_near_create(const am_span_table* t, const uint32_t* group_mask /* n_needles, host */, const am_near_query* queries, uint32_t n_queries, struct am_near** out);
AM_API void am_near_destroy(struct am_near* p);
AM_API int am_near_spans(const struct am_near* p, const struct am_spans* s, am_near_hits** out);
AM_API int am_near_batch(const struct am_near* p, int case_mode, const am_batch* b, am_near_hits** out, struct am_spans** spans_out /* nullable */);
AM_API int am_near(const struct am_near* p, int case_mode, const am_slice* hay, size_t n_hay, am_near_hits** out, struct am_spans** spans_out /* nullable */);
AM_API uint64_t am_near_hits_size(const am_near_hits* x);          /* pairs */
AM_API uint64_t am_near_hits_haystacks(const am_near_hits* x);
AM_API uint64_t am_near_hits_queries(const am_near_hits* x);
AM_API uint64_t am_near_hits_hay_words(const am_near_hits* x);
AM_API const uint64_t* am_near_hits_offsets(am_near_hits* x);
AM_API const am_near_pair* am_near_hits_data(am_near_hits* x);
AM_API const uint64_t* am_near_hits_fired(am_near_hits* x);
AM_API const uint64_t* am_near_hits_counts(am_near_hits* x);
AM_API const void* am_near_hits_device_offsets(const am_near_hits* x);
AM_API const void* am_near_hits_device_data(const am_near_hits* x);
AM_API const void* am_near_hits_device_fired(const am_near_hits* x);
AM_API const void* am_near_hits_device_counts(const am_near_hits* x);
AM_API void am_near_hits_free(am_near_hits* x);
AM_API int am_select_near(const am_near_hits* x, uint32_t query, int invert, const am_batch* src, am_selection** out);
AM_API void am_near_geometry(uint32_t* tile_spans, uint32_t* word_spans);

/* ---- extract: the matched text with some characters around it, in HBM; the snippets are a batch of their own ---------------
 * `grep -o`, `grep -o -E '.{0,40}needle.{0,40}'`, a keyword-in-context concordance, the snippets of a search front end, the windows an entity-extraction pipeline gives
 * to its next model -- over a batch, without the spans (24 bytes each) or the snippets crossing the wire.
 * A byte b is a START byte iff (b & 0xC0) != 0x80.  The definition is on bytes, so it holds for text that is not valid UTF-8.  For a span (s, l) of haystack h with L
 * bytes, e = s + l, before = B and after = A (code points):
 *   ws = the index of the B-th START byte of h among the indices < s, counted leftwards from s; 0 if there are fewer than B; s if B == 0
 *   we = the index of the A-th START byte of h among the indices > e, counted rightwards; L if there are fewer than A; e if A == 0
 *   the WINDOW is [ws, we), i.e. am_fragment {ws, we - ws}, relative to the haystack like every fragment.
 * On valid UTF-8, where spans lie on code point boundaries, the window is the span plus at most B whole code points before it and at most A after it.  The walks NEVER
 * LEAVE THE HAYSTACK: bytes of the neighbouring haystacks are never counted or included, and neither is the padding behind the text (in a borrowed batch the padding
 * need not be zero).
 *   AM_EXTRACT_EACH    one fragment per span, in the spans' order, with the spans' own CSR offsets: fragment k belongs to span k.  Overlapping windows repeat text;
 *                      ZERO-LENGTH fragments are kept.  Takes an AM_SPANS_ALL or an AM_SPANS_LEFTMOST_LONGEST result.
 *   AM_EXTRACT_MERGED  per haystack, the union of the windows as disjoint ascending pieces, as `grep -C` prints them: window i joins the piece of window i - 1 of the SAME
 *                      haystack iff ws_i <= we_{i-1} -- TOUCHING windows join, a gap of one byte separates; a piece is [ws of its first window, we of its last).  The
 *                      first span of a haystack always opens a piece, whatever the last window of the haystack before it was.  Takes an AM_SPANS_LEFTMOST_LONGEST
 *                      result only (those rows ascend by start and do not overlap, so ws and we are both non-decreasing and a comparison with the neighbour decides);
 *                      AM_ERR_INVALID for an AM_SPANS_ALL result, as in am_batch_substitute.
 * The stage runs in HBM (csrc/am_extract.hip): one lane per span walks aligned 16-byte groups of the text -- one load, the 16-bit mask of the group's START bytes cut to
 * the haystack and to the walk's side of the span, a popcount, a select in the group that holds the wanted byte; MERGED flags the spans that open a piece, ranks them
 * with one exclusive sum, and only the piece count crosses to the host.  WORKSPACE of AM_EXTRACT_MERGED, freed when the call returns: 28 bytes per span (none in
 * AM_EXTRACT_EACH); the result holds 16 bytes per fragment and 8 per haystack.  The library's device buffers are allocated an eighth larger than asked.
 *   am_fragments_from_spans  the stage alone: to am_spans what am_batch_substitute is, with am_fragments as the result.  src must be the batch the spans were made from:
 *                            AM_ERR_INVALID when the haystack count, the total bytes or the device differ.  The result carries src's size, so
 *                            am_batch_from_fragments(src, result, ...) accepts it, and am_fragments_offsets maps a fragment back to its haystack.  No haystacks gives
 *                            offsets = [0] and AM_OK; no spans gives n_hay empty rows.
 *   am_extract_batch         am_spans_batch(t, case_mode, spans_mode, b), the stage and am_batch_from_fragments in one call: the new batch has ONE HAYSTACK PER FRAGMENT
 *                            (a zero-length fragment is an empty haystack), owned by the library (am_batch_destroy), usable by every *_batch entry point.  frags_out
 *                            (nullable): the fragments in SOURCE coordinates (am_fragments_free); their offsets map a snippet back to its document.  A span table with
 *                            a word class extracts whole words only (the stage reads spans).  AM_ERR_UNSUPPORTED where am_batch_from_fragments returns it (2^32 - 1
 *                            fragments and more).  Record memory is NOT bounded here, as in am_spans_batch.
 *   am_extract               the one-shot form on host slices (the calling thread's one-shot batch).  The result is a batch of its own and stays valid after the
 *                            one-shot batch is reused.  n_hay == 0 gives a batch without haystacks and AM_OK.
 * Arguments are checked before any device work: AM_ERR_INVALID for null table / batch / spans / out, a case_mode that is neither AM_CASE_SENSITIVE nor AM_IGNORE_CASE, a
 * spans_mode that is neither AM_SPANS_ALL nor AM_SPANS_LEFTMOST_LONGEST, a mode that is neither AM_EXTRACT_EACH nor AM_EXTRACT_MERGED, AM_EXTRACT_MERGED with
 * AM_SPANS_ALL, n_hay >= 0xFFFFFFFF, slices without memory, handles on different devices.  *out (and *frags_out) is NULL after every failure. */
#define AM_EXTRACT_EACH 0
#define AM_EXTRACT_MERGED 1
AM_API int am_fragments_from_spans(const am_batch* src, const struct am_spans* s, uint32_t before, uint32_t after, int mode, am_fragments** out);
AM_API int am_extract_batch(const am_span_table* t, int case_mode, int spans_mode, uint32_t before, uint32_t after, int mode,
                            const am_batch* b, am_batch** out, am_fragments** frags_out /* nullable */);
AM_API int am_extract(const am_span_table* t, int case_mode, int spans_mode, uint32_t before, uint32_t after, int mode,
                      const am_slice* hay, size_t n_hay, am_batch** out, am_fragments** frags_out /* nullable */);

/* ---- coordinates: match positions in code points, UTF-16 code units, line and column, in HBM ---------------
 * Every position the library returns is a byte offset into the UTF-8 text (am_match.end_pos, am_span.start / .len, am_fragment.start / .len): the reference's contract,
 * and the default.  A Python caller wants code points (text[start:]), a JavaScript / Java / .NET / Language-Server consumer UTF-16 code units, a code-search or
 * secret-scanning front end line:column inside a whole document -- and under AM_IGNORE_CASE a match has the text's own width, so none of it follows from the needle.
 * This stage converts a result in HBM into a result in HBM; it changes no other entry point.
 * THE DEFINITION is on bytes, so it holds for any input.  For a haystack that occupies the bytes [base, end) of its batch and a position 0 <= p <= end - base:
 *   cp(p)         the number of bytes b of [base, base + p) with (b & 0xC0) != 0x80 (the START bytes of "extract")
 *   u16(p)        cp(p) + the number of bytes >= 0xF0 of the same range (a four-byte sequence is a surrogate pair)
 *   line(p)       the number of 0x0A bytes of [base, base + p), 0-based; 0x0D is not special
 *   linestart(p)  1 + the position of the last 0x0A of [base, base + p), or 0 if there is none: never in another haystack
 *   col_U(p)      U(p) - U(linestart(p)), U one of bytes, cp, u16
 * A span or fragment (start, len) in unit U becomes (U(start), U(start + len) - U(start)).  On valid UTF-8 at code point boundaries these are Python's
 * len(b[:p].decode()), len(s[:i].encode("utf-16-le")) // 2, s.count("\n", 0, i) and i - (s.rfind("\n", 0, i) + 1).  Bytes outside [base, base + p) NEVER COUNT: not a
 * neighbouring haystack's, not the padding up to round_up(total, 16), whatever a borrowed batch holds there.
 * THE INDEX (csrc/am_coords.hip, am_coords.h): one pass over the text counts, per tile of 128 aligned bytes, the bytes of every class `what` asks for; an exclusive sum
 * per class turns the counts into uint64 prefixes, 8 bytes per class and tile (at most 24 bytes per 128 bytes of text: 19 %), which the index keeps in HBM.  A lookup
 * is one prefix entry and at most eight 16-byte loads of the position's own tile; a line start is found in the position's tile or by a binary search over the
 * newline prefix.  What crosses to the host: nothing, except the one flag word of am_coords_positions*.
 *   am_coords_create      builds the index of a batch for AM_COORDS_CODE_POINTS | AM_COORDS_UTF16 (implies CODE_POINTS) | AM_COORDS_LINES; what == 0 is an index that
 *                         serves AM_UNIT_BYTES only.  OWNERSHIP: the index borrows the batch's text and offsets, THE BATCH MUST OUTLIVE THE INDEX.  A batch without
 *                         haystacks gives an index whose calls return empty results.
 *   am_coords_index_bytes the bytes of HBM the index keeps (0 for NULL).
 *   am_coords_spans       a result of the same type, row count, offsets, haystack, needle and mode as `s`; only start / len are in `unit`.  The result is MARKED AS
 *   am_coords_fragments   CONVERTED: the stages that read byte spans -- am_batch_substitute, am_fragments_from_spans, am_near_spans, am_batch_from_fragments and
 *                         am_coords_* itself -- refuse it with AM_ERR_INVALID.  AM_UNIT_BYTES gives a plain copy that is not marked.
 *   am_coords_ranges      line and column of every span's start and of its end (start + len), the columns in `unit`; CSR like am_spans, row k belongs to span k and the
 *                         offsets are the spans'.  Needs an index with AM_COORDS_LINES and the prefixes `unit` needs.
 *   am_coords_positions   converts any (haystack, relative position) list -- this is how am_match.end_pos is converted -- from host arrays into a host array;
 *   am_coords_positions_device   the same over arrays in HBM (hay uint32[n], pos uint64[n], out uint64[n]) on the calling thread's stream.  hay[i] >= the batch's
 *                         haystack count, or pos[i] beyond the haystack's length: the kernel raises one flag word, the host reads that word and the call returns
 *                         AM_ERR_INVALID (d_out is unspecified then).  n == 0 is AM_OK.
 * Arguments are checked before any device work: AM_ERR_INVALID for null handles / arrays / out, an unknown unit, bits of `what` that are not defined, a result that
 * is marked as converted, spans or fragments that were not produced from the index's batch (haystack count, total bytes, device), and an index that lacks what the
 * call needs -- the message names the missing flag (AM_COORDS_CODE_POINTS, AM_COORDS_UTF16, AM_COORDS_LINES).  No haystacks, and no rows, give empty results and
 * AM_OK.  *out is NULL after every failure. */
#define AM_UNIT_BYTES 0
#define AM_UNIT_CODE_POINTS 1
#define AM_UNIT_UTF16 2
#define AM_COORDS_CODE_POINTS 1u   /* which prefixes the index carries */
#define AM_COORDS_UTF16 2u         /* implies CODE_POINTS */
#define AM_COORDS_LINES 4u
typedef struct am_coords am_coords;
typedef struct am_span_range { uint64_t start_line, start_col, end_line, end_col; } am_span_range;   /* 32 bytes */
typedef struct am_ranges am_ranges;   /* CSR like am_spans: row k belongs to span k, offsets are the spans' */
AM_API int am_coords_create(const am_batch* b, uint32_t what, am_coords** out);
AM_API void am_coords_destroy(am_coords* c);
AM_API uint64_t am_coords_index_bytes(const am_coords* c);
AM_API int am_coords_spans(const am_coords* c, const struct am_spans* s, int unit, struct am_spans** out);
AM_API int am_coords_fragments(const am_coords* c, const am_fragments* f, int unit, am_fragments** out);
AM_API int am_coords_ranges(const am_coords* c, const struct am_spans* s, int unit /* of the columns */, am_ranges** out);
AM_API uint64_t am_ranges_size(const am_ranges* r);
AM_API uint64_t am_ranges_haystacks(const am_ranges* r);
AM_API const uint64_t* am_ranges_offsets(am_ranges* r);
AM_API const am_span_range* am_ranges_data(am_ranges* r);
AM_API const void* am_ranges_device_offsets(const am_ranges* r);
AM_API const void* am_ranges_device_data(const am_ranges* r);
AM_API void am_ranges_free(am_ranges* r);
AM_API int am_coords_positions(const am_coords* c, const uint32_t* hay, const uint64_t* pos, uint64_t n, int unit, uint64_t* out /* host arrays */);
AM_API int am_coords_positions_device(const am_coords* c, const void* d_hay, const void* d_pos, uint64_t n, int unit, void* d_out /* HBM, the calling stream */);

/* ---- postings: the spans of a result by NEEDLE -- a positional inverted index, document frequencies, the concordance of one term, in HBM ---------------
 * Every other result is keyed by haystack.  The transposed questions -- where does each term occur, in how many documents does it occur (the IDF half of TF-IDF),
 * show every occurrence of this one term with context -- need the rows of a spans result ordered by needle: a stable sort by a small integer key, done in HBM.
 * THE DEFINITION.  S is a spans result with n = am_spans_size(S) rows -- AM_SPANS_ALL or AM_SPANS_LEFTMOST_LONGEST, with or without a word class, in any unit --
 * and N the n_needles of the table it was made with.
 *   perm         the STABLE sort of 0 .. n-1 by S.data[i].needle
 *   data[k]      S.data[perm[k]], the same 24-byte am_span
 *   source[k]    perm[k] as uint64: the row of S that data[k] came from.  It carries am_ranges rows, am_near pair indices or a caller's own per-span array through
 *                the permutation
 *   offsets[v]   for v = 0 .. N: the number of rows with needle < v.  Row v is [offsets[v], offsets[v+1]); a needle that never occurs has an empty row;
 *                offsets[v+1] - offsets[v] equals am_count_spans_by_needle_batch's counts[v] in AM_SPANS_ALL mode.  Inside a row the entries ascend by (haystack, then
 *                S's own order), because S does
 *   doc_freq[v]  uint64[N]: the distinct haystacks in row v -- the k of the row that are its first entry or have data[k].haystack != data[k-1].haystack
 * Everything is bit-identical from run to run.  Needles nike (0) and shoe (1), texts "shoe nike shoe" and "nike", case sensitive, AM_SPANS_ALL:
 *   S         (0,4,h0,1) (5,4,h0,0) (10,4,h0,1) (0,4,h1,0)            as (start, len, haystack, needle)
 *   offsets   [0,2,4]
 *   data      (5,4,h0,0) (0,4,h1,0) (0,4,h0,1) (10,4,h0,1)
 *   source    [1,3,0,2]
 *   doc_freq  [2,1]
 * THE SORT (csrc/am_postings.hip, am_postings.h) is a least-significant-digit radix sort over (needle uint32, row index uint32) pairs in plain launches: no
 * workgroup waits for another.  passes = 0 for N <= 1, else ceil(bitlen(N-1) / 8), 4 at the most; the bits are divided evenly among the passes.  Per pass a count
 * table per tile, the library's exclusive sum over it, and a scatter whose order inside a tile comes from wavefront ballots, not from the order of atomics.  Then one
 * gather of the 24-byte rows, a binary search per needle for the offsets, and a segmented count for doc_freq.
 * The sort never reads start or len: converted spans (am_coords_spans) are accepted and the result carries S's unit, mode, source size and haystack count.
 * LIMIT: n >= 0xFFFFFFFF rows are AM_ERR_UNSUPPORTED (the sort carries 32-bit row indices; am_batch_from_fragments has the same limit).  That is 96 GiB of spans:
 * no test reaches it.  WORKSPACE, freed when the call returns: 16 bytes per span (two key and two index arrays that take turns) and, per pass, 12 bytes per digit
 * value and tile of am_postings_geometry's tile_spans spans -- at most 3 KiB per tile, 0.4 bytes per span.  The result holds 32 bytes per span (data, source) and
 * 16 bytes per needle (offsets, doc_freq).  Nothing crosses to the host during the stage.  Record memory is NOT bounded in am_postings_batch, as in am_spans_batch.
 *   am_postings_from_spans  the stage alone over a spans result the caller holds.  AM_ERR_UNSUPPORTED for a result whose rows are not in HBM.
 *   am_postings_batch       am_spans_batch(t, case_mode, spans_mode, b) and the stage.  AM_ERR_INVALID for table and batch on different devices.
 *   am_postings             the one-shot form on host slices (the calling thread's one-shot batch).
 *   am_postings_size / _needles / _haystacks   n, N and S's haystack count.
 *   am_postings_offsets / _data / _source / _doc_freq   host copies, made on first use: N + 1, n, n and N entries.  Never NULL on success: an array without entries is
 *                           one placeholder element.
 *   am_postings_device_*    the arrays in HBM, NULL where there is nothing: a result without rows (n == 0: no haystacks, no spans, N == 0) keeps nothing in HBM, its
 *                           offsets are N + 1 zeros ([0] for N == 0) and its doc_freq N zeros.
 *   am_spans_of_needle      row `needle` as a spans result of its own, with S's haystack count, source size, mode, unit and n_needles: the per-haystack offsets are
 *                           rebuilt in HBM, one binary search per haystack over the row's haystack field; the row is a device-to-device copy.  What crosses: the
 *                           row's two offsets.  A subset of leftmost-longest spans still ascends and does not overlap, so am_fragments_from_spans (EACH and MERGED),
 *                           am_coords_* and am_batch_substitute take it as any spans result; a row of converted-unit postings is refused by the byte-span stages as
 *                           converted spans are.  The concordance of one term AMONG THE DICTIONARY'S matches: a one-needle automaton cannot give that under
 *                           leftmost-longest or whole words.  AM_ERR_INVALID for needle >= N.
 *   am_postings_geometry    for tests, known without a device: the spans of a workgroup tile, the consecutive spans of a wavefront's portion (a round is 64 of
 *                           them), the passes for n_needles and the bits each pass sorts, lowest first (bits[4], zero beyond passes).
 * Arguments are checked before any device work: AM_ERR_INVALID for null handles or a null out, a case_mode or spans_mode that is neither of the two, slices without
 * memory, n_hay >= 0xFFFFFFFF, needle >= N.  *out is NULL after every failure. */
struct am_postings;                                     /* (no typedef: am_postings alone names the one-shot entry point, as am_spans does) */
AM_API int am_postings_from_spans(const struct am_spans* s, struct am_postings** out);
AM_API int am_postings_batch(const am_span_table* t, int case_mode, int spans_mode, const am_batch* b, struct am_postings** out);
AM_API int am_postings(const am_span_table* t, int case_mode, int spans_mode, const am_slice* hay, size_t n_hay, struct am_postings** out);
AM_API uint64_t am_postings_size(const struct am_postings* p);
AM_API uint64_t am_postings_needles(const struct am_postings* p);
AM_API uint64_t am_postings_haystacks(const struct am_postings* p);
AM_API const uint64_t* am_postings_offsets(struct am_postings* p);      /* N + 1 */
AM_API const am_span* am_postings_data(struct am_postings* p);
AM_API const uint64_t* am_postings_source(struct am_postings* p);
AM_API const uint64_t* am_postings_doc_freq(struct am_postings* p);     /* N */
AM_API const void* am_postings_device_offsets(const struct am_postings* p);
AM_API const void* am_postings_device_data(const struct am_postings* p);
AM_API const void* am_postings_device_source(const struct am_postings* p);
AM_API const void* am_postings_device_doc_freq(const struct am_postings* p);
AM_API void am_postings_free(struct am_postings* p);
AM_API int am_spans_of_needle(const struct am_postings* p, uint32_t needle, struct am_spans** out);
AM_API void am_postings_geometry(uint64_t n_needles, uint32_t* tile_spans, uint32_t* wave_spans, uint32_t* passes, uint32_t* bits /* [4] */);

/* Checksum of the fold sequence of a result (harness aid; SURVEY 8d "parity check at scale",
 * benchmark/benchmark.py:65-69 asserts count identity on every run).  For every haystack i < n_hay:
 *   hash_out[i]  = foldl (\h (pos, v) -> h * 0x100000001B3 + mix pos v) 0  over the matches the reference's
 *                  runWithCase would hand to its fold function for haystack i, in its order, where
 *                  mix pos v = let x0 = (pos * 0x9E3779B97F4A7C15) xor (v + 0x632BE59BD9B4E019); x1 = x0 xor (x0 >> 32);
 *                                  x2 = x1 * 0xD6E8FEB86659FD93 in x2 xor (x2 >> 32)          (all mod 2^64)
 *   count_out[i] = the number of those matches (= countMatches, benchmark/haskell/app/Main.hs:67-76); nullable.
 * `values` carries machineValues in flat form (am_needle_ids_create; any uint32 payload handles, n_needles unused).
 * Computed on the device from the records in HBM; two runs agree on hash and count iff they fold the same
 * (matchPos, value) sequences (up to 64-bit collisions). */
AM_API int am_matches_fold_hash(const am_matches* m, const am_needle_ids* values, size_t n_hay, uint64_t* hash_out, uint64_t* count_out);

/* ---- Replacer: all passes of Replacer.run on the device -----------------------------------------
 * Replaces the loop `runWithLimit.go` (src/Data/Text/AhoCorasick/Replacer.hs:219-242) for a batch of
 * haystacks: per pass one scan (:223-225), prependMatch/makeMatch (:252-274), the replacementLength
 * check (:183-187, :240), sort + removeOverlap (:191-198, :241) and replace (:163-180) all run in HBM;
 * only finished haystacks travel back.  The caller hands over machineValues of the Replacer's
 * automaton (`Searcher Payload`, :72-77) in flat form:
 *   values_offsets  n_states + 1 entries; the list of state s (in the reference's order) is
 *                   payloads[values[values_offsets[s] .. values_offsets[s+1])]
 *   payloads        Payload (:59-70) per needle: priority, lengths of the ORIGINAL needle in bytes
 *                   and code points (:112-113), replacement = repl_bytes[repl_off .. +repl_len)
 *   min_priority    1 - numNeedles (:217)
 * Priorities must be distinct and <= 0, as build (:100-104) and compose (:127-131) make them; any such values do, INT64_MIN excepted
 * (the fold's seed, :222).  min_priority must be <= every priority given: it only ends the loop early (:241); a larger one cuts the lower priorities off.
 * `a` must outlive the replacer.  case_mode is the Replacer's replacerCaseSensitivity.
 * Batches of many documents (>= 64, <= 1 MiB on average, no document with more than 4096 matches) run ALL passes of a
 * haystack inside one kernel (one wavefront per haystack, csrc/am_rploop.hip); everything else goes pass by pass
 * (csrc/am_replace.hip).  The results are the same texts either way; am_replaced_passes reports the passes of the
 * haystack that needed the most. */
typedef struct am_payload {
    int64_t priority;
    uint32_t len_bytes;
    uint32_t len_code_points;
    uint64_t repl_off;
    uint32_t repl_len;
    uint32_t reserved;
} am_payload;
AM_API int am_replacer_create(const am_automaton* a, int case_mode,
                       const uint64_t* values_offsets, const uint32_t* values,
                       const am_payload* payloads, size_t n_payloads,
                       const uint8_t* repl_bytes, size_t n_repl_bytes,
                       int64_t min_priority, am_replacer** out);
AM_API void am_replacer_destroy(am_replacer* r);
/* max_length: runWithLimit's maxLength (:203); UINT64_MAX = `run` (:200-201, maxBound). */
AM_API int am_replacer_run(const am_replacer* r, const am_slice* hay, size_t n_hay, uint64_t max_length, am_replaced** out);
AM_API int am_replacer_run_batch(const am_replacer* r, const am_batch* b, uint64_t max_length, am_replaced** out);   /* b is not modified */
/* The same, but the rewritten texts STAY IN DEVICE MEMORY (the batch's device), for callers that feed them to the next device
   stage: am_replaced_get then returns device pointers, am_replaced_read copies one text to the host.  This is what a
   device-resident pipeline measures; am_replacer_run_batch additionally moves every result over PCIe into pinned host memory. */
AM_API int am_replacer_run_batch_device(const am_replacer* r, const am_batch* b, uint64_t max_length, am_replaced** out);
/* One pass only, for callers that keep sort / removeOverlap / replace (Replacer.hs:159-198) on their side: the fold
 * `prependMatch` (:252-260) with seed (minBound, []) and the given threshold per haystack.  best_out[i] = the best
 * priority below thresholds[i] among the matches of haystack i (INT64_MIN: none); *matches_out = every match that
 * carries it, as makeMatch (:264-274) builds them (start and length in code units of the haystack), in
 * (haystack, start) order = the order `sort` (:241) gives them.  Free with am_prio_matches_free. */
typedef struct am_prio_match {
    uint64_t start;
    uint64_t len;
    uint32_t haystack;
    uint32_t payload;    /* index into the payload table given to am_replacer_create */
} am_prio_match;
AM_API int am_run_priority(const am_replacer* r, const am_slice* hay, size_t n_hay, const int64_t* thresholds,
                    int64_t* best_out, am_prio_match** matches_out, size_t* n_matches_out);
AM_API void am_prio_matches_free(am_prio_match* m);
AM_API uint64_t am_replaced_size(const am_replaced* r);
/* Returns 1 and the text for `Just`, 0 for `Nothing` (longer than max_length), < 0 on error.  *ptr is owned by r. */
AM_API int am_replaced_get(const am_replaced* r, size_t i, const uint8_t** ptr, size_t* len);
AM_API int am_replaced_device(const am_replaced* r);               /* -1: the texts are in host memory; otherwise the device that holds them */
/* Copies text i into dst (host memory, cap bytes) wherever the result lives; *len = its length.  Returns like am_replaced_get. */
AM_API int am_replaced_read(const am_replaced* r, size_t i, uint8_t* dst, size_t cap, size_t* len);
AM_API uint64_t am_replaced_passes(const am_replaced* r);          /* scans that were needed (max over the batch) */
AM_API uint64_t am_replaced_scanned_bytes(const am_replaced* r);   /* haystack bytes scanned over all passes (after the first pass only windows around the replacements) */
AM_API uint64_t am_replaced_spliced_bytes(const am_replaced* r);   /* bytes of rewritten text produced over all passes */
AM_API void am_replaced_free(am_replaced* r);

/* ---- several GPUs ---------------------------------------------------------------------
 * Every handle lives on one device: an automaton / batch on the device that was current when it was made (or that its
 * memory belongs to: am_batch_from_device, am_automaton_from_image), results and replacers with their automaton.
 * Entry points make that device current for the calling thread while they run, so one process can drive all GPUs.
 *
 * am_multi spans the devices with RCCL.  The path shards trivially (independent haystacks, read-only automaton), so
 * the only traffic between devices is one broadcast of the flattened automaton over xGMI and an all-reduce of match
 * counts; match lists are concatenated on the host in haystack order.
 *   am_multi_create        one process drives devices 0..n-1 (ncclCommInitAll); n_devices = 0: all visible devices
 *   am_multi_create_rank   one process per GPU (ncclCommInitRank on the current device); the id comes from
 *                          am_multi_unique_id on one rank and reaches the others through the launcher
 * Reference shape of a foreign binding: benchmark/rust-ffi/app/Main.hs:28-45 (`foreign import ccall`, slices). */
typedef struct am_multi am_multi;
#define AM_UNIQUE_ID_BYTES 128
AM_API int am_multi_unique_id(uint8_t id_out[AM_UNIQUE_ID_BYTES]);
AM_API int am_multi_create(int n_devices, am_multi** out);
AM_API int am_multi_create_rank(int n_ranks, int rank, const uint8_t id[AM_UNIQUE_ID_BYTES], am_multi** out);
AM_API void am_multi_destroy(am_multi* m);
AM_API int am_multi_local_devices(const am_multi* m);     /* devices this process drives */
AM_API int am_multi_world_size(const am_multi* m);        /* devices in all */
AM_API int am_multi_device(const am_multi* m, int i);     /* HIP device id of local device i */
/* ncclBroadcast of the flattened image of `a` (held by global rank `root`; NULL in processes that do not hold the
 * root) to every device; autos_out[i] = a handle on local device i attached to its copy (am_automaton_destroy each). */
AM_API int am_multi_broadcast_automaton(am_multi* m, const am_automaton* a, int case_mode, int root, am_automaton** autos_out);
/* ncclAllReduce(sum) of `count` (<= 512) uint64 per device: values = local_devices x count, row i belongs to local
 * device i; every row holds the sums afterwards. */
AM_API int am_multi_allreduce_sum(am_multi* m, uint64_t* values, size_t count);
/* This process's haystacks cut into contiguous blocks, one per local device (block i = haystacks [n*i/D, n*(i+1)/D)),
 * scanned concurrently; counts_out (nullable) per haystack in order; *total_out = sum over ALL devices (all-reduce):
 * countMatches (benchmark/haskell/app/Main.hs:67-76) of the whole job. */
AM_API int am_multi_count(am_multi* m, am_automaton* const* autos, int case_mode, const am_slice* hay, size_t n_hay, uint64_t* counts_out, uint64_t* total_out);
/* runWithCase on every local device's block; the records of all blocks concatenated on the host in haystack order
 * (haystack = index into `hay`).  Free with am_multi_matches_free. */
AM_API int am_multi_run(am_multi* m, am_automaton* const* autos, int case_mode, const am_slice* hay, size_t n_hay, am_match** matches_out, size_t* n_out);
AM_API void am_multi_matches_free(am_match* p);
/* The same on DEVICE-RESIDENT batches: batches[i] lives on local device i (made there by am_batch_upload or
 * am_batch_from_device; NULL = no work for that device); one host thread and stream per device; nothing but the counts
 * leaves the devices.  BASELINE configs[3] (100 GiB of haystacks spread over the HBM of 8 GPUs) from a C / Haskell host.
 *   am_multi_count_batch  counts_out (nullable; then one nullable array of batch-i-many counts per local device);
 *                         local_totals_out (nullable): one sum per local device; *total_out: all devices (all-reduce)
 *   am_multi_run_batch    results_out[i] = the records of batch i, left in device i's HBM (am_matches_free each);
 *                         *total_records_out = records on all devices (all-reduce)
 * Error behaviour of every am_multi_* collective: a failure on one device is carried into the collective as a flag, so
 * every rank returns (none blocks) and every rank returns an error. */
/* am_batch_upload onto local device i of m (a host without HIP of its own has no other way to choose the device). */
AM_API int am_multi_batch_upload(const am_multi* m, int local_device, const am_slice* hay, size_t n_hay, am_batch** out);
AM_API int am_multi_count_batch(am_multi* m, am_automaton* const* autos, int case_mode, am_batch* const* batches, uint64_t* const* counts_out,
                         uint64_t* local_totals_out, uint64_t* total_out);
AM_API int am_multi_run_batch(am_multi* m, am_automaton* const* autos, int case_mode, am_batch* const* batches, am_matches** results_out, uint64_t* total_records_out);

/* ONE haystack on all devices ("a single huge haystack splits into G ranges with maxNeedleCodePoints overlap"; BASELINE configs[1]
 * shape (i), 1 x 1 GiB): global device g of W owns the end positions in (len * g / W, len * (g + 1) / W] (am_run_range on its own device).
 * Every process passes the WHOLE haystack; each device uploads only its window of it.
 *   am_multi_count_single  local_counts_out (nullable): one count per local device; *total_out: the whole haystack (all-reduce)
 *   am_multi_run_single    *matches_out = the records of this process's ranges in position order (haystack = 0, end_pos relative to the whole
 *                          haystack; am_multi_matches_free); with one process per GPU the launcher concatenates the ranks' arrays in rank
 *                          order.  *total_records_out (nullable) = records on all devices. */
AM_API int am_multi_count_single(am_multi* m, am_automaton* const* autos, int case_mode, const am_slice* hay, uint64_t* local_counts_out, uint64_t* total_out);
AM_API int am_multi_run_single(am_multi* m, am_automaton* const* autos, int case_mode, const am_slice* hay, am_match** matches_out, size_t* n_out, uint64_t* total_records_out);

/* ---- multi-GPU: move the flattened automaton between devices -----------------------------------
 * The image is one position-independent blob, so rank 0 flattens once and the blob is broadcast
 * over xGMI (RCCL broadcast of a byte tensor); every other rank attaches to its received copy. */
AM_API int am_automaton_image_size(const am_automaton* a, int case_mode, size_t* nbytes);
AM_API int am_automaton_image_copy(const am_automaton* a, int case_mode, void* d_dst, size_t nbytes);   /* device -> device */
AM_API int am_automaton_from_image(const void* d_image, size_t nbytes, am_automaton** out);            /* copies the blob; TRUSTED input: a blob made by am_automaton_image_copy in this job (header checked only) */
/* Serialised automaton: the same blob in host memory (write it to a file as is).  Loading checks the
 * header (magic, version, every section inside the blob), a checksum of the body and every index the kernels
 * follow (states, node and edge ids, table slots), so a truncated, damaged or stale file is refused with
 * AM_ERR_INVALID; it skips build + flatten entirely (the reference's JSON instances store only
 * the needles and rebuild, Searcher.hs:68-77).  A handle made from an image serves the image's case mode. */
AM_API int am_automaton_image_read(const am_automaton* a, int case_mode, void* host_dst, size_t nbytes);   /* device -> host */
AM_API int am_automaton_from_host_image(const void* image, size_t nbytes, am_automaton** out);

/* ---- UTF-8 helpers on the path -------------------------------------------------------------------
 * am_lower_code_point: Utf8.lowerCodePoint (src/Data/Text/Utf8.hs:145-151) with the BUILT-IN table: simple mapping of
 * Unicode 14.0 (am_unicode_version() = 0x0E00: major << 8 | minor).  The reference uses GHC base's Data.Char.toLower, whose
 * Unicode version follows the compiler: a caller that needs exactly its own hands its table to am_automaton_create_ex; a
 * flattened image carries the table it was baked with and a hash of it (am_automaton_lower_hash).
 * am_unlower_code_point: Utf8.unlowerCodePoint (src/Data/Text/Utf8/Unlower.hs:26-28) as an ascending set, built-in table;
 * returns the set size (may exceed cap).
 * am_image_version: layout version of the flattened image (am_automaton_image_*); images of another version are refused. */
AM_API uint32_t am_lower_code_point(uint32_t cp);
AM_API uint32_t am_unicode_version(void);
AM_API uint32_t am_image_version(void);
AM_API size_t am_unlower_code_point(uint32_t cp, uint32_t* out, size_t cap);

/* ---- runtime knobs ------------------------------------------------------------------------------ */
AM_API int am_set_stream(void* hip_stream);   /* hipStream_t for all subsequent launches OF THE CALLING THREAD; NULL = the thread's library stream */
AM_API int am_get_stream(void** hip_stream);  /* the stream the calling thread's launches on the current device go to (to order other work after them) */
AM_API int am_device_info(int* n_cu, size_t* hbm_bytes, char* name, size_t name_cap);
/* Host blocks of large results are the library's own (am_matches_data); one freed block -- page-locked, up to 1 GiB -- is kept for the next
 * large result, and so is one pageable block of a result beyond that (up to 8 GiB: its pages are there, the next result of that size is
 * copied into it at the speed of the wire).  This gives both back to the system now (page-locked memory is a shared, limited resource). */
AM_API int am_release_host_memory(void);
/* Device memory the library keeps between calls: up to four device arrays of freed results per device (16 GiB in all) and, per calling thread and device, the
 * one-shot batch of am_run / am_count / am_contains_any (text + workspaces, up to a sixteenth of the device's memory) -- freeing VRAM is not free (the driver wipes it
 * on the engines the host copies use), so arrays that will be wanted again are kept.  This frees the kept result arrays of every device and the CALLING thread's
 * one-shot batches now. */
AM_API int am_release_device_memory(void);
/* Per-kernel timing with HIP events on the launch stream (off by default). */
AM_API int am_profile_enable(int on);
AM_API int am_profile_reset(void);
AM_API int am_profile_read(const char* kernel /* "sf" | "ac" | "hidx" | "scan" | "permute" | "rp_pass" | "rp_splice" | ... */, double* total_ms, uint64_t* launches);

#ifdef __cplusplus
}
#endif
#endif /* AM_H */
