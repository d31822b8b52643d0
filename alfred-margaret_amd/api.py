"""ctypes front-end over libam.so (C ABI, include/am.h) and libam_host.so (C++ host mirror).

The classes mirror the reference modules (same names and argument meaning):
  Automaton  ~ Data.Text.AhoCorasick.Automaton  (build, run_with_case / run_text / run_lower, count_matches)
  Searcher   ~ Data.Text.AhoCorasick.Searcher   (build, contains_any, contains_all, set_case_sensitivity)
  Replacer   ~ Data.Text.AhoCorasick.Replacer   (build, run, run_with_limit)
  Splitter   ~ Data.Text.AhoCorasick.Splitter   (build, split, split_ignore_case; split_batch_device / fragments_batch / lines_batch: the fold on the device)
Every match position comes from the HIP kernels; there is no Python or CPU matching path, and
importing this module fails loudly if the native libraries are missing and cannot be built.
"""
import ctypes as C
import os

import numpy as np

from . import build as _build

CASE_SENSITIVE = 0
IGNORE_CASE = 1

AM_OK = 0
AM_ERR_INVALID, AM_ERR_NO_DEVICE, AM_ERR_HIP, AM_ERR_OOM, AM_ERR_UNSUPPORTED = -1, -2, -3, -4, -5


class AmError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("libam error %d: %s" % (code, msg))
        self.code = code


class _Match:
    """am.MATCH: the segment of a substitution template that stands for the matched text itself (AM_SEG_MATCH) -- sed's &."""
    __slots__ = ()

    def __repr__(self):
        return "am.MATCH"


MATCH = _Match()


class Slice(C.Structure):          # am_slice
    _fields_ = [("ptr", C.c_void_p), ("off", C.c_size_t), ("len", C.c_size_t)]


MATCH_DTYPE = np.dtype([("end_pos", np.uint64), ("haystack", np.uint32), ("state", np.uint32)])   # am_match
FRAGMENT_DTYPE = np.dtype([("start", np.uint64), ("len", np.uint64)])   # am_fragment
NEEDLE_COUNT_DTYPE = np.dtype([("count", np.uint64), ("needle", np.uint32), ("haystack", np.uint32)])   # am_needle_count
SPAN_DTYPE = np.dtype([("start", np.uint64), ("len", np.uint64), ("haystack", np.uint32), ("needle", np.uint32)])   # am_span
RULE_NEGATE = 0x80000000
RULE_NONE = 0xFFFFFFFF               # the label of a haystack on which no rule fires
RULE_FIRED, RULE_FIRST = 0, 1
SCORED_DTYPE = np.dtype([("score", np.int64), ("haystack", np.uint32), ("reserved", np.uint32)])   # am_scored
SCORE_MAX_COLUMNS = 8                # AM_SCORE_MAX_COLUMNS
NEAR_QUERY_DTYPE = np.dtype([("group_a", np.uint32), ("group_b", np.uint32), ("flags", np.uint32), ("reserved", np.uint32), ("max_gap", np.uint64)])   # am_near_query
NEAR_PAIR_DTYPE = np.dtype([("a", np.uint64), ("b", np.uint64), ("gap", np.uint64), ("haystack", np.uint32), ("query", np.uint32)])   # am_near_pair
NEAR_MAX_GROUPS, NEAR_MAX_QUERIES, NEAR_ORDERED = 32, 64, 1          # AM_NEAR_MAX_GROUPS, AM_NEAR_MAX_QUERIES, AM_NEAR_ORDERED
NEAR_ANYWHERE = 2 ** 64 - 1          # a max_gap that every pair of one haystack meets
SPANS_ALL = 0
SPANS_LEFTMOST_LONGEST = 1
SPAN_TABLE_WORDS = 1                 # AM_SPAN_TABLE_WORDS: a flag of am_span_table_create_cased
SUBST_MAX_SEGMENTS, SEG_LITERAL, SEG_MATCH = 64, 0, 1          # AM_SUBST_MAX_SEGMENTS, AM_SEG_LITERAL, AM_SEG_MATCH
EXTRACT_EACH = 0
EXTRACT_MERGED = 1
BYTES, CODE_POINTS, UTF16 = 0, 1, 2                          # AM_UNIT_*: what start / len / columns / positions are counted in
COORDS_CODE_POINTS, COORDS_UTF16, COORDS_LINES = 1, 2, 4     # AM_COORDS_*: which prefixes a Coords index carries
SPAN_RANGE_DTYPE = np.dtype([("start_line", np.uint64), ("start_col", np.uint64), ("end_line", np.uint64), ("end_col", np.uint64)])   # am_span_range
PRIO_MATCH_DTYPE = np.dtype([("start", np.uint64), ("len", np.uint64), ("haystack", np.uint32), ("payload", np.uint32)])   # am_prio_match

_u8p, _u32p, _u64p = C.POINTER(C.c_uint8), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
_vp, _sz = C.c_void_p, C.c_size_t

# name -> (restype, argtypes): every symbol include/am.h declares
ABI = {
    "am_last_error": (C.c_char_p, []),
    "am_automaton_create": (C.c_int, [_vp, _sz, _vp, _sz, _vp, _vp, C.POINTER(_vp)]),
    "am_automaton_create_ex": (C.c_int, [_vp, _sz, _vp, _sz, _vp, _vp, _vp, _vp, _sz, C.POINTER(_vp)]),
    "am_automaton_lower_hash": (C.c_uint32, [_vp]),
    "am_lower_table_hash": (C.c_uint32, [_vp, _vp, _sz]),
    "am_automaton_destroy": (None, [_vp]),
    "am_automaton_set_kernel": (C.c_int, [_vp, C.c_int]),
    "am_count": (C.c_int, [_vp, C.c_int, C.POINTER(Slice), _sz, _vp]),
    "am_contains_any": (C.c_int, [_vp, C.c_int, C.POINTER(Slice), _sz, _vp]),
    "am_run": (C.c_int, [_vp, C.c_int, C.POINTER(Slice), _sz, C.POINTER(_vp)]),
    "am_run_range": (C.c_int, [_vp, C.c_int, C.POINTER(Slice), C.c_uint64, C.c_uint64, C.POINTER(_vp)]),
    "am_count_range": (C.c_int, [_vp, C.c_int, C.POINTER(Slice), C.c_uint64, C.c_uint64, _u64p]),
    "am_batch_upload": (C.c_int, [C.POINTER(Slice), _sz, C.POINTER(_vp)]),
    "am_batch_from_device": (C.c_int, [_vp, _vp, _sz, C.c_uint64, C.POINTER(_vp)]),
    "am_batch_destroy": (None, [_vp]),
    "am_batch_total_bytes": (C.c_uint64, [_vp]),
    "am_count_batch": (C.c_int, [_vp, C.c_int, _vp, _vp, _u64p]),
    "am_contains_any_batch": (C.c_int, [_vp, C.c_int, _vp, _vp]),
    "am_run_batch": (C.c_int, [_vp, C.c_int, _vp, C.POINTER(_vp)]),
    "am_matches_size": (C.c_uint64, [_vp]),
    "am_matches_data": (_vp, [_vp]),
    "am_matches_device_data": (_vp, [_vp]),
    "am_matches_haystack_range": (C.c_int, [_vp, C.c_uint32, _u64p, _u64p]),
    "am_matches_copy": (C.c_int, [_vp, C.c_uint64, C.c_uint64, _vp]),
    "am_matches_free": (None, [_vp]),
    "am_matches_fold_hash": (C.c_int, [_vp, _vp, _sz, _vp, _vp]),
    "am_count_by_needle_batch": (C.c_int, [_vp, C.c_int, _vp, _vp]),
    "am_count_by_needle": (C.c_int, [_vp, C.c_int, C.POINTER(Slice), _sz, _vp]),
    "am_matches_count_by_needle": (C.c_int, [_vp, _vp, _vp]),
    "am_count_matrix_batch": (C.c_int, [_vp, C.c_int, _vp, C.POINTER(_vp)]),
    "am_count_matrix": (C.c_int, [_vp, C.c_int, C.POINTER(Slice), _sz, C.POINTER(_vp)]),
    "am_matches_count_matrix": (C.c_int, [_vp, _vp, _sz, C.POINTER(_vp)]),
    "am_needle_matrix_size": (C.c_uint64, [_vp]),
    "am_needle_matrix_haystacks": (C.c_uint64, [_vp]),
    "am_needle_matrix_offsets": (_vp, [_vp]),
    "am_needle_matrix_data": (_vp, [_vp]),
    "am_needle_matrix_device_offsets": (_vp, [_vp]),
    "am_needle_matrix_device_data": (_vp, [_vp]),
    "am_needle_matrix_free": (None, [_vp]),
    "am_splitter_create": (C.c_int, [_vp, C.c_uint32, C.c_uint32, C.POINTER(_vp)]),
    "am_splitter_destroy": (None, [_vp]),
    "am_split_batch": (C.c_int, [_vp, C.c_int, _vp, C.POINTER(_vp)]),
    "am_split": (C.c_int, [_vp, C.c_int, C.POINTER(Slice), _sz, C.POINTER(_vp)]),
    "am_fragments_size": (C.c_uint64, [_vp]),
    "am_fragments_haystacks": (C.c_uint64, [_vp]),
    "am_fragments_offsets": (_vp, [_vp]),
    "am_fragments_data": (_vp, [_vp]),
    "am_fragments_device_offsets": (_vp, [_vp]),
    "am_fragments_device_data": (_vp, [_vp]),
    "am_fragments_free": (None, [_vp]),
    "am_batch_from_fragments": (C.c_int, [_vp, _vp, C.POINTER(_vp)]),
    "am_span_table_create": (C.c_int, [_vp, _vp, _vp, C.POINTER(_vp)]),
    "am_span_table_destroy": (None, [_vp]),
    "am_word_bytes_default": (None, [_vp]),
    "am_span_table_create_words": (C.c_int, [_vp, _vp, _vp, _vp, C.POINTER(_vp)]),
    "am_span_table_word_bytes": (C.c_int, [_vp, _vp]),
    "am_span_table_create_cased": (C.c_int, [_vp, _vp, _vp, C.c_uint32, _vp, _vp, _vp, C.POINTER(_vp)]),
    "am_span_table_check_exact": (C.c_int, [_vp, _vp, C.c_uint32, _vp, _vp]),
    "am_span_table_exact": (C.c_int, [_vp, C.c_uint32, C.POINTER(_vp), _u64p]),
    "am_count_spans_by_needle_batch": (C.c_int, [_vp, C.c_int, _vp, _vp]),
    "am_count_spans_by_needle": (C.c_int, [_vp, C.c_int, C.POINTER(Slice), _sz, _vp]),
    "am_spans_batch": (C.c_int, [_vp, C.c_int, C.c_int, _vp, C.POINTER(_vp)]),
    "am_spans": (C.c_int, [_vp, C.c_int, C.c_int, C.POINTER(Slice), _sz, C.POINTER(_vp)]),
    "am_spans_size": (C.c_uint64, [_vp]),
    "am_spans_haystacks": (C.c_uint64, [_vp]),
    "am_spans_offsets": (_vp, [_vp]),
    "am_spans_data": (_vp, [_vp]),
    "am_spans_device_offsets": (_vp, [_vp]),
    "am_spans_device_data": (_vp, [_vp]),
    "am_spans_rounds": (C.c_uint32, [_vp]),
    "am_spans_free": (None, [_vp]),
    "am_subst_table_create": (C.c_int, [_vp, _vp, _vp, C.POINTER(_vp)]),
    "am_subst_table_create_templates": (C.c_int, [_vp, _vp, _vp, _vp, _vp, C.POINTER(_vp)]),
    "am_subst_table_destroy": (None, [_vp]),
    "am_batch_substitute": (C.c_int, [_vp, _vp, _vp, C.POINTER(_vp)]),
    "am_substitute_batch": (C.c_int, [_vp, C.c_int, _vp, C.POINTER(_vp), C.POINTER(_vp)]),
    "am_substitute": (C.c_int, [_vp, C.c_int, C.POINTER(Slice), _sz, C.POINTER(_vp)]),
    "am_substitute_geometry": (None, [_u32p, _u32p]),
    "am_batch_haystacks": (C.c_uint64, [_vp]),
    "am_batch_device_text": (_vp, [_vp]),
    "am_batch_device_offsets": (_vp, [_vp]),
    "am_batch_read_offsets": (C.c_int, [_vp, _vp]),
    "am_batch_read_text": (C.c_int, [_vp, C.c_uint64, C.c_uint64, _vp]),
    "am_select_any_batch": (C.c_int, [_vp, C.c_int, C.c_int, _vp, C.POINTER(_vp)]),
    "am_select_all_batch": (C.c_int, [_vp, C.c_int, C.c_int, _vp, C.POINTER(_vp)]),
    "am_select_spans_batch": (C.c_int, [_vp, C.c_int, C.c_int, _vp, C.POINTER(_vp)]),
    "am_select_flags": (C.c_int, [_vp, _vp, C.c_int, C.POINTER(_vp)]),
    "am_select_any": (C.c_int, [_vp, C.c_int, C.c_int, C.POINTER(Slice), _sz, C.POINTER(_vp)]),
    "am_select_all": (C.c_int, [_vp, C.c_int, C.c_int, C.POINTER(Slice), _sz, C.POINTER(_vp)]),
    "am_selection_size": (C.c_uint64, [_vp]),
    "am_selection_source_haystacks": (C.c_uint64, [_vp]),
    "am_selection_total_bytes": (C.c_uint64, [_vp]),
    "am_selection_indices": (_vp, [_vp]),
    "am_selection_device_indices": (_vp, [_vp]),
    "am_selection_free": (None, [_vp]),
    "am_batch_from_selection": (C.c_int, [_vp, _vp, C.POINTER(_vp)]),
    "am_select_geometry": (None, [_u32p, _u32p]),
    "am_rules_create": (C.c_int, [_vp, _vp, _vp, _vp, C.c_uint32, C.POINTER(_vp)]),
    "am_rules_destroy": (None, [_vp]),
    "am_rules_eval_batch": (C.c_int, [_vp, C.c_int, _vp, C.POINTER(_vp)]),
    "am_rules_eval": (C.c_int, [_vp, C.c_int, C.POINTER(Slice), _sz, C.POINTER(_vp)]),
    "am_rule_hits_haystacks": (C.c_uint64, [_vp]),
    "am_rule_hits_rules": (C.c_uint64, [_vp]),
    "am_rule_hits_hay_words": (C.c_uint64, [_vp]),
    "am_rule_hits_fired": (_vp, [_vp]),
    "am_rule_hits_labels": (_vp, [_vp]),
    "am_rule_hits_counts": (_vp, [_vp]),
    "am_rule_hits_device_fired": (_vp, [_vp]),
    "am_rule_hits_device_labels": (_vp, [_vp]),
    "am_rule_hits_device_counts": (_vp, [_vp]),
    "am_rule_hits_free": (None, [_vp]),
    "am_select_rule": (C.c_int, [_vp, C.c_uint32, C.c_int, C.c_int, _vp, C.POINTER(_vp)]),
    "am_rules_geometry": (None, [_u32p, _u32p, _u32p]),
    "am_weights_create": (C.c_int, [_vp, _vp, C.c_uint32, C.POINTER(_vp)]),
    "am_weights_destroy": (None, [_vp]),
    "am_score_batch": (C.c_int, [_vp, C.c_int, _vp, C.POINTER(_vp)]),
    "am_score": (C.c_int, [_vp, C.c_int, C.POINTER(Slice), _sz, C.POINTER(_vp)]),
    "am_score_spans_batch": (C.c_int, [_vp, _vp, C.c_int, _vp, C.POINTER(_vp)]),
    "am_matches_score": (C.c_int, [_vp, _vp, _sz, C.POINTER(_vp)]),
    "am_scores_haystacks": (C.c_uint64, [_vp]),
    "am_scores_columns": (C.c_uint64, [_vp]),
    "am_scores_data": (_vp, [_vp]),
    "am_scores_device_data": (_vp, [_vp]),
    "am_scores_free": (None, [_vp]),
    "am_scores_top_k": (C.c_int, [_vp, C.c_uint32, C.c_uint64, C.c_int, _vp, _u64p]),
    "am_select_top_k": (C.c_int, [_vp, C.c_uint32, C.c_uint64, C.c_int, _vp, C.POINTER(_vp)]),
    "am_select_score": (C.c_int, [_vp, C.c_uint32, C.c_int64, C.c_int64, C.c_int, _vp, C.POINTER(_vp)]),
    "am_score_geometry": (None, [_u32p, _u32p]),
    "am_near_create": (C.c_int, [_vp, _vp, _vp, C.c_uint32, C.POINTER(_vp)]),
    "am_near_destroy": (None, [_vp]),
    "am_near_spans": (C.c_int, [_vp, _vp, C.POINTER(_vp)]),
    "am_near_batch": (C.c_int, [_vp, C.c_int, _vp, C.POINTER(_vp), C.POINTER(_vp)]),
    "am_near": (C.c_int, [_vp, C.c_int, C.POINTER(Slice), _sz, C.POINTER(_vp), C.POINTER(_vp)]),
    "am_near_hits_size": (C.c_uint64, [_vp]),
    "am_near_hits_haystacks": (C.c_uint64, [_vp]),
    "am_near_hits_queries": (C.c_uint64, [_vp]),
    "am_near_hits_hay_words": (C.c_uint64, [_vp]),
    "am_near_hits_offsets": (_vp, [_vp]),
    "am_near_hits_data": (_vp, [_vp]),
    "am_near_hits_fired": (_vp, [_vp]),
    "am_near_hits_counts": (_vp, [_vp]),
    "am_near_hits_device_offsets": (_vp, [_vp]),
    "am_near_hits_device_data": (_vp, [_vp]),
    "am_near_hits_device_fired": (_vp, [_vp]),
    "am_near_hits_device_counts": (_vp, [_vp]),
    "am_near_hits_free": (None, [_vp]),
    "am_select_near": (C.c_int, [_vp, C.c_uint32, C.c_int, _vp, C.POINTER(_vp)]),
    "am_near_geometry": (None, [_u32p, _u32p]),
    "am_fragments_from_spans": (C.c_int, [_vp, _vp, C.c_uint32, C.c_uint32, C.c_int, C.POINTER(_vp)]),
    "am_extract_batch": (C.c_int, [_vp, C.c_int, C.c_int, C.c_uint32, C.c_uint32, C.c_int, _vp, C.POINTER(_vp), C.POINTER(_vp)]),
    "am_extract": (C.c_int, [_vp, C.c_int, C.c_int, C.c_uint32, C.c_uint32, C.c_int, C.POINTER(Slice), _sz, C.POINTER(_vp), C.POINTER(_vp)]),
    "am_coords_create": (C.c_int, [_vp, C.c_uint32, C.POINTER(_vp)]),
    "am_coords_destroy": (None, [_vp]),
    "am_coords_index_bytes": (C.c_uint64, [_vp]),
    "am_coords_spans": (C.c_int, [_vp, _vp, C.c_int, C.POINTER(_vp)]),
    "am_coords_fragments": (C.c_int, [_vp, _vp, C.c_int, C.POINTER(_vp)]),
    "am_coords_ranges": (C.c_int, [_vp, _vp, C.c_int, C.POINTER(_vp)]),
    "am_ranges_size": (C.c_uint64, [_vp]),
    "am_ranges_haystacks": (C.c_uint64, [_vp]),
    "am_ranges_offsets": (_vp, [_vp]),
    "am_ranges_data": (_vp, [_vp]),
    "am_ranges_device_offsets": (_vp, [_vp]),
    "am_ranges_device_data": (_vp, [_vp]),
    "am_ranges_free": (None, [_vp]),
    "am_coords_positions": (C.c_int, [_vp, _vp, _vp, C.c_uint64, C.c_int, _vp]),
    "am_coords_positions_device": (C.c_int, [_vp, _vp, _vp, C.c_uint64, C.c_int, _vp]),
    "am_postings_from_spans": (C.c_int, [_vp, C.POINTER(_vp)]),
    "am_postings_batch": (C.c_int, [_vp, C.c_int, C.c_int, _vp, C.POINTER(_vp)]),
    "am_postings": (C.c_int, [_vp, C.c_int, C.c_int, C.POINTER(Slice), _sz, C.POINTER(_vp)]),
    "am_postings_size": (C.c_uint64, [_vp]),
    "am_postings_needles": (C.c_uint64, [_vp]),
    "am_postings_haystacks": (C.c_uint64, [_vp]),
    "am_postings_offsets": (_vp, [_vp]),
    "am_postings_data": (_vp, [_vp]),
    "am_postings_source": (_vp, [_vp]),
    "am_postings_doc_freq": (_vp, [_vp]),
    "am_postings_device_offsets": (_vp, [_vp]),
    "am_postings_device_data": (_vp, [_vp]),
    "am_postings_device_source": (_vp, [_vp]),
    "am_postings_device_doc_freq": (_vp, [_vp]),
    "am_postings_free": (None, [_vp]),
    "am_spans_of_needle": (C.c_int, [_vp, C.c_uint32, C.POINTER(_vp)]),
    "am_postings_geometry": (None, [C.c_uint64, _u32p, _u32p, _u32p, _u32p]),
    "am_needle_ids_create": (C.c_int, [_vp, _vp, _vp, C.c_uint32, C.POINTER(_vp)]),
    "am_needle_ids_destroy": (None, [_vp]),
    "am_contains_all": (C.c_int, [_vp, C.c_int, C.POINTER(Slice), _sz, _vp]),
    "am_contains_all_batch": (C.c_int, [_vp, C.c_int, _vp, _vp]),
    "am_replacer_create": (C.c_int, [_vp, C.c_int, _vp, _vp, _vp, _sz, _vp, _sz, C.c_int64, C.POINTER(_vp)]),
    "am_replacer_destroy": (None, [_vp]),
    "am_replacer_run": (C.c_int, [_vp, C.POINTER(Slice), _sz, C.c_uint64, C.POINTER(_vp)]),
    "am_replacer_run_batch": (C.c_int, [_vp, _vp, C.c_uint64, C.POINTER(_vp)]),
    "am_replacer_run_batch_device": (C.c_int, [_vp, _vp, C.c_uint64, C.POINTER(_vp)]),
    "am_replaced_device": (C.c_int, [_vp]),
    "am_replaced_read": (C.c_int, [_vp, _sz, _vp, _sz, C.POINTER(_sz)]),
    "am_run_priority": (C.c_int, [_vp, C.POINTER(Slice), _sz, _vp, _vp, C.POINTER(_vp), C.POINTER(_sz)]),
    "am_prio_matches_free": (None, [_vp]),
    "am_replaced_size": (C.c_uint64, [_vp]),
    "am_replaced_get": (C.c_int, [_vp, _sz, C.POINTER(_vp), C.POINTER(_sz)]),
    "am_replaced_passes": (C.c_uint64, [_vp]),
    "am_replaced_scanned_bytes": (C.c_uint64, [_vp]),
    "am_replaced_spliced_bytes": (C.c_uint64, [_vp]),
    "am_replaced_free": (None, [_vp]),
    "am_automaton_image_size": (C.c_int, [_vp, C.c_int, C.POINTER(_sz)]),
    "am_automaton_image_copy": (C.c_int, [_vp, C.c_int, _vp, _sz]),
    "am_automaton_from_image": (C.c_int, [_vp, _sz, C.POINTER(_vp)]),
    "am_automaton_image_read": (C.c_int, [_vp, C.c_int, _vp, _sz]),
    "am_automaton_from_host_image": (C.c_int, [_vp, _sz, C.POINTER(_vp)]),
    "am_multi_unique_id": (C.c_int, [_vp]),
    "am_multi_create": (C.c_int, [C.c_int, C.POINTER(_vp)]),
    "am_multi_create_rank": (C.c_int, [C.c_int, C.c_int, _vp, C.POINTER(_vp)]),
    "am_multi_destroy": (None, [_vp]),
    "am_multi_local_devices": (C.c_int, [_vp]),
    "am_multi_world_size": (C.c_int, [_vp]),
    "am_multi_device": (C.c_int, [_vp, C.c_int]),
    "am_multi_broadcast_automaton": (C.c_int, [_vp, _vp, C.c_int, C.c_int, C.POINTER(_vp)]),
    "am_multi_allreduce_sum": (C.c_int, [_vp, _vp, _sz]),
    "am_multi_count": (C.c_int, [_vp, C.POINTER(_vp), C.c_int, C.POINTER(Slice), _sz, _vp, _u64p]),
    "am_multi_run": (C.c_int, [_vp, C.POINTER(_vp), C.c_int, C.POINTER(Slice), _sz, C.POINTER(_vp), C.POINTER(_sz)]),
    "am_multi_matches_free": (None, [_vp]),
    "am_multi_batch_upload": (C.c_int, [_vp, C.c_int, C.POINTER(Slice), _sz, C.POINTER(_vp)]),
    "am_multi_count_batch": (C.c_int, [_vp, C.POINTER(_vp), C.c_int, C.POINTER(_vp), C.POINTER(_vp), _u64p, _u64p]),
    "am_multi_run_batch": (C.c_int, [_vp, C.POINTER(_vp), C.c_int, C.POINTER(_vp), C.POINTER(_vp), _u64p]),
    "am_multi_count_single": (C.c_int, [_vp, C.POINTER(_vp), C.c_int, C.POINTER(Slice), _u64p, _u64p]),
    "am_multi_run_single": (C.c_int, [_vp, C.POINTER(_vp), C.c_int, C.POINTER(Slice), C.POINTER(_vp), C.POINTER(_sz), _u64p]),
    "am_lower_code_point": (C.c_uint32, [C.c_uint32]),
    "am_unicode_version": (C.c_uint32, []),
    "am_image_version": (C.c_uint32, []),
    "am_unlower_code_point": (_sz, [C.c_uint32, _vp, _sz]),
    "am_set_stream": (C.c_int, [_vp]),
    "am_get_stream": (C.c_int, [C.POINTER(_vp)]),
    "am_device_info": (C.c_int, [C.POINTER(C.c_int), C.POINTER(_sz), C.c_char_p, _sz]),
    "am_release_host_memory": (C.c_int, []),
    "am_release_device_memory": (C.c_int, []),
    "am_profile_enable": (C.c_int, [C.c_int]),
    "am_profile_reset": (C.c_int, []),
    "am_profile_read": (C.c_int, [C.c_char_p, C.POINTER(C.c_double), _u64p]),
}

_HOST = {
    "amh_last_error": (C.c_char_p, []),
    "amh_build": (C.c_int, [C.c_char_p, _vp, _sz, _vp, C.POINTER(_vp)]),
    "amh_build_ex": (C.c_int, [C.c_char_p, _vp, _sz, _vp, _vp, _vp, _sz, C.POINTER(_vp)]),
    "amh_free": (None, [_vp]),
    "amh_num_states": (_sz, [_vp]),
    "amh_num_transitions": (_sz, [_vp]),
    "amh_transitions": (_u64p, [_vp]),
    "amh_offsets": (_u32p, [_vp]),
    "amh_root_ascii": (_u64p, [_vp]),
    "amh_values_off": (_u64p, [_vp]),
    "amh_values": (_u32p, [_vp]),
    "amh_device": (_vp, [_vp]),
    "amh_run_list": (C.c_int, [_vp, C.c_int, C.POINTER(Slice), _sz, _vp, _vp, _vp, C.c_uint64, _u64p]),
    "amh_count": (C.c_int, [_vp, C.c_int, C.POINTER(Slice), _sz, _vp]),
    "amh_count_by_needle": (C.c_int, [_vp, C.c_int, C.POINTER(Slice), _sz, _sz, _vp]),
    "amh_count_matrix": (C.c_int, [_vp, C.c_int, C.POINTER(Slice), _sz, _sz, C.POINTER(_vp), C.POINTER(_vp), _u64p]),
    "amh_spans_fold": (C.c_int, [C.c_int, C.c_int, _vp, _vp, _vp, C.c_uint64, C.POINTER(Slice), _sz, _vp, _vp, _sz, C.POINTER(_vp), C.POINTER(_vp), _u64p]),
    "amh_spans_fold_words": (C.c_int, [C.c_int, C.c_int, _vp, _vp, _vp, C.c_uint64, C.POINTER(Slice), _sz, _vp, _vp, _sz, _vp, C.POINTER(_vp), C.POINTER(_vp), _u64p]),
    "amh_spans": (C.c_int, [_vp, C.c_int, C.c_int, C.POINTER(Slice), _sz, _vp, _vp, _sz, C.POINTER(_vp), C.POINTER(_vp), _u64p]),
    "amh_spans_fold_cased": (C.c_int, [C.c_int, C.c_int, _vp, _vp, _vp, C.c_uint64, C.POINTER(Slice), _sz, _vp, _vp, _sz, _vp, _vp, _vp, C.POINTER(_vp), C.POINTER(_vp), _u64p]),
    "amh_spans_cased": (C.c_int, [_vp, C.c_int, C.c_int, C.POINTER(Slice), _sz, _vp, _vp, _sz, _vp, _vp, _vp, C.POINTER(_vp), C.POINTER(_vp), _u64p]),
    "amh_extract_fold": (C.c_int, [_vp, _vp, C.POINTER(Slice), _sz, C.c_uint32, C.c_uint32, C.c_int, C.POINTER(_vp), C.POINTER(_vp), _u64p]),
    "amh_rules_fold": (C.c_int, [_vp, _vp, C.c_uint64, _sz, _sz, _vp, _vp, _vp, C.c_uint32, _vp, _vp, _vp]),
    "amh_score": (C.c_int, [_vp, _vp, C.c_uint64, _sz, _sz, _vp, C.c_uint32, _vp]),
    "amh_near_fold": (C.c_int, [_vp, _vp, _sz, _vp, _sz, _vp, C.c_uint32, C.POINTER(_vp), C.POINTER(_vp), _u64p, _vp, _vp]),
    "amh_substitute_fold": (C.c_int, [C.c_int, _vp, _vp, _vp, C.c_uint64, C.POINTER(Slice), _sz, _vp, _vp, _sz, _vp, _vp, C.POINTER(_vp), _vp]),
    "amh_substitute_fold_words": (C.c_int, [C.c_int, _vp, _vp, _vp, C.c_uint64, C.POINTER(Slice), _sz, _vp, _vp, _sz, _vp, _vp, _vp, C.POINTER(_vp), _vp]),
    "amh_substitute_fold_cased": (C.c_int, [C.c_int, _vp, _vp, _vp, C.c_uint64, C.POINTER(Slice), _sz, _vp, _vp, _sz, _vp, _vp, _vp, _vp, _vp, C.POINTER(_vp), _vp]),
    "amh_substitute": (C.c_int, [_vp, C.c_int, C.POINTER(Slice), _sz, _vp, _vp, _sz, _vp, _vp, C.POINTER(_vp), _vp]),
    "amh_substitute_templates_fold": (C.c_int, [C.c_int, _vp, _vp, _vp, C.c_uint64, C.POINTER(Slice), _sz, _vp, _vp, _sz, _vp, _vp, _vp, _vp, _vp, C.POINTER(_vp), _vp]),
    "amh_substitute_templates": (C.c_int, [_vp, C.c_int, C.POINTER(Slice), _sz, _vp, _vp, _sz, _vp, _vp, _vp, _vp, C.POINTER(_vp), _vp]),
    "amh_searcher_build": (C.c_int, [C.c_int, C.c_char_p, _vp, _sz, C.POINTER(_vp)]),
    "amh_searcher_free": (None, [_vp]),
    "amh_searcher_set_case": (None, [_vp, C.c_int]),
    "amh_searcher_contains_any": (C.c_int, [_vp, C.POINTER(Slice), _sz, _vp]),
    "amh_searcher_contains_all": (C.c_int, [_vp, C.POINTER(Slice), _sz, _vp]),
    "amh_searcher_contains_all_host_fold": (C.c_int, [_vp, C.POINTER(Slice), _sz, _vp]),
    "amh_replacer_build": (C.c_int, [C.c_int, C.c_char_p, _vp, C.c_char_p, _vp, _sz, C.POINTER(_vp)]),
    "amh_replacer_build_ex": (C.c_int, [C.c_int, C.c_char_p, _vp, C.c_char_p, _vp, _sz, _vp, _vp, _sz, C.POINTER(_vp)]),
    "amh_replacer_free": (None, [_vp]),
    "amh_replacer_with_replacements": (C.c_int, [_vp, C.c_char_p, _vp, C.POINTER(_vp)]),
    "amh_replacer_set_case": (C.c_int, [_vp, C.c_int, C.POINTER(_vp)]),
    "amh_replacer_compose": (C.c_int, [_vp, _vp, C.POINTER(_vp)]),
    "amh_replacer_run_batch": (C.c_int, [_vp, C.POINTER(Slice), _sz, C.c_longlong, C.POINTER(_vp), _vp, _vp]),
    "amh_replacer_run_batch_host_splice": (C.c_int, [_vp, C.POINTER(Slice), _sz, C.c_longlong, C.POINTER(_vp), _vp, _vp]),
    "amh_replacer_last_stats": (None, [_vp, _vp, _vp]),
    "amh_replacer_device": (C.c_int, [_vp, C.POINTER(_vp)]),
    "amh_free_blob": (None, [_vp]),
    "amh_splitter_build": (C.c_int, [C.c_char_p, _sz, C.POINTER(_vp)]),
    "amh_splitter_free": (None, [_vp]),
    "amh_splitter_split_batch": (C.c_int, [_vp, C.c_int, C.POINTER(Slice), _sz, C.POINTER(_vp), C.POINTER(_vp), _u64p, _vp]),
    "amh_splitter_device": (C.c_int, [_vp, C.POINTER(_vp)]),
    "amh_splitter_automaton": (C.c_int, [_vp, C.POINTER(_vp)]),
    "amh_splitter_split_batch_device": (C.c_int, [_vp, C.c_int, C.POINTER(Slice), _sz, C.POINTER(_vp), C.POINTER(_vp), _u64p, _vp]),
    "amh_splitter_fragments_batch": (C.c_int, [_vp, C.c_int, C.POINTER(Slice), _sz, C.POINTER(_vp), C.POINTER(_vp), _u64p]),
    "amh_free_u64": (None, [_vp]),
    "amh_skip_code_points_backwards": (C.c_int64, [C.c_char_p, _sz, _sz, _sz]),
    "amh_lower_utf8": (_sz, [C.c_char_p, _sz, _vp, _sz]),
    "amh_is_case_invariant": (C.c_int, [C.c_char_p, _sz, _vp, _vp, _sz]),
    "amh_needle_casings": (C.c_int, [C.c_char_p, _sz, _vp, _vp, _sz, C.POINTER(_vp), C.POINTER(_vp), _u64p]),
}

# include/am_debug.h: tests and measurements only
DEBUG_ABI = {
    "am_debug_set": (C.c_int, [C.c_char_p, C.c_long]),
    "am_debug_pinned_bytes": (C.c_uint64, []),
    "am_debug_device_buffer_bytes": (C.c_uint64, []),
    "am_debug_bounds_report": (C.c_int, [_u64p, _u32p, _u32p]),
    "am_debug_sf_phase_cycles": (C.c_int, [_vp]),
    "am_debug_sf_wave_records": (C.c_int, [_vp, _sz]),
    "am_debug_resident_waves": (C.c_int, [_vp, _vp]),
    "am_debug_set_general_kernel": (C.c_int, [_vp, C.c_uint32]),
    "am_debug_rp_lds_haystacks": (C.c_uint32, []),
    "am_debug_hist_adds": (C.c_int, [_vp]),
    "am_debug_split_rounds": (C.c_uint32, []),
    "am_debug_needle_matrix_limits": (C.c_int, [_vp]),
    "am_debug_sf_unit_chunks": (C.c_uint32, [C.c_uint64, C.c_int]),
    "am_debug_sf_last_variant": (C.c_uint32, []),
}

_libam = None
_libhost = None
_libcheck = None


def _bind(lib, table):
    for name, (rt, at) in table.items():
        fn = getattr(lib, name)      # AttributeError = missing export: fail loudly
        fn.restype = rt
        fn.argtypes = at
    return lib


def libam():
    """The product library.  Built in-tree by build.py (hipcc --offload-arch=gfx950); never replaced by a fallback."""
    global _libam
    if _libam is None:
        path = os.path.join(_build.LIB, "libam.so")
        if not os.path.exists(path):
            path = _build.build_libam()
        _libam = _bind(_bind(C.CDLL(path, mode=C.RTLD_GLOBAL), ABI), DEBUG_ABI)
    return _libam


def load_check():
    """TEST INFRASTRUCTURE: loads libam_check.so (tests/native/am_ac.hip), which hands k_ac -- the general AC-walk kernel, the parity gate's
    independent second algorithm -- to libam; Automaton.set_kernel(1) works afterwards.  Called by tests/conftest.py, bench.py's parity gate
    and __graft_entry__.smoke(); nothing in this package calls it."""
    global _libcheck
    if _libcheck is None:
        libam()
        path = os.path.join(_build.LIB, "libam_check.so")
        if not os.path.exists(path):
            path = _build.build_check()
        lib = C.CDLL(path)
        lib.am_check_registered.restype = C.c_int
        if lib.am_check_registered() != 1:
            raise RuntimeError("libam_check.so could not register k_ac with libam (built against another image version?)")
        _libcheck = lib
    return _libcheck


def libhost():
    global _libhost
    if _libhost is None:
        libam()
        path = os.path.join(_build.LIB, "libam_host.so")
        if not os.path.exists(path):
            path = _build.build_host()
        _libhost = _bind(C.CDLL(path), _HOST)
    return _libhost


def check(rc):
    if rc != AM_OK:
        raise AmError(rc, (libam().am_last_error() or b"").decode("utf-8", "replace"))


def _hcheck(rc):
    if rc != AM_OK:
        raise AmError(rc, (libhost().amh_last_error() or b"").decode("utf-8", "replace"))


def _as_bytes(t):
    return t.encode("utf-8") if isinstance(t, str) else bytes(t)


def pack_texts(texts):
    bs = [_as_bytes(t) for t in texts]
    offs = np.zeros(len(bs) + 1, dtype=np.uint64)
    if bs:
        offs[1:] = np.cumsum(np.fromiter(map(len, bs), dtype=np.uint64, count=len(bs)))
    return b"".join(bs), offs


class _Slices:
    """Keeps the Python buffers alive while C borrows them.  Accepts str/bytes or (bytes, off, len)."""

    def __init__(self, texts):
        self.keep = []
        self.n = len(texts)
        self.arr = (Slice * max(self.n, 1))()
        for i, t in enumerate(texts):
            off, ln = 0, None
            if isinstance(t, tuple):
                t, off, ln = t
            if isinstance(t, np.ndarray):
                assert t.dtype == np.uint8 and t.flags["C_CONTIGUOUS"]
                ptr, size = t.ctypes.data, t.size
                self.keep.append(t)
            else:
                b = _as_bytes(t)
                buf = C.create_string_buffer(b, len(b) + 1)
                self.keep.append(buf)
                ptr, size = C.addressof(buf), len(b)
            self.arr[i] = Slice(ptr, off, size - off if ln is None else ln)


class _LowerArrays:
    """The caller's lower-case table as the two arrays the C ABI takes.  None = the built-in table (NULL, NULL, 0); an EMPTY list is a
    table of its own -- ASCII-only lower-casing -- and travels as two valid pointers with n = 0, as am_automaton_create_ex reads it."""

    def __init__(self, pairs):
        self.n = 0 if pairs is None else len(pairs)
        self.f = self.t = None
        if pairs is not None:
            self.f = np.zeros(max(self.n, 1), dtype=np.uint32)
            self.t = np.zeros(max(self.n, 1), dtype=np.uint32)
            for i, (a, b) in enumerate(pairs):
                self.f[i], self.t[i] = a, b
        self.from_ptr = None if self.f is None else self.f.ctypes.data
        self.to_ptr = None if self.t is None else self.t.ctypes.data


def lower_table_hash(pairs=None):
    la = _LowerArrays(pairs)
    return int(libam().am_lower_table_hash(la.from_ptr, la.to_ptr, la.n))


class Automaton:
    """AcMachine v with v = uint32 handles (needle index by default)."""

    def __init__(self, needles, values=None, lower_pairs=None):
        """lower_pairs: the caller's lower-casing as [(c, toLower c)] (am_automaton_create_ex); None = the built-in Unicode 14.0 table."""
        self.needles = [_as_bytes(n) for n in needles]            # (encoded once: 100k needles are 20 ms of the build per pass over them)
        blob, offs = pack_texts(self.needles)
        vptr = None
        if values is not None:
            self._vals = np.ascontiguousarray(values, dtype=np.uint32)
            vptr = self._vals.ctypes.data
        h = _vp()
        la = _LowerArrays(lower_pairs)
        _hcheck(libhost().amh_build_ex(blob, offs.ctypes.data, len(needles), vptr, la.from_ptr, la.to_ptr, la.n, C.byref(h)))
        self._h = h

    def _span_table(self, whole_words=False, n_needles=None):
        """The span table the methods below scan with: the needles' lengths and the word class where one is asked for.  The one place where they make a table:
        am.Cased's automaton overrides it to add its spellings."""
        return SpanTable(self, n_needles=n_needles, word_bytes=whole_words)

    def _needs_span_table(self, whole_words):
        """Whether a call has to go through a span table (a predicate decides its rows) or may take the route over the values alone."""
        return bool(whole_words)

    def _group_names(self):
        """The names by which near's groups refer to the needles."""
        return self.needles

    @property
    def lower_hash(self):
        return int(libam().am_automaton_lower_hash(self.device))

    @classmethod
    def build(cls, needles_with_values):
        """Automaton.hs:176 build :: [(Text, v)] -> AcMachine v (v = uint32)."""
        return cls([n for n, _ in needles_with_values], [v for _, v in needles_with_values])

    def __del__(self):
        if getattr(self, "_h", None):
            libhost().amh_free(self._h)
            self._h = None

    @property
    def device(self):
        return libhost().amh_device(self._h)

    @property
    def n_states(self):
        return libhost().amh_num_states(self._h)

    def transitions(self):
        return np.ctypeslib.as_array(libhost().amh_transitions(self._h), shape=(libhost().amh_num_transitions(self._h),)).copy()

    def offsets(self):
        return np.ctypeslib.as_array(libhost().amh_offsets(self._h), shape=(self.n_states + 1,)).copy()

    def root_ascii(self):
        return np.ctypeslib.as_array(libhost().amh_root_ascii(self._h), shape=(128,)).copy()

    def values_off(self):
        return np.ctypeslib.as_array(libhost().amh_values_off(self._h), shape=(self.n_states + 1,)).copy()

    def values(self):
        n = int(self.values_off()[-1])
        return np.ctypeslib.as_array(libhost().amh_values(self._h), shape=(n,)).copy() if n else np.zeros(0, np.uint32)

    def set_kernel(self, k):
        check(libam().am_automaton_set_kernel(self.device, k))

    def image_bytes(self, case):
        """The flattened automaton of one case mode as a serialisable blob (am_automaton_image_read)."""
        n = C.c_size_t(0)
        check(libam().am_automaton_image_size(self.device, case, C.byref(n)))
        buf = (C.c_uint8 * n.value)()
        check(libam().am_automaton_image_read(self.device, case, buf, n.value))
        return bytes(buf)

    def save_image(self, path, case):
        with open(path, "wb") as f:
            f.write(self.image_bytes(case))

    def run_batch_with_case(self, case, texts, unit=BYTES):
        """Per-haystack list fold of runWithCase: returns (haystack, matchPos, value) arrays in fold order.  unit: what matchPos is counted in -- BYTES (the
        reference's code units, the default) or CODE_POINTS / UTF16, converted in HBM (am_coords_positions)."""
        if unit != BYTES:
            hay, pos, val = self.run_batch_with_case(case, texts)
            with _Uploaded(texts) as b:
                return hay, Coords(b, utf16=unit == UTF16).positions(hay, pos, unit), val
        s = _Slices(texts)
        n = C.c_uint64(0)
        _hcheck(libhost().amh_run_list(self._h, case, s.arr, s.n, None, None, None, 0, C.byref(n)))
        k = int(n.value)
        hay, pos, val = np.zeros(max(k, 1), np.uint32), np.zeros(max(k, 1), np.uint64), np.zeros(max(k, 1), np.uint32)
        _hcheck(libhost().amh_run_list(self._h, case, s.arr, s.n, hay.ctypes.data, pos.ctypes.data, val.ctypes.data, k, C.byref(n)))
        return hay[:k], pos[:k], val[:k]

    def run_with_case(self, case, text):
        _, pos, val = self.run_batch_with_case(case, [text])
        return pos, val

    def run_text(self, text):
        return self.run_with_case(CASE_SENSITIVE, text)

    def run_lower(self, text):
        return self.run_with_case(IGNORE_CASE, text)

    def count_matches(self, case, texts):
        """countMatches (benchmark/haskell/app/Main.hs:67-76) per haystack."""
        s = _Slices(texts)
        out = np.zeros(max(s.n, 1), np.uint64)
        _hcheck(libhost().amh_count(self._h, case, s.arr, s.n, out.ctypes.data))
        return out[:s.n]

    def run_records(self, case, texts):
        """Raw am_match records straight from the C ABI (am_run)."""
        s = _Slices(texts)
        m = _vp()
        check(libam().am_run(self.device, case, s.arr, s.n, C.byref(m)))
        try:
            return matches_to_numpy(m)
        finally:
            libam().am_matches_free(m)

    def count_by_needle(self, case, texts, n_values=None):
        """How often every value is matched over all the texts: the fold `Map.insertWith (+) v 1` of runWithCase (Automaton.hs:442-553) as np.uint64[n], index = value
        handle, n = len(needles) unless given (handles >= n are skipped).  am_count_by_needle: scanned and folded in HBM, n counts come back."""
        n = len(self.needles) if n_values is None else int(n_values)
        if n == 0:
            return np.zeros(0, np.uint64)
        return ValuesTable(self, n).count_by_needle_texts(case, texts)

    def count_by_needle_host_mirror(self, case, texts, n_values=None):
        """The same through the C++ host mirror (host/automaton.hpp countByNeedle)."""
        n = len(self.needles) if n_values is None else int(n_values)
        s = _Slices(texts)
        out = np.zeros(max(n, 1), np.uint64)
        _hcheck(libhost().amh_count_by_needle(self._h, case, s.arr, s.n, n, out.ctypes.data))
        return out[:n]


    def count_matrix(self, case, texts, n_values=None):
        """Which values are matched in which text, and how often: (offsets np.uint64[len(texts) + 1], entries NEEDLE_COUNT_DTYPE[offsets[-1]]); row i =
        entries[offsets[i]:offsets[i + 1]] = Map.toAscList of the fold `Map.insertWith (+) v 1` of runWithCase (Automaton.hs:442-553) over texts[i], ascending by
        value, n = len(needles) unless given (handles >= n are skipped).  am_count_matrix: scanned and folded in HBM, the matrix comes back."""
        n = len(self.needles) if n_values is None else int(n_values)
        if n == 0:
            return np.zeros(len(texts) + 1, np.uint64), np.zeros(0, NEEDLE_COUNT_DTYPE)
        return ValuesTable(self, n).count_matrix_texts(case, texts)

    def count_matrix_host_mirror(self, case, texts, n_values=None):
        """The same through the C++ host mirror (host/automaton.hpp countMatrix)."""
        n = len(self.needles) if n_values is None else int(n_values)
        s = _Slices(texts)
        po, pe, ne = _vp(), _vp(), C.c_uint64(0)
        _hcheck(libhost().amh_count_matrix(self._h, case, s.arr, s.n, n, C.byref(po), C.byref(pe), C.byref(ne)))
        try:
            offs = np.frombuffer((C.c_char * ((s.n + 1) * 8)).from_address(po.value), dtype=np.uint64).copy()
            k = int(ne.value)
            ents = np.frombuffer((C.c_char * (k * 16)).from_address(pe.value), dtype=NEEDLE_COUNT_DTYPE).copy() if k else np.zeros(0, NEEDLE_COUNT_DTYPE)
        finally:
            libhost().amh_free_u64(po)
            libhost().amh_free_u64(pe)
        return offs, ents

    def score(self, case, texts, weights, whole_words=False, n_values=None):
        """A number per match, added up per text: np.int64[n_cols, len(texts)], scores[c, i] = the sum of weights[c][v] over every fold step `Match _ v` of
        runWithCase (Automaton.hs:442-553) over texts[i], modulo 2^64 -- the fold `acc + weight v`.  weights: one column (a flat list, one weight per value handle) or
        up to SCORE_MAX_COLUMNS of them.  am_score: scanned and summed in HBM, the scores come back.  whole_words: True (the default word class) or a class as
        SpanTable takes it -- only the whole-word occurrences add (include/am.h "whole words")."""
        n = len(self.needles) if n_values is None else int(n_values)
        if not self._needs_span_table(whole_words):
            return Weights(ValuesTable(self, n), weights).score_texts(case, texts).scores
        t = self._span_table(whole_words, n)
        w = Weights(t.values, weights)
        s = _Slices(texts)
        b = _vp()
        check(libam().am_batch_upload(s.arr, s.n, C.byref(b)))
        try:
            return t.score_batch(case, b, w).scores
        finally:
            libam().am_batch_destroy(b)

    def score_host_mirror(self, case, texts, weights, n_values=None):
        """The same through the C++ host mirror (host/automaton.hpp scoreByHaystack over the fold steps of amh_run_list)."""
        n = len(self.needles) if n_values is None else int(n_values)
        hay, _, val = self.run_batch_with_case(case, texts)
        return score_host(hay, val, len(texts), n, weights)

    def near(self, case, texts, groups, queries, whole_words=False):
        """Which matches lie near which (include/am.h "proximity"): groups = {"brand": [needles], "item": [needles]} over this automaton's needles (a needle may be in
        several groups or in none), queries = [("brand", "item", 20), ...] or NearQuery objects whose a / b are group names.  Per text a list with one list per query
        of (a_start, a_len, b_start, b_len, gap): every leftmost-longest match of group a whose nearest other match of group b lies at most max_gap bytes away.
        am_near: scanned, selected and joined in HBM; the pairs and the spans they index come back.  whole_words: as in spans."""
        names = list(groups)
        if len(names) > NEAR_MAX_GROUPS:
            raise AmError(AM_ERR_INVALID, "near: at most %d groups" % NEAR_MAX_GROUPS)
        member = {}
        for g, name in enumerate(names):
            for n in groups[name]:
                member[_as_bytes(n)] = member.get(_as_bytes(n), 0) | (1 << g)
        needle_names = self._group_names()
        known = set(_as_bytes(n) for n in needle_names)
        for n in member:
            if n not in known:
                raise AmError(AM_ERR_INVALID, "near: %r is in a group and not among the needles" % (n,))
        qs = []
        for q in queries:
            q = q if isinstance(q, NearQuery) else NearQuery(*q)
            if q.a not in groups or q.b not in groups:
                raise AmError(AM_ERR_INVALID, "near: a query names a group that is not given")
            qs.append(NearQuery(names.index(q.a), names.index(q.b), q.max_gap, q.ordered))
        t = self._span_table(whole_words)
        hits, (so, sp) = Near(t, [member.get(_as_bytes(n), 0) for n in needle_names], qs).near_texts(case, texts, spans=True)
        po, pairs = hits.offsets, hits.pairs
        out = []
        for i in range(len(texts)):
            rows = [[] for _ in qs]
            for r in pairs[int(po[i]):int(po[i + 1])]:
                a, b = sp[int(r["a"])], sp[int(r["b"])]
                rows[int(r["query"])].append((int(a["start"]), int(a["len"]), int(b["start"]), int(b["len"]), int(r["gap"])))
            out.append(rows)
        return out

    def postings(self, case, texts, leftmost_longest=False, whole_words=False):
        """Where each needle occurs (include/am.h "postings"): a Postings -- the spans of spans(case, texts, leftmost_longest, whole_words) ordered by needle, row v =
        the occurrences of needle v in (text, start) order, with the row of the spans each came from and the document frequencies.  am_postings: scanned, expanded,
        selected and sorted in HBM."""
        return self._span_table(whole_words).postings_texts(case, texts, SPANS_LEFTMOST_LONGEST if leftmost_longest else SPANS_ALL)

    def doc_freq(self, case, texts, whole_words=False):
        """In how many of the texts each needle occurs: np.uint64[len(needles)], the IDF half of TF-IDF (a Weights for score is made from it).  Over every
        occurrence (SPANS_ALL), with whole_words over the whole-word occurrences."""
        with self.postings(case, texts, whole_words=whole_words) as p:
            return p.doc_freq

    def concordance(self, case, texts, needle, before=0, after=0, leftmost_longest=True, whole_words=False):
        """Every occurrence of ONE needle among this dictionary's matches with up to `before` / `after` code points of its text around it, in (text, start) order: a
        list of bytes.  needle: one of the needles, or its index.  Postings, then the needle's row as spans (am_spans_of_needle), their windows
        (am_fragments_from_spans) and the gather (am_batch_from_fragments), all in HBM; the snippets come back.  Under leftmost_longest `he` inside `the` is no
        occurrence of `he` when `the` is a needle: a one-needle automaton cannot say that."""
        if isinstance(needle, (int, np.integer)) and not isinstance(needle, bool):
            v = int(needle)
        else:
            known = [_as_bytes(n) for n in self.needles]
            if _as_bytes(needle) not in known:
                raise AmError(AM_ERR_INVALID, "concordance: %r is not among the needles" % (needle,))
            v = known.index(_as_bytes(needle))
        t = self._span_table(whole_words)
        with _Uploaded(texts) as b, t.postings_batch(case, b, SPANS_LEFTMOST_LONGEST if leftmost_longest else SPANS_ALL) as p:
            row = p.spans_of(v, raw=True)
            try:
                fr = t.fragments_from_spans(b, row, before, after, False, raw=True)
            finally:
                libam().am_spans_free(row)
            nb = _vp()
            try:
                check(libam().am_batch_from_fragments(b, fr, C.byref(nb)))
            finally:
                libam().am_fragments_free(fr)
            try:
                return batch_to_bytes(nb)[1]
            finally:
                libam().am_batch_destroy(nb)

    def spans(self, case, texts, leftmost_longest=False, whole_words=False, unit=BYTES):
        """Where every match starts: (offsets np.uint64[len(texts) + 1], spans SPAN_DTYPE[offsets[-1]]); the spans of text i are spans[offsets[i]:offsets[i + 1]],
        start and len in bytes relative to the text, needle = the value handle.  All fold steps of runWithCase (Automaton.hs:442-553) in fold order with the span
        makeMatch gives them (Replacer.hs:264-274), or -- leftmost_longest -- the non-overlapping selection: smallest start, then longest, then smallest handle, never a
        zero-length span.  am_spans: scanned, expanded and selected in HBM.  whole_words: True (the default word class) or a class as SpanTable takes it -- only the
        spans whose neighbours inside the text are no word bytes, filtered BEFORE the selection (include/am.h "whole words").  unit: CODE_POINTS or UTF16 give start
        and len in that unit, converted in HBM (include/am.h "coordinates"): Automaton(["nike"]).spans(IGNORE_CASE, ["é NIKE"], unit=CODE_POINTS) has start 2, len 4."""
        mode = SPANS_LEFTMOST_LONGEST if leftmost_longest else SPANS_ALL
        if unit == BYTES:
            return self._span_table(whole_words).spans_texts(case, texts, mode)
        with _Uploaded(texts) as b:
            return self._span_table(whole_words).spans_batch(case, b, mode, unit=unit)

    def locate(self, case, texts, unit=CODE_POINTS, leftmost_longest=True, whole_words=False):
        """Where every match lies in its document, file:line:col: (offsets np.uint64[len(texts) + 1], spans SPAN_DTYPE in `unit`, ranges SPAN_RANGE_DTYPE) -- row k of
        ranges is the 0-based line and the column, in `unit`, of the start and of the end of span k (include/am.h "coordinates").  With unit=UTF16 a row is a
        Language-Server range.  Scanned, selected and converted in HBM."""
        t = self._span_table(whole_words)
        with _Uploaded(texts) as b:
            raw = t.spans_batch(case, b, SPANS_LEFTMOST_LONGEST if leftmost_longest else SPANS_ALL, raw=True)
            try:
                c = Coords(b, lines=True, utf16=unit == UTF16)
                offs, spans = c.spans(raw, unit)
                ranges = c.ranges(raw, unit)[1]
                del c                                       # (the batch outlives the index)
                return offs, spans, ranges
            finally:
                libam().am_spans_free(raw)

    def spans_host_mirror(self, case, texts, leftmost_longest=False, n_values=None, lengths=None):
        """The same through the C++ host mirror (host/spans.hpp spansFold over the fold steps of amh_run_list).  lengths: (len_bytes, len_code_points) per value handle
        where the handles are not the needle indices."""
        lb, lc = _handle_lengths(self.needles, n_values, lengths)
        nv = (len(self.needles) if lengths is None else len(lengths[0])) if n_values is None else int(n_values)
        s = _Slices(texts)
        po, pe, ne = _vp(), _vp(), C.c_uint64(0)
        _hcheck(libhost().amh_spans(self._h, case, SPANS_LEFTMOST_LONGEST if leftmost_longest else SPANS_ALL, s.arr, s.n, lb.ctypes.data, lc.ctypes.data, nv,
                                    C.byref(po), C.byref(pe), C.byref(ne)))
        return _take_spans(po, pe, s.n, int(ne.value))

    def substitute(self, case, texts, replacements, whole_words=False):
        """Every leftmost-longest match replaced once, replacements[v] for needle v, never scanned again (include/am.h "substitute"): a list of bytes, one per text.
        am_substitute: scanned, selected and spliced in HBM.  whole_words: as in spans -- the leftmost-longest WHOLE-WORD matches.  A replacement is bytes / str, or a
        TEMPLATE: a list or tuple of bytes / str / am.MATCH, where am.MATCH stands for the matched text as it is spelled in the haystack (include/am.h "substitute
        templates"): ["<b>", am.MATCH, "</b>"]."""
        return SubstTable(self._span_table(whole_words), replacements).substitute_texts(case, texts)

    def highlight(self, case, texts, before, after, whole_words=False):
        """Every leftmost-longest match wrapped: the template [before, am.MATCH, after] for every needle.  Under IGNORE_CASE the text keeps its own spelling:
        Automaton(["nike"]).highlight(IGNORE_CASE, ["NIKE shoe"], "<b>", "</b>") == [b"<b>NIKE</b> shoe"]."""
        return self.substitute(case, texts, [[before, MATCH, after]] * len(self.needles), whole_words=whole_words)

    def mask(self, case, texts, fill="*", whole_words=False):
        """Every leftmost-longest match overwritten, one `fill` per CODE POINT of the match: the fixed replacement fill * code_points(needle), through the plain table.
        This is exact per code point in both case modes: a span is made by makeMatch (Replacer.hs:264-274), which under CASE_SENSITIVE takes the needle's own bytes
        and under IGNORE_CASE walks back over exactly the needle's number of code points -- so a match always has as many code points as its needle, whatever its
        width in bytes (U+212A for k: three bytes, one code point, one `fill`)."""
        return self.substitute(case, texts, self.mask_replacements(fill), whole_words=whole_words)

    def mask_replacements(self, fill="*"):
        """The fixed replacements mask() uses: fill * code_points(needle) per needle."""
        fill = _as_bytes(fill)
        return [fill * len(_as_bytes(n).decode("utf-8")) for n in self.needles]

    def count_whole_words(self, case, texts, word_bytes=True):
        """How often every needle occurs as a whole word over all the texts: np.uint64[len(needles)], the bincount of the whole-word spans(..., whole_words=word_bytes)
        rows.  am_count_spans_by_needle: scanned, filtered and folded in HBM, the counts come back."""
        if not self.needles:
            return np.zeros(0, np.uint64)
        return SpanTable(self, word_bytes=word_bytes).count_by_needle_texts(case, texts)

    def grep(self, case, texts, invert=False, whole_words=False):
        """The texts that contain a needle -- `grep -F -f needles`; invert: `grep -v`; whole_words (True or a class as SpanTable takes it): `grep -w` -- as
        (indices np.uint32, [bytes]): the kept texts' indices, ascending, and the kept texts.  Decided and compacted in HBM (include/am.h "select")."""
        s = _Slices(texts)
        if not self._needs_span_table(whole_words):
            return _grep_texts(texts, _select(lambda out: libam().am_select_any(self.device, case, int(bool(invert)), s.arr, s.n, out)))
        t = self._span_table(whole_words)
        b = _vp()
        check(libam().am_batch_upload(s.arr, s.n, C.byref(b)))
        try:
            return _grep_texts(texts, t.select_batch(case, b, invert))
        finally:
            libam().am_batch_destroy(b)

    def extract(self, case, texts, before=0, after=0, merged=False, leftmost_longest=True, whole_words=False):
        """The matched text with up to `before` / `after` code points of its own text around it (include/am.h "extract"): a list of lists of bytes, one list per
        text -- a snippet per match (`grep -o` with context), or -- merged -- the union of overlapping and touching windows per text, as `grep -C` prints them
        (leftmost-longest matches only).  am_extract: scanned, selected, windowed and gathered in HBM.  whole_words: as in spans."""
        s = _Slices(texts)
        t = self._span_table(whole_words)
        nb, fr = _vp(), _vp()
        check(libam().am_extract(t.handle, case, SPANS_LEFTMOST_LONGEST if leftmost_longest else SPANS_ALL, int(before), int(after),
                                 EXTRACT_MERGED if merged else EXTRACT_EACH, s.arr, s.n, C.byref(nb), C.byref(fr)))
        try:
            offs = fragments_to_numpy(fr)[0]
            snippets = batch_to_bytes(nb)[1]
        finally:
            libam().am_fragments_free(fr)
            libam().am_batch_destroy(nb)
        return [snippets[int(offs[i]):int(offs[i + 1])] for i in range(len(offs) - 1)]

    def substitute_host_mirror(self, case, texts, replacements, n_values=None, lengths=None):
        """The same through the C++ host mirror (host/spans.hpp substitute over spansFold over the fold steps of amh_run_list)."""
        lb, lc = _handle_lengths(self.needles, n_values, lengths)
        nv = (len(self.needles) if lengths is None else len(lengths[0])) if n_values is None else int(n_values)
        pool, offs = _pack_replacements(replacements, nv)
        s = _Slices(texts)
        blob, out_offs = _vp(), np.zeros(s.n + 1, np.uint64)
        _hcheck(libhost().amh_substitute(self._h, case, s.arr, s.n, lb.ctypes.data, lc.ctypes.data, nv, pool, offs.ctypes.data, C.byref(blob), out_offs.ctypes.data))
        return _take_texts(blob, out_offs)


    def substitute_templates_host_mirror(self, case, texts, templates, n_values=None, lengths=None):
        """substitute with templates through the C++ host mirror (host/spans.hpp substituteTemplates over spansFold over the fold steps of amh_run_list)."""
        lb, lc = _handle_lengths(self.needles, n_values, lengths)
        nv = (len(self.needles) if lengths is None else len(lengths[0])) if n_values is None else int(n_values)
        seg_off, kind, lit_off, pool = _pack_templates(templates, nv)
        s = _Slices(texts)
        blob, out_offs = _vp(), np.zeros(s.n + 1, np.uint64)
        _hcheck(libhost().amh_substitute_templates(self._h, case, s.arr, s.n, lb.ctypes.data, lc.ctypes.data, nv, seg_off.ctypes.data, kind.ctypes.data, lit_off.ctypes.data,
                                                   pool or None, C.byref(blob), out_offs.ctypes.data))
        return _take_texts(blob, out_offs)


def _is_template(x):
    return isinstance(x, (list, tuple))


def _pack_templates(templates, n):
    """(seg_off np.uint64[n + 1], seg_kind np.uint8[n_seg (+ 1)], lit_off np.uint64[n_seg + 1], pool bytes) of am_subst_table_create_templates for value handles
    0 .. n - 1; a plain replacement is the template of that one literal."""
    tpls = [list(x) if _is_template(x) else [x] for x in templates]
    if len(tpls) != n:
        raise AmError(AM_ERR_INVALID, "replacements: one per value handle (%d given, %d handles)" % (len(tpls), n))
    seg_off, kinds, lits = np.zeros(n + 1, np.uint64), [], []
    for v, t in enumerate(tpls):
        for seg in t:
            if seg is MATCH:
                kinds.append(SEG_MATCH)
                lits.append(b"")
            elif isinstance(seg, (bytes, bytearray, str)):
                kinds.append(SEG_LITERAL)
                lits.append(_as_bytes(seg))
            else:
                raise AmError(AM_ERR_INVALID, "a template's segments are bytes, str or am.MATCH (needle %d)" % v)
        seg_off[v + 1] = len(kinds)
    pool, lit_off = pack_texts(lits)
    return seg_off, np.array(kinds + [0], np.uint8), lit_off, pool


def _pack_replacements(replacements, n):
    """(pool bytes, repl_off np.uint64[n + 1]) of am_subst_table_create for value handles 0 .. n - 1."""
    bs = [_as_bytes(x) for x in replacements]
    if len(bs) != n:
        raise AmError(AM_ERR_INVALID, "replacements: one per value handle (%d given, %d handles)" % (len(bs), n))
    pool, offs = pack_texts(bs)
    return pool, offs


def _take_texts(blob, offs):
    """Copies and frees the blob a facade call hands back: a list of bytes per offsets row."""
    try:
        whole = C.string_at(blob.value, int(offs[-1])) if int(offs[-1]) else b""
    finally:
        libhost().amh_free_blob(blob)
    return [whole[int(offs[i]):int(offs[i + 1])] for i in range(len(offs) - 1)]


def default_word_bytes():
    """am_word_bytes_default: the default word class as 256 flags (bytes of 0 / 1): 0-9 A-Z a-z _ and every byte 0x80-0xFF.  Runs without a device."""
    out = (C.c_uint8 * 256)()
    libam().am_word_bytes_default(out)
    return bytes(out)


def _word_flags(word_bytes):
    """None / False: no class (None).  True: the default class.  bytes or an iterable of byte values: the class of exactly those values (empty: the empty class).
    Returns np.uint8[256] flags or None."""
    if word_bytes is None or word_bytes is False:
        return None
    if word_bytes is True:
        return np.frombuffer(default_word_bytes(), dtype=np.uint8).copy()
    flags = np.zeros(256, np.uint8)
    for b in (word_bytes.encode("utf-8") if isinstance(word_bytes, str) else word_bytes):
        b = int(b)
        if not 0 <= b <= 255:
            raise AmError(AM_ERR_INVALID, "word_bytes: byte values 0 .. 255")
        flags[b] = 1
    return flags


def _pack_exact(exact, n):
    """(exact_off np.uint64[n + 1], pool bytes or None) of am_span_table_create_cased for value handles 0 .. n - 1, or (None, None) where no handle has a spelling.
    exact: None, or one entry per handle -- None (no spelling), bytes or str.  An empty spelling cannot be told from none by the C ABI and is refused here."""
    if exact is None:
        return None, None
    exact = list(exact)
    if len(exact) != n:
        raise AmError(AM_ERR_INVALID, "exact: one entry per value handle (%d given, %d handles)" % (len(exact), n))
    bs = [None if x is None else _as_bytes(x) for x in exact]
    if any(x is not None and len(x) == 0 for x in bs):
        raise AmError(AM_ERR_INVALID, "exact: an empty spelling (None means: no spelling)")
    if all(x is None for x in bs):
        return None, None
    pool, offs = pack_texts([x or b"" for x in bs])
    return offs, pool


def substitute_fold_host(case, triples, texts, len_bytes, len_code_points, replacements, word_bytes=None, exact=None):
    """amh_substitute_fold: the sequential definition of am_substitute over fold steps the caller brings (as spans_fold_host).  Runs without a device.  word_bytes: a
    word class as SpanTable takes it (amh_substitute_fold_words).  exact: spellings as SpanTable takes them (amh_substitute_fold_cased)."""
    hay = np.ascontiguousarray(triples[0], dtype=np.uint32)
    pos = np.ascontiguousarray(triples[1], dtype=np.uint64)
    val = np.ascontiguousarray(triples[2], dtype=np.uint32)
    lb = np.ascontiguousarray(len_bytes, dtype=np.uint32)
    lc = np.ascontiguousarray(len_code_points, dtype=np.uint32)
    n, nv = len(hay), len(lb)
    pad = lambda a, t: a if a.size else np.zeros(1, t)
    hay, pos, val, lb, lc = pad(hay, np.uint32), pad(pos, np.uint64), pad(val, np.uint32), pad(lb, np.uint32), pad(lc, np.uint32)
    pool, offs = _pack_replacements(replacements, nv)
    s = _Slices(texts)
    blob, out_offs = _vp(), np.zeros(s.n + 1, np.uint64)
    flags = _word_flags(word_bytes)
    eoff, epool = _pack_exact(exact, nv)
    if eoff is not None:
        _hcheck(libhost().amh_substitute_fold_cased(case, hay.ctypes.data, pos.ctypes.data, val.ctypes.data, n, s.arr, s.n, lb.ctypes.data, lc.ctypes.data, nv, pool,
                                                    offs.ctypes.data, None if flags is None else flags.ctypes.data, eoff.ctypes.data, epool, C.byref(blob),
                                                    out_offs.ctypes.data))
        return _take_texts(blob, out_offs)
    _hcheck(libhost().amh_substitute_fold_words(case, hay.ctypes.data, pos.ctypes.data, val.ctypes.data, n, s.arr, s.n, lb.ctypes.data, lc.ctypes.data, nv, pool,
                                                offs.ctypes.data, None if flags is None else flags.ctypes.data, C.byref(blob), out_offs.ctypes.data))
    return _take_texts(blob, out_offs)


def substitute_templates_fold_host(case, triples, texts, len_bytes, len_code_points, templates, word_bytes=None):
    """amh_substitute_templates_fold: the sequential definition of am_substitute with templates (a list per value handle of bytes / str / am.MATCH, or a plain
    replacement) over fold steps the caller brings, as substitute_fold_host.  Runs without a device."""
    hay = np.ascontiguousarray(triples[0], dtype=np.uint32)
    pos = np.ascontiguousarray(triples[1], dtype=np.uint64)
    val = np.ascontiguousarray(triples[2], dtype=np.uint32)
    lb = np.ascontiguousarray(len_bytes, dtype=np.uint32)
    lc = np.ascontiguousarray(len_code_points, dtype=np.uint32)
    n, nv = len(hay), len(lb)
    pad = lambda a, t: a if a.size else np.zeros(1, t)
    hay, pos, val, lb, lc = pad(hay, np.uint32), pad(pos, np.uint64), pad(val, np.uint32), pad(lb, np.uint32), pad(lc, np.uint32)
    seg_off, kind, lit_off, pool = _pack_templates(templates, nv)
    s = _Slices(texts)
    blob, out_offs = _vp(), np.zeros(s.n + 1, np.uint64)
    flags = _word_flags(word_bytes)
    _hcheck(libhost().amh_substitute_templates_fold(case, hay.ctypes.data, pos.ctypes.data, val.ctypes.data, n, s.arr, s.n, lb.ctypes.data, lc.ctypes.data, nv,
                                                    seg_off.ctypes.data, kind.ctypes.data, lit_off.ctypes.data, pool or None,
                                                    None if flags is None else flags.ctypes.data, C.byref(blob), out_offs.ctypes.data))
    return _take_texts(blob, out_offs)


def needle_lengths(needles, n_values=None):
    """(len_bytes, len_code_points) np.uint32 arrays of am_span_table_create for value handles 0 .. n - 1 = the needles in order (n = len(needles) unless given: fewer
    drops the last needles, more is refused)."""
    bs = [_as_bytes(x) for x in needles]
    n = len(bs) if n_values is None else int(n_values)
    if n > len(bs):
        raise AmError(AM_ERR_INVALID, "needle_lengths: more value handles than needles")
    lb = np.zeros(max(n, 1), np.uint32)
    lc = np.zeros(max(n, 1), np.uint32)
    for i in range(n):
        lb[i] = len(bs[i])
        lc[i] = sum(1 for c in bs[i] if (c & 0xC0) != 0x80)
    return lb, lc


def _handle_lengths(needles, n, lengths):
    """needle_lengths, or the caller's (len_bytes, len_code_points) per value handle cut or checked against n."""
    if lengths is None:
        return needle_lengths(needles, n)
    lb, lc = (np.ascontiguousarray(a, dtype=np.uint32) for a in lengths)
    n = len(lb) if n is None else int(n)
    if len(lb) != len(lc) or n > len(lb):
        raise AmError(AM_ERR_INVALID, "lengths: two arrays of at least n entries each")
    pad = np.zeros(1, np.uint32)
    return np.concatenate([lb[:n], pad]), np.concatenate([lc[:n], pad])


def _take_spans(po, pe, n_hay, k):
    """Copies and frees the two blocks a facade spans call hands back."""
    try:
        offs = np.frombuffer((C.c_char * ((n_hay + 1) * 8)).from_address(po.value), dtype=np.uint64).copy()
        spans = np.frombuffer((C.c_char * (k * SPAN_DTYPE.itemsize)).from_address(pe.value), dtype=SPAN_DTYPE).copy() if k else np.zeros(0, SPAN_DTYPE)
    finally:
        libhost().amh_free_u64(po)
        libhost().amh_free_u64(pe)
    return offs, spans


def spans_fold_host(case, mode, triples, texts, len_bytes, len_code_points, word_bytes=None, exact=None):
    """amh_spans_fold: the sequential definition of am_spans over fold steps the caller brings -- (haystack, matchPos, value) arrays in fold order -- the texts and the
    two length arrays.  Runs without a device.  word_bytes: a word class as SpanTable takes it (amh_spans_fold_words).  exact: spellings as SpanTable takes them
    (amh_spans_fold_cased, include/am.h "exact case")."""
    hay = np.ascontiguousarray(triples[0], dtype=np.uint32)
    pos = np.ascontiguousarray(triples[1], dtype=np.uint64)
    val = np.ascontiguousarray(triples[2], dtype=np.uint32)
    lb = np.ascontiguousarray(len_bytes, dtype=np.uint32)
    lc = np.ascontiguousarray(len_code_points, dtype=np.uint32)
    n, nv = len(hay), len(lb)
    pad = lambda a, t: a if a.size else np.zeros(1, t)
    hay, pos, val, lb, lc = pad(hay, np.uint32), pad(pos, np.uint64), pad(val, np.uint32), pad(lb, np.uint32), pad(lc, np.uint32)
    s = _Slices(texts)
    po, pe, ne = _vp(), _vp(), C.c_uint64(0)
    flags = _word_flags(word_bytes)
    eoff, epool = _pack_exact(exact, nv)
    if eoff is not None:
        _hcheck(libhost().amh_spans_fold_cased(case, mode, hay.ctypes.data, pos.ctypes.data, val.ctypes.data, n, s.arr, s.n, lb.ctypes.data, lc.ctypes.data, nv,
                                               None if flags is None else flags.ctypes.data, eoff.ctypes.data, epool, C.byref(po), C.byref(pe), C.byref(ne)))
        return _take_spans(po, pe, s.n, int(ne.value))
    _hcheck(libhost().amh_spans_fold_words(case, mode, hay.ctypes.data, pos.ctypes.data, val.ctypes.data, n, s.arr, s.n, lb.ctypes.data, lc.ctypes.data, nv,
                                           None if flags is None else flags.ctypes.data, C.byref(po), C.byref(pe), C.byref(ne)))
    return _take_spans(po, pe, s.n, int(ne.value))


def extract_fold_host(spans_offsets, spans, texts, before, after, merged=False):
    """amh_extract_fold: the sequential definition of am_fragments_from_spans (host/spans.hpp extractFold, a byte at a time) over spans the caller brings -- CSR offsets
    and SPAN_DTYPE rows as spans_fold_host returns them -- and the texts: (offsets np.uint64[len(texts) + 1], fragments FRAGMENT_DTYPE).  Runs without a device."""
    so = np.ascontiguousarray(spans_offsets, dtype=np.uint64)
    sp = np.ascontiguousarray(spans, dtype=SPAN_DTYPE)
    s = _Slices(texts)
    if len(so) != s.n + 1 or int(so[-1]) != len(sp):
        raise AmError(AM_ERR_INVALID, "extract_fold_host: the spans are not those of these texts")
    if not sp.size:
        sp = np.zeros(1, SPAN_DTYPE)
    po, pf, nf = _vp(), _vp(), C.c_uint64(0)
    _hcheck(libhost().amh_extract_fold(so.ctypes.data, sp.ctypes.data, s.arr, s.n, int(before), int(after), int(bool(merged)), C.byref(po), C.byref(pf), C.byref(nf)))
    k = int(nf.value)
    try:
        offs = np.frombuffer((C.c_char * ((s.n + 1) * 8)).from_address(po.value), dtype=np.uint64).copy()
        frags = np.frombuffer((C.c_char * (k * FRAGMENT_DTYPE.itemsize)).from_address(pf.value), dtype=FRAGMENT_DTYPE).copy() if k else np.zeros(0, FRAGMENT_DTYPE)
    finally:
        libhost().amh_free_u64(po)
        libhost().amh_free_u64(pf)
    return offs, frags


class ValuesTable:
    """machineValues of an Automaton in flat form on the device (am_needle_ids): what the fold-checksum and
    containsAll kernels expand records with."""

    def __init__(self, automaton, n_needles=None):
        self._a = automaton                      # the am_automaton must outlive the table
        self._off = np.ascontiguousarray(automaton.values_off(), dtype=np.uint64)
        self._val = np.ascontiguousarray(automaton.values(), dtype=np.uint32)
        if self._val.size == 0:
            self._val = np.zeros(1, np.uint32)
        h = _vp()
        n = len(automaton.needles) if n_needles is None else n_needles
        check(libam().am_needle_ids_create(automaton.device, self._off.ctypes.data, self._val.ctypes.data, n, C.byref(h)))
        self._h = h
        self.n_needles = int(n)

    def __del__(self):
        if getattr(self, "_h", None):
            libam().am_needle_ids_destroy(self._h)
            self._h = None

    @property
    def handle(self):
        return self._h

    def fold_hash(self, matches, n_hay):
        """am_matches_fold_hash: (hash[n_hay], count[n_hay]) of the fold sequences of an am_matches* result."""
        hashes, counts = np.zeros(max(n_hay, 1), np.uint64), np.zeros(max(n_hay, 1), np.uint64)
        check(libam().am_matches_fold_hash(matches, self._h, n_hay, hashes.ctypes.data, counts.ctypes.data))
        return hashes[:n_hay], counts[:n_hay]

    def _counts(self, call):
        out = np.zeros(max(self.n_needles, 1), np.uint64)
        check(call(out.ctypes.data))
        return out[:self.n_needles]

    def count_by_needle(self, matches):
        """am_matches_count_by_needle: per-value match counts (np.uint64[n_needles]) of an am_matches* result whose records are in HBM."""
        return self._counts(lambda out: libam().am_matches_count_by_needle(matches, self._h, out))

    def count_by_needle_batch(self, case, batch):
        """am_count_by_needle_batch: the same over a device-resident batch (an am_batch* handle: am_batch_upload / am_batch_from_device)."""
        return self._counts(lambda out: libam().am_count_by_needle_batch(self._h, case, batch, out))

    def count_by_needle_texts(self, case, texts):
        """am_count_by_needle: the one-shot form on host texts."""
        s = _Slices(texts)
        return self._counts(lambda out: libam().am_count_by_needle(self._h, case, s.arr, s.n, out))


    def _matrix(self, call, raw):
        return _csr_call(call, matrix_to_numpy, libam().am_needle_matrix_free, raw)

    def count_matrix(self, matches, n_hay, raw=False):
        """am_matches_count_matrix: the term-document matrix (offsets np.uint64[n_hay + 1], entries NEEDLE_COUNT_DTYPE) of an am_matches* result whose records are in
        HBM.  raw: the am_needle_matrix* itself, in HBM (measurements; free with am_needle_matrix_free)."""
        return self._matrix(lambda out: libam().am_matches_count_matrix(matches, self._h, n_hay, out), raw)

    def count_matrix_batch(self, case, batch, raw=False):
        """am_count_matrix_batch: the same over a device-resident batch (an am_batch* handle: am_batch_upload / am_batch_from_device / Splitter.lines_batch)."""
        return self._matrix(lambda out: libam().am_count_matrix_batch(self._h, case, batch, out), raw)

    def count_matrix_texts(self, case, texts, raw=False):
        """am_count_matrix: the one-shot form on host texts."""
        s = _Slices(texts)
        return self._matrix(lambda out: libam().am_count_matrix(self._h, case, s.arr, s.n, out), raw)

    def select_all_batch(self, case, batch, invert=False):
        """am_select_all_batch on a device-resident batch (an am_batch* handle): the Selection of the haystacks that contain every needle id (Searcher.containsAll)."""
        return _select(lambda out: libam().am_select_all_batch(self._h, case, int(bool(invert)), batch, out))

    def select_all_texts(self, case, texts, invert=False):
        """am_select_all: the one-shot form on host texts."""
        s = _Slices(texts)
        return _select(lambda out: libam().am_select_all(self._h, case, int(bool(invert)), s.arr, s.n, out))


class SpanTable:
    """The needles' lengths beside machineValues on the device (am_span_table): what am_spans* turns a fold step into a span with.  Lengths come from
    automaton.needles, handle = needle index; n_needles below len(needles) skips the handles from n_needles on.  lengths: (len_bytes, len_code_points) per value handle
    for an automaton built with handles of its own.  word_bytes: None -- no word class, every span is a row; True -- the default class; bytes or an iterable of byte
    values -- the class of those values (am_span_table_create_words): every consumer of the table then sees the whole-word spans only.  exact: None, or one entry
    per handle -- None, bytes or str: the spelling a span of that handle must have in the text to be a row (am_span_table_create_cased, include/am.h "exact case");
    all None is the plain or the words table, made through the old entry points."""

    def __init__(self, automaton, n_needles=None, lengths=None, word_bytes=None, exact=None):
        if n_needles is None and lengths is not None:
            n_needles = len(lengths[0])
        self._values = ValuesTable(automaton, n_needles)      # (the am_needle_ids must outlive the table)
        self.n_needles = self._values.n_needles
        self._lb, self._lc = _handle_lengths(automaton.needles, self.n_needles, lengths)
        self._words = _word_flags(word_bytes)
        self._exact_off, self._exact_pool = _pack_exact(exact, self.n_needles)
        h = _vp()
        if self._exact_off is not None:
            check(libam().am_span_table_create_cased(self._values.handle, self._lb.ctypes.data, self._lc.ctypes.data, 0 if self._words is None else SPAN_TABLE_WORDS,
                                                     None if self._words is None else self._words.ctypes.data, self._exact_off.ctypes.data, self._exact_pool,
                                                     C.byref(h)))
        elif self._words is None:
            check(libam().am_span_table_create(self._values.handle, self._lb.ctypes.data, self._lc.ctypes.data, C.byref(h)))
        else:
            check(libam().am_span_table_create_words(self._values.handle, self._lb.ctypes.data, self._lc.ctypes.data, self._words.ctypes.data, C.byref(h)))
        self._h = h

    def __del__(self):
        if getattr(self, "_h", None):
            libam().am_span_table_destroy(self._h)
            self._h = None

    @property
    def handle(self):
        return self._h

    @property
    def word_bytes(self):
        """am_span_table_word_bytes: the table's class as 256 flags (bytes of 0 / 1), None for a table without one."""
        out = (C.c_uint8 * 256)()
        return bytes(out) if libam().am_span_table_word_bytes(self._h, out) else None

    @property
    def exact(self):
        """am_span_table_exact per handle: the table's spellings as a list of bytes / None."""
        out = []
        for v in range(self.n_needles):
            p, n = _vp(), C.c_uint64(0)
            out.append(C.string_at(p.value, int(n.value)) if libam().am_span_table_exact(self._h, v, C.byref(p), C.byref(n)) else None)
        return out

    def _spans(self, call, raw):
        return _csr_call(call, spans_to_numpy, libam().am_spans_free, raw)

    def _counts(self, call):
        out = np.zeros(max(self.n_needles, 1), np.uint64)
        check(call(out.ctypes.data))
        return out[:self.n_needles]

    def count_by_needle_batch(self, case, batch):
        """am_count_spans_by_needle_batch on a device-resident batch: np.uint64[n_needles], counts[v] = the AM_SPANS_ALL rows of this table with needle v (with a word
        class: the whole-word occurrences; without one: ValuesTable.count_by_needle_batch's vector)."""
        return self._counts(lambda out: libam().am_count_spans_by_needle_batch(self._h, case, batch, out))

    def count_by_needle_texts(self, case, texts):
        """am_count_spans_by_needle: the one-shot form on host texts."""
        s = _Slices(texts)
        return self._counts(lambda out: libam().am_count_spans_by_needle(self._h, case, s.arr, s.n, out))

    def spans_batch(self, case, batch, mode, raw=False, unit=BYTES):
        """am_spans_batch on a device-resident batch (an am_batch* handle: am_batch_upload / am_batch_from_device / Splitter.lines_batch): (offsets np.uint64[n_hay + 1],
        spans SPAN_DTYPE[offsets[-1]]).  raw: the am_spans* itself, in HBM (measurements; free with am_spans_free).  unit: CODE_POINTS or UTF16 convert start and len
        in HBM through an index built for this call (Coords; a caller with many calls on one batch keeps a Coords of its own)."""
        if unit == BYTES:
            return self._spans(lambda out: libam().am_spans_batch(self._h, case, mode, batch, out), raw)
        spans_raw = self._spans(lambda out: libam().am_spans_batch(self._h, case, mode, batch, out), True)
        try:
            return Coords(batch, utf16=unit == UTF16).spans(spans_raw, unit, raw)
        finally:
            libam().am_spans_free(spans_raw)

    def spans_texts(self, case, texts, mode):
        """am_spans: the one-shot form on host texts."""
        s = _Slices(texts)
        return self._spans(lambda out: libam().am_spans(self._h, case, mode, s.arr, s.n, out), False)

    def postings_batch(self, case, batch, mode, raw=False):
        """am_postings_batch on a device-resident batch: the Postings of its spans in `mode` (SPANS_ALL / SPANS_LEFTMOST_LONGEST).  raw: the am_postings* itself
        (measurements; free with am_postings_free)."""
        h = _vp()
        check(libam().am_postings_batch(self._h, case, mode, batch, C.byref(h)))
        return h if raw else Postings(h)

    def postings_texts(self, case, texts, mode):
        """am_postings: the one-shot form on host texts."""
        s = _Slices(texts)
        h = _vp()
        check(libam().am_postings(self._h, case, mode, s.arr, s.n, C.byref(h)))
        return Postings(h)

    def postings_from_spans(self, spans_raw):
        """am_postings_from_spans: the stage alone over an am_spans* the caller holds (spans_batch(..., raw=True), Coords.spans(..., raw=True))."""
        h = _vp()
        check(libam().am_postings_from_spans(spans_raw, C.byref(h)))
        return Postings(h)

    def select_batch(self, case, batch, invert=False):
        """am_select_spans_batch on a device-resident batch: the Selection of the haystacks whose SPANS_ALL row under this table is not empty (with a word class:
        the haystacks that hold a needle as a whole word)."""
        return _select(lambda out: libam().am_select_spans_batch(self._h, case, int(bool(invert)), batch, out))

    @property
    def values(self):
        """The ValuesTable the table was made over: what a Weights for score_batch is made over."""
        return self._values

    def score_batch(self, case, batch, weights):
        """am_score_spans_batch on a device-resident batch: the Scores of its haystacks over the AM_SPANS_ALL rows of this table (with a word class: the whole-word
        occurrences only).  weights: a Weights made over this table's `values`."""
        return _scores(lambda out: libam().am_score_spans_batch(self._h, weights.handle, case, batch, out))

    def fragments_from_spans(self, batch, spans_raw, before, after, merged, raw=False):
        """am_fragments_from_spans: the windows of an am_spans* the caller holds (spans_batch(..., raw=True) on `batch`) as (offsets np.uint64[n_hay + 1], fragments
        FRAGMENT_DTYPE), relative to their haystacks.  raw: the am_fragments* itself, in HBM (am_batch_from_fragments takes it; free with am_fragments_free)."""
        return _csr_call(lambda out: libam().am_fragments_from_spans(batch, spans_raw, int(before), int(after), EXTRACT_MERGED if merged else EXTRACT_EACH, out),
                         fragments_to_numpy, libam().am_fragments_free, raw)

    def extract_batch(self, case, batch, before=0, after=0, merged=False, leftmost_longest=True):
        """am_extract_batch on a device-resident batch: (the new am_batch* handle with one haystack per fragment -- free with am_batch_destroy --, offsets
        np.uint64[n_hay + 1], fragments FRAGMENT_DTYPE in SOURCE coordinates: the snippets of haystack i are haystacks offsets[i] .. offsets[i + 1] of the new batch)."""
        nb, fr = _vp(), _vp()
        check(libam().am_extract_batch(self._h, case, SPANS_LEFTMOST_LONGEST if leftmost_longest else SPANS_ALL, int(before), int(after),
                                       EXTRACT_MERGED if merged else EXTRACT_EACH, batch, C.byref(nb), C.byref(fr)))
        try:
            offs, frags = fragments_to_numpy(fr)
        except Exception:
            libam().am_batch_destroy(nb)
            raise
        finally:
            libam().am_fragments_free(fr)
        return nb, offs, frags


class _Uploaded:
    """Host texts as a device-resident batch for the length of a with block (am_batch_upload / am_batch_destroy)."""

    def __init__(self, texts):
        self._s = _Slices(texts)
        self._b = _vp()

    def __enter__(self):
        check(libam().am_batch_upload(self._s.arr, self._s.n, C.byref(self._b)))
        return self._b

    def __exit__(self, *exc):
        libam().am_batch_destroy(self._b)


class Coords:
    """The coordinate index of a device-resident batch (am_coords, include/am.h "coordinates"): per 128-byte tile of the text the running counts of code points, of
    four-byte sequences (utf16) and of newlines (lines), in HBM.  Converts results that are in bytes -- spans, fragments, positions -- into CODE_POINTS or UTF16 and
    gives every span its line and column, without the rows leaving the device.  The batch must outlive the index."""

    def __init__(self, batch, lines=False, utf16=False):
        self._batch = batch
        h = _vp()
        check(libam().am_coords_create(batch, COORDS_CODE_POINTS | (COORDS_UTF16 if utf16 else 0) | (COORDS_LINES if lines else 0), C.byref(h)))
        self._h = h

    def __del__(self):
        if getattr(self, "_h", None):
            libam().am_coords_destroy(self._h)
            self._h = None

    @property
    def handle(self):
        return self._h

    @property
    def index_bytes(self):
        """am_coords_index_bytes: the bytes of HBM the index keeps."""
        return int(libam().am_coords_index_bytes(self._h))

    def spans(self, spans_raw, unit, raw=False):
        """am_coords_spans: an am_spans* the caller holds (spans_batch(..., raw=True) on this batch) with start and len in `unit`, as (offsets, spans SPAN_DTYPE).
        raw: the new am_spans* itself, in HBM (free with am_spans_free)."""
        return _csr_call(lambda out: libam().am_coords_spans(self._h, spans_raw, int(unit), out), spans_to_numpy, libam().am_spans_free, raw)

    def fragments(self, fragments_raw, unit, raw=False):
        """am_coords_fragments: the same for an am_fragments* (Splitter.split_fragments, fragments_from_spans(..., raw=True)), as (offsets, fragments FRAGMENT_DTYPE)."""
        return _csr_call(lambda out: libam().am_coords_fragments(self._h, fragments_raw, int(unit), out), fragments_to_numpy, libam().am_fragments_free, raw)

    def ranges(self, spans_raw, unit, raw=False):
        """am_coords_ranges: (offsets, ranges SPAN_RANGE_DTYPE) -- 0-based line and column, in `unit`, of the start and of the end of every span; needs lines=True.
        raw: the am_ranges* itself, in HBM (free with am_ranges_free)."""
        return _csr_call(lambda out: libam().am_coords_ranges(self._h, spans_raw, int(unit), out), ranges_to_numpy, libam().am_ranges_free, raw)

    def positions(self, hay, pos, unit):
        """am_coords_positions: pos[i], a byte position relative to haystack hay[i], in `unit` (np.uint64).  AmError(AM_ERR_INVALID) for a haystack index or a position
        outside the batch."""
        hay, pos = np.ascontiguousarray(hay, dtype=np.uint32), np.ascontiguousarray(pos, dtype=np.uint64)
        if hay.shape != pos.shape or hay.ndim != 1:
            raise AmError(AM_ERR_INVALID, "positions: hay and pos are two flat arrays of one length")
        out = np.zeros(max(len(hay), 1), np.uint64)
        check(libam().am_coords_positions(self._h, hay.ctypes.data, pos.ctypes.data, len(hay), int(unit), out.ctypes.data))
        return out[:len(hay)]


class Selection:
    """Which haystacks of a batch a select kept (am_selection): ascending source indices in HBM, copied to the host on first use."""

    def __init__(self, handle):
        self._h = handle

    def __del__(self):
        if getattr(self, "_h", None):
            libam().am_selection_free(self._h)
            self._h = None

    @property
    def handle(self):
        return self._h

    @property
    def size(self):
        return int(libam().am_selection_size(self._h))

    @property
    def source_haystacks(self):
        return int(libam().am_selection_source_haystacks(self._h))

    @property
    def total_bytes(self):
        return int(libam().am_selection_total_bytes(self._h))

    @property
    def indices(self):
        """np.uint32[size]: the kept haystacks' indices in the source batch, ascending."""
        p = libam().am_selection_indices(self._h)
        if not p:
            check(AM_ERR_HIP)
        n = self.size
        return np.ctypeslib.as_array(C.cast(p, _u32p), shape=(max(n, 1),))[:n].copy()

    def batch(self, src):
        """am_batch_from_selection: the kept haystacks of `src` (the am_batch* the selection was made from) as a new am_batch* in HBM; free with am_batch_destroy."""
        nb = _vp()
        check(libam().am_batch_from_selection(src, self._h, C.byref(nb)))
        return nb


def _select(call):
    h = _vp()
    check(call(C.byref(h)))
    return Selection(h)


def select_flags(batch, flags, invert=False):
    """am_select_flags: the caller's own predicate over an am_batch* handle, one flag per haystack (non-zero = true)."""
    f = np.ascontiguousarray(np.asarray(flags) != 0, dtype=np.uint8)
    return _select(lambda out: libam().am_select_flags(batch, f.ctypes.data if f.size else None, int(bool(invert)), out))


def select_geometry():
    """(tile_bytes, scan_block_items) of the select's gather and of the compaction's exclusive sums (am_select_geometry)."""
    t, s = C.c_uint32(0), C.c_uint32(0)
    libam().am_select_geometry(C.byref(t), C.byref(s))
    return int(t.value), int(s.value)


def rules_geometry():
    """(tile_haystacks, lds_slot_words, lds_rules) of the rule evaluation (am_rules_geometry): every internal limit a test must cross."""
    t, w, r = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
    libam().am_rules_geometry(C.byref(t), C.byref(w), C.byref(r))
    return int(t.value), int(w.value), int(r.value)


def score_geometry():
    """(tile_records, topk_block_items) of the scoring fold and of the top-k histogram (am_score_geometry): known without a device."""
    t, b = C.c_uint32(0), C.c_uint32(0)
    libam().am_score_geometry(C.byref(t), C.byref(b))
    return int(t.value), int(b.value)


def _weight_columns(columns, n_needles):
    """np.int64[n_cols, n_needles], C-contiguous, of one column or a list of columns."""
    w = np.asarray(columns, dtype=np.int64)
    if w.ndim == 1:
        w = w.reshape(1, -1)
    if w.ndim != 2 or w.shape[1] != n_needles:
        raise AmError(AM_ERR_INVALID, "weights: columns of one weight per value handle (%s given, %d handles)" % (w.shape, n_needles))
    return np.ascontiguousarray(w)


def score_host(hay, val, n_hay, n_values, columns):
    """amh_score: the sequential definition of am_score (host/automaton.hpp scoreByHaystack) over fold steps the caller brings -- (haystack, value) arrays in fold
    order -- and weight columns.  Runs without a device.  np.int64[n_cols, n_hay]."""
    hay, val = np.ascontiguousarray(hay, np.uint32), np.ascontiguousarray(val, np.uint32)
    w = _weight_columns(columns, n_values)
    out = np.zeros(max(w.shape[0] * n_hay, 1), np.int64)
    _hcheck(libhost().amh_score(hay.ctypes.data if hay.size else None, val.ctypes.data if val.size else None, hay.size, n_hay, n_values,
                                w.ctypes.data if w.size else None, w.shape[0], out.ctypes.data))
    return out[:w.shape[0] * n_hay].reshape(w.shape[0], n_hay)


class Weights:
    """Weight columns over the value handles of a ValuesTable, on the device (am_weights): Weights(table, [[w of handle 0, w of handle 1, ...], ...]), one to
    SCORE_MAX_COLUMNS columns of int64 (one flat list: one column)."""

    def __init__(self, values_table, columns):
        self._t = values_table                   # the am_needle_ids must outlive the weights
        self.columns = _weight_columns(columns, values_table.n_needles)
        h = _vp()
        check(libam().am_weights_create(values_table.handle, self.columns.ctypes.data if self.columns.size else None, self.columns.shape[0], C.byref(h)))
        self._h = h

    def __del__(self):
        if getattr(self, "_h", None):
            libam().am_weights_destroy(self._h)
            self._h = None

    @property
    def handle(self):
        return self._h

    @property
    def n_cols(self):
        return int(self.columns.shape[0])

    def score_batch(self, case, batch):
        """am_score_batch on a device-resident batch (an am_batch* handle): the Scores of its haystacks."""
        return _scores(lambda out: libam().am_score_batch(self._h, case, batch, out))

    def score_texts(self, case, texts):
        """am_score: the one-shot form on host texts."""
        s = _Slices(texts)
        return _scores(lambda out: libam().am_score(self._h, case, s.arr, s.n, out))

    def score_matches(self, matches, n_hay):
        """am_matches_score: the same fold over an am_matches* result whose records are in HBM."""
        return _scores(lambda out: libam().am_matches_score(matches, self._h, n_hay, out))


class Scores:
    """What a scoring call left in HBM (am_scores): int64[n_cols, n_hay], copied to the host on first use."""

    def __init__(self, handle):
        self._h = handle

    def __del__(self):
        if getattr(self, "_h", None):
            libam().am_scores_free(self._h)
            self._h = None

    @property
    def handle(self):
        return self._h

    @property
    def n_hay(self):
        return int(libam().am_scores_haystacks(self._h))

    @property
    def n_cols(self):
        return int(libam().am_scores_columns(self._h))

    @property
    def scores(self):
        """np.int64[n_cols, n_hay]: scores[c, i] = the sum of column c's weights over the fold steps of haystack i, modulo 2^64."""
        p = libam().am_scores_data(self._h)
        if not p:
            check(AM_ERR_HIP)
        n = self.n_cols * self.n_hay
        return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_int64)), shape=(max(n, 1),))[:n].copy().reshape(self.n_cols, self.n_hay)

    def top_k(self, k, column=0, largest=True):
        """am_scores_top_k: the min(k, n_hay) best haystacks of a column as SCORED_DTYPE[...] in order -- (score descending, haystack ascending), or with
        largest=False (score ascending, haystack ascending).  The cut is found on the device; the winners cross."""
        out = np.zeros(max(min(int(k), self.n_hay), 1), SCORED_DTYPE)
        n = C.c_uint64(0)
        check(libam().am_scores_top_k(self._h, int(column), int(k), int(bool(largest)), out.ctypes.data, C.byref(n)))
        return out[:int(n.value)]

    def select_top_k(self, k, column=0, largest=True, batch=None):
        """am_select_top_k: the same haystacks as a Selection of `batch` (the am_batch* the scores were made from), ascending indices."""
        return _select(lambda out: libam().am_select_top_k(self._h, int(column), int(k), int(bool(largest)), batch, out))

    def select(self, lo, hi, column=0, invert=False, batch=None):
        """am_select_score: the Selection of the haystacks of `batch` with lo <= score <= hi (lo > hi: none); invert: the others."""
        return _select(lambda out: libam().am_select_score(self._h, int(column), int(lo), int(hi), int(bool(invert)), batch, out))


def _scores(call):
    h = _vp()
    check(call(C.byref(h)))
    return Scores(h)


def postings_geometry(n_needles):
    """(tile_spans, wave_spans, passes, bits) of the postings sort for n_needles (am_postings_geometry): the spans of a workgroup tile, the consecutive spans of a
    wavefront's portion (taken 64 per round), the passes and the bits each pass sorts, lowest first (a list of `passes` entries).  Known without a device."""
    t, w, p = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
    bits = (C.c_uint32 * 4)()
    libam().am_postings_geometry(int(n_needles), C.byref(t), C.byref(w), C.byref(p), bits)
    return int(t.value), int(w.value), int(p.value), [int(b) for b in bits[:p.value]]


def postings_host(offsets, spans, n_needles):
    """The definition of am_postings_from_spans in numpy over spans the caller brings -- CSR offsets and SPAN_DTYPE rows: (offsets np.uint64[n_needles + 1], spans
    SPAN_DTYPE, source np.uint64, doc_freq np.uint64[n_needles]).  Runs without a device."""
    so = np.ascontiguousarray(offsets, dtype=np.uint64)
    sp = np.ascontiguousarray(spans, dtype=SPAN_DTYPE)
    n = int(n_needles)
    if len(so) < 1 or int(so[-1]) != len(sp):
        raise AmError(AM_ERR_INVALID, "postings_host: the offsets are not those of the spans")
    if len(sp) and int(sp["needle"].max()) >= n:
        raise AmError(AM_ERR_INVALID, "postings_host: a needle handle is not below n_needles")
    perm = np.argsort(sp["needle"], kind="stable")
    data = sp[perm]
    offs = np.searchsorted(data["needle"], np.arange(n + 1, dtype=np.uint64), side="left").astype(np.uint64)
    head = np.ones(len(data), bool)
    head[1:] = (data["needle"][1:] != data["needle"][:-1]) | (data["haystack"][1:] != data["haystack"][:-1])
    return offs, data, perm.astype(np.uint64), np.bincount(data["needle"][head], minlength=n).astype(np.uint64)[:n]


class Postings:
    """The spans of a result by needle (am_postings, include/am.h "postings"): row v = the occurrences of needle v, in HBM, copied to the host on first use.  A context
    manager: leaving the block frees the handle."""

    def __init__(self, handle):
        self._h = handle

    def close(self):
        if getattr(self, "_h", None):
            libam().am_postings_free(self._h)
            self._h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    @property
    def handle(self):
        return self._h

    @property
    def size(self):
        return int(libam().am_postings_size(self._h))

    @property
    def n_needles(self):
        return int(libam().am_postings_needles(self._h))

    @property
    def n_hay(self):
        return int(libam().am_postings_haystacks(self._h))

    def _host(self, fn, n, dtype):
        p = fn(self._h)
        if not p:
            raise AmError(AM_ERR_HIP, (libam().am_last_error() or b"").decode())
        return np.frombuffer((C.c_char * (n * dtype.itemsize)).from_address(p), dtype=dtype).copy() if n else np.zeros(0, dtype)

    @property
    def offsets(self):
        """np.uint64[n_needles + 1]: the occurrences of needle v are spans[offsets[v]:offsets[v + 1]]."""
        return self._host(libam().am_postings_offsets, self.n_needles + 1, np.dtype(np.uint64))

    @property
    def spans(self):
        """SPAN_DTYPE[size]: ascending by (needle, haystack, then the order of the spans they were made from)."""
        return self._host(libam().am_postings_data, self.size, SPAN_DTYPE)

    @property
    def source(self):
        """np.uint64[size]: source[k] = the row of the spans result that spans[k] came from."""
        return self._host(libam().am_postings_source, self.size, np.dtype(np.uint64))

    @property
    def doc_freq(self):
        """np.uint64[n_needles]: the distinct haystacks in each row."""
        return self._host(libam().am_postings_doc_freq, self.n_needles, np.dtype(np.uint64))

    def row(self, v):
        """The occurrences of needle v: SPAN_DTYPE rows (through the host copies)."""
        if not 0 <= int(v) < self.n_needles:
            raise AmError(AM_ERR_INVALID, "row: the needle is not below n_needles")
        o = self.offsets
        return self.spans[int(o[int(v)]):int(o[int(v) + 1])]

    def spans_of(self, v, raw=False):
        """am_spans_of_needle: row v as a spans result of its own, per-haystack offsets rebuilt in HBM: (offsets np.uint64[n_hay + 1], spans SPAN_DTYPE).  raw: the
        am_spans* itself (fragments_from_spans, Coords and SubstTable.splice take it; free with am_spans_free)."""
        return _csr_call(lambda out: libam().am_spans_of_needle(self._h, int(v), out), spans_to_numpy, libam().am_spans_free, raw)


def near_geometry():
    """(tile_spans, word_spans) of the proximity stage (am_near_geometry): the spans a workgroup step handles -- a sweep of the word links covers 4 x tile_spans words
    -- and the spans of a bitmap word.  Known without a device."""
    t, w = C.c_uint32(0), C.c_uint32(0)
    libam().am_near_geometry(C.byref(t), C.byref(w))
    return int(t.value), int(w.value)


class NearQuery:
    """One proximity query: every span of group a with its nearest other span of group b, a pair where the gap between them is at most max_gap bytes.  ordered: only
    a b BEHIND the anchor counts (AM_NEAR_ORDERED).  a / b: group indices 0 .. 31 (Automaton.near takes group names)."""

    def __init__(self, a, b, max_gap, ordered=False):
        self.a, self.b, self.max_gap, self.ordered = a, b, int(max_gap), bool(ordered)


def _near_queries(queries):
    """NEAR_QUERY_DTYPE[n] of NearQuery objects, (a, b, max_gap[, ordered]) tuples or a ready array (taken as it is: the library checks it)."""
    if isinstance(queries, np.ndarray) and queries.dtype == NEAR_QUERY_DTYPE:
        return np.ascontiguousarray(queries)
    out = np.zeros(len(queries), NEAR_QUERY_DTYPE)
    for i, q in enumerate(queries):
        q = q if isinstance(q, NearQuery) else NearQuery(*q)
        out[i] = (int(q.a), int(q.b), NEAR_ORDERED if q.ordered else 0, 0, q.max_gap)
    return out


def near_host(spans_offsets, spans, group_mask, queries):
    """amh_near_fold: the sequential definition of am_near_spans (host/near.hpp nearFold: a plain loop to the left and to the right of every anchor) over leftmost-longest
    spans the caller brings -- CSR offsets and SPAN_DTYPE rows -- a mask per needle handle and queries.  Runs without a device.
    (offsets np.uint64[n_hay + 1], pairs NEAR_PAIR_DTYPE, fired_words np.uint64[n_queries, hay_words], counts np.uint64[n_queries])."""
    so = np.ascontiguousarray(spans_offsets, dtype=np.uint64)
    sp = np.ascontiguousarray(spans, dtype=SPAN_DTYPE)
    gm = np.ascontiguousarray(group_mask, dtype=np.uint32)
    qs = _near_queries(queries)
    n_hay, nq, hw = len(so) - 1, len(qs), (len(so) - 1 + 63) // 64
    if n_hay < 0 or int(so[-1]) != len(sp):
        raise AmError(AM_ERR_INVALID, "near_host: the offsets are not those of the spans")
    pad = lambda a, t: a if a.size else np.zeros(1, t)
    fired, counts = np.zeros(max(nq * hw, 1), np.uint64), np.zeros(max(nq, 1), np.uint64)
    po, pp, n = _vp(), _vp(), C.c_uint64(0)
    _hcheck(libhost().amh_near_fold(so.ctypes.data, pad(sp, SPAN_DTYPE).ctypes.data, n_hay, pad(gm, np.uint32).ctypes.data, len(gm), pad(qs, NEAR_QUERY_DTYPE).ctypes.data, nq,
                                    C.byref(po), C.byref(pp), C.byref(n), fired.ctypes.data, counts.ctypes.data))
    k = int(n.value)
    try:
        offs = np.frombuffer((C.c_char * ((n_hay + 1) * 8)).from_address(po.value), dtype=np.uint64).copy()
        pairs = np.frombuffer((C.c_char * (k * NEAR_PAIR_DTYPE.itemsize)).from_address(pp.value), dtype=NEAR_PAIR_DTYPE).copy() if k else np.zeros(0, NEAR_PAIR_DTYPE)
    finally:
        libhost().amh_free_u64(po)
        libhost().amh_free_u64(pp)
    return offs, pairs, fired[:nq * hw].reshape(nq, hw), counts[:nq]


class NearHits:
    """What a proximity call found (am_near_hits): the pairs as CSR rows, query-major haystack bitmaps and per-query counts in HBM, copied to the host on first use."""

    def __init__(self, handle):
        self._h = handle

    def __del__(self):
        if getattr(self, "_h", None):
            libam().am_near_hits_free(self._h)
            self._h = None

    @property
    def handle(self):
        return self._h

    @property
    def n_hay(self):
        return int(libam().am_near_hits_haystacks(self._h))

    @property
    def n_queries(self):
        return int(libam().am_near_hits_queries(self._h))

    @property
    def hay_words(self):
        return int(libam().am_near_hits_hay_words(self._h))

    def _host(self, fn, n, dtype):
        p = fn(self._h)
        if not p:
            check(AM_ERR_HIP)
        return np.frombuffer((C.c_char * (n * dtype.itemsize)).from_address(p), dtype=dtype).copy() if n else np.zeros(0, dtype)

    @property
    def pairs(self):
        """NEAR_PAIR_DTYPE[size]: a and b index the data array of the spans the hits were made from; rows ascend by (haystack, a, query)."""
        return self._host(libam().am_near_hits_data, int(libam().am_near_hits_size(self._h)), NEAR_PAIR_DTYPE)

    @property
    def offsets(self):
        """np.uint64[n_hay + 1]: the pairs of haystack i are pairs[offsets[i]:offsets[i + 1]]."""
        return self._host(libam().am_near_hits_offsets, self.n_hay + 1, np.dtype(np.uint64))

    @property
    def fired_words(self):
        """np.uint64[n_queries, hay_words]: bit h % 64 of word h // 64 of row q is set iff query q has a pair in haystack h; the bits beyond n_hay are zero."""
        return self._host(libam().am_near_hits_fired, self.n_queries * self.hay_words, np.dtype(np.uint64)).reshape(self.n_queries, self.hay_words)

    @property
    def fired(self):
        """bool[n_queries, n_hay]."""
        return _fired_bits(self.fired_words, self.n_queries, self.n_hay)

    @property
    def counts(self):
        """np.uint64[n_queries]: the pairs of each query."""
        return self._host(libam().am_near_hits_counts, self.n_queries, np.dtype(np.uint64))

    def select(self, query, batch=None, invert=False):
        """am_select_near: the Selection of the haystacks of `batch` (the am_batch* the spans of the hits were made from) in which `query` has a pair; invert: the others."""
        return _select(lambda out: libam().am_select_near(self._h, int(query), int(bool(invert)), batch, out))


class Near:
    """Groups and queries of a proximity call over a SpanTable, on the device (am_near): Near(table, group_mask, queries) with one uint32 mask per needle handle (bit g:
    the needle is in group g) and up to NEAR_MAX_QUERIES NearQuery objects or (a, b, max_gap[, ordered]) tuples."""

    def __init__(self, span_table, group_mask, queries):
        self._t = span_table                     # the am_span_table must outlive the handle
        self.group_mask = np.ascontiguousarray(group_mask, dtype=np.uint32)
        if self.group_mask.shape != (span_table.n_needles,):
            raise AmError(AM_ERR_INVALID, "group_mask: one mask per value handle (%s given, %d handles)" % (self.group_mask.shape, span_table.n_needles))
        self.queries = _near_queries(queries)
        h = _vp()
        check(libam().am_near_create(span_table.handle, self.group_mask.ctypes.data if self.group_mask.size else None,
                                     self.queries.ctypes.data if self.queries.size else None, len(self.queries), C.byref(h)))
        self._h = h

    def __del__(self):
        if getattr(self, "_h", None):
            libam().am_near_destroy(self._h)
            self._h = None

    @property
    def handle(self):
        return self._h

    def near_spans(self, spans_raw):
        """am_near_spans: the stage alone over an am_spans* the caller holds (SpanTable.spans_batch(..., SPANS_LEFTMOST_LONGEST, raw=True))."""
        h = _vp()
        check(libam().am_near_spans(self._h, spans_raw, C.byref(h)))
        return NearHits(h)

    def _with_spans(self, call, spans):
        h, s = _vp(), _vp()
        check(call(C.byref(h), C.byref(s) if spans else None))
        hits = NearHits(h)
        if not spans:
            return hits
        try:
            return hits, spans_to_numpy(s)
        finally:
            libam().am_spans_free(s)

    def near_batch(self, case, batch, spans=False):
        """am_near_batch on a device-resident batch (an am_batch* handle): the NearHits; spans=True: (NearHits, (offsets, SPAN_DTYPE rows)) -- the spans a and b index."""
        return self._with_spans(lambda out, s: libam().am_near_batch(self._h, case, batch, out, s), spans)

    def near_texts(self, case, texts, spans=False):
        """am_near: the one-shot form on host texts."""
        sl = _Slices(texts)
        return self._with_spans(lambda out, s: libam().am_near(self._h, case, sl.arr, sl.n, out, s), spans)


class Not:
    """A negated needle inside Rule.cnf: the literal is true where the needle does NOT occur."""

    def __init__(self, needle):
        self.needle = needle


class Rule:
    """One rule of a RuleSet, in conjunctive normal form over needles: every needle of all_of occurs, AND some needle of any_of occurs, AND no needle of none_of
    occurs.  An absent any_of adds no clause; an explicit empty any_of=[] adds an empty clause, which is false.  A rule without a clause is true.  Rule.cnf takes the
    clauses themselves: a list of lists of needles, a needle wrapped in Not negated."""

    def __init__(self, all_of=(), any_of=None, none_of=()):
        self.clauses = [[(n, False)] for n in all_of]
        if any_of is not None:
            self.clauses.append([(n, False) for n in any_of])
        self.clauses += [[(n, True)] for n in none_of]

    @classmethod
    def cnf(cls, clauses):
        r = cls()
        r.clauses = [[(x.needle, True) if isinstance(x, Not) else (x, False) for x in c] for c in clauses]
        return r


def compile_rules(case, rules):
    """Needles to slots, on the host: (needles [bytes], slots [int per needle], n_slots, rule_off, clause_off, literals) as am_rules_create takes them.
    IgnoreCase needles are lower-cased the way Searcher does; needles are deduplicated by text.  A slot's bit says "one of my needles occurred", so needles that occur in
    exactly the same clauses, all of them positively, share ONE slot -- a 5 000-word any_of used by one rule costs one bit per haystack.  A needle with a negated
    membership keeps a slot of its own: NOT a OR NOT b is not NOT (a OR b)."""
    texts, members = {}, []                                # needle text -> index; per needle the set of (clause, negated)
    clauses, rule_off = [], [0]
    for rule in rules:
        for clause in rule.clauses:
            ids = []
            for needle, neg in clause:
                t = _as_bytes(needle)
                if case == IGNORE_CASE:
                    t = lower_utf8(t)
                k = texts.setdefault(t, len(texts))
                if k == len(members):
                    members.append(set())
                members[k].add((len(clauses), bool(neg)))
                ids.append((k, bool(neg)))
            clauses.append(ids)
        rule_off.append(len(clauses))
    groups, slots = {}, []
    for k, m in enumerate(members):
        key = frozenset(m) if not any(neg for _, neg in m) else ("own", k)
        slots.append(groups.setdefault(key, len(groups)))
    clause_off, literals = [0], []
    for ids in clauses:
        seen = set()
        for k, neg in ids:
            lit = slots[k] | (RULE_NEGATE if neg else 0)
            if lit not in seen:
                seen.add(lit)
                literals.append(lit)
        clause_off.append(len(literals))
    return (list(texts), slots, len(groups), np.asarray(rule_off, np.uint64), np.asarray(clause_off, np.uint64), np.asarray(literals, np.uint32))


def _fired_bits(words, n_rules, n_hay):
    """bool[n_rules, n_hay] of uint64[n_rules, hay_words] (bit h % 64 of word h / 64)."""
    if n_rules == 0 or n_hay == 0:
        return np.zeros((n_rules, n_hay), bool)
    bits = np.unpackbits(np.ascontiguousarray(words).view(np.uint8).reshape(n_rules, -1), axis=1, bitorder="little")
    return bits[:, :n_hay].astype(bool)


def rules_fold_host(hay, val, n_hay, n_slots, rule_off, clause_off, literals):
    """amh_rules_fold: the sequential definition of am_rules_eval (host/rules.hpp rulesFold) over fold steps the caller brings -- (haystack, value) arrays in fold order
    -- and a program as am_rules_create takes it.  Runs without a device.  (fired_words uint64[n_rules, hay_words], labels, counts)."""
    hay, val = np.ascontiguousarray(hay, np.uint32), np.ascontiguousarray(val, np.uint32)
    ro, co, li = np.ascontiguousarray(rule_off, np.uint64), np.ascontiguousarray(clause_off, np.uint64), np.ascontiguousarray(literals, np.uint32)
    n_rules, hw = len(ro) - 1, (n_hay + 63) // 64
    fired, labels, counts = np.zeros(max(n_rules * hw, 1), np.uint64), np.zeros(max(n_hay, 1), np.uint32), np.zeros(max(n_rules, 1), np.uint64)
    _hcheck(libhost().amh_rules_fold(hay.ctypes.data if hay.size else None, val.ctypes.data if val.size else None, hay.size, n_hay, n_slots, ro.ctypes.data, co.ctypes.data,
                                     li.ctypes.data if li.size else None, n_rules, fired.ctypes.data, labels.ctypes.data, counts.ctypes.data))
    return fired[:n_rules * hw].reshape(n_rules, hw), labels[:n_hay], counts[:n_rules]


class RuleHits:
    """What a RuleSet found in a batch (am_rule_hits): rule-major bitmaps, first-rule-wins labels and per-rule counts in HBM, copied to the host on first use."""

    def __init__(self, handle):
        self._h = handle

    def __del__(self):
        if getattr(self, "_h", None):
            libam().am_rule_hits_free(self._h)
            self._h = None

    @property
    def handle(self):
        return self._h

    @property
    def n_hay(self):
        return int(libam().am_rule_hits_haystacks(self._h))

    @property
    def n_rules(self):
        return int(libam().am_rule_hits_rules(self._h))

    @property
    def hay_words(self):
        return int(libam().am_rule_hits_hay_words(self._h))

    def _host(self, fn, n, ctype):
        p = fn(self._h)
        if not p:
            check(AM_ERR_HIP)
        return np.ctypeslib.as_array(C.cast(p, C.POINTER(ctype)), shape=(max(n, 1),))[:n].copy()

    @property
    def fired_words(self):
        """np.uint64[n_rules, hay_words]: bit h % 64 of word h // 64 of row r is set iff rule r fires on haystack h; the bits beyond n_hay are zero."""
        return self._host(libam().am_rule_hits_fired, self.n_rules * self.hay_words, C.c_uint64).reshape(self.n_rules, self.hay_words)

    @property
    def fired(self):
        """bool[n_rules, n_hay]."""
        return _fired_bits(self.fired_words, self.n_rules, self.n_hay)

    @property
    def labels(self):
        """np.uint32[n_hay]: the smallest rule that fires, RULE_NONE where none does."""
        return self._host(libam().am_rule_hits_labels, self.n_hay, C.c_uint32)

    @property
    def counts(self):
        """np.uint64[n_rules]: the haystacks on which each rule fires."""
        return self._host(libam().am_rule_hits_counts, self.n_rules, C.c_uint64)

    def select(self, rule, first=False, invert=False, batch=None):
        """am_select_rule: the Selection of the haystacks of `batch` (the am_batch* the hits were made from) on which `rule` fires -- first=True: for which it is the
        FIRST rule that fires (label == rule); invert: the others."""
        return _select(lambda out: libam().am_select_rule(self._h, int(rule), RULE_FIRST if first else RULE_FIRED, int(bool(invert)), batch, out))


class RuleSet:
    """Many boolean rules over needles, evaluated from ONE scan (am_rules): rs = RuleSet(IGNORE_CASE, [Rule(all_of=["nike", "shoe"], none_of=["kids"]), ...]);
    rs.eval(texts) / rs.eval_batch(batch) give a RuleHits.  The needles are compiled to slots on the host (compile_rules); n_slots is the width of a haystack's row."""

    def __init__(self, case, rules):
        self.case = case
        self.rules = list(rules)
        self.needles, self.slots, self.n_slots, self.rule_off, self.clause_off, self.literals = compile_rules(case, self.rules)
        self._a = self._t = self._h = None                  # the automaton, its slot table and the program on the device, made on first use

    @classmethod
    def from_program(cls, case, needles, slots, n_slots, rule_off, clause_off, literals):
        """A rule set from a program the caller compiled: needles[i] carries slot slots[i] (a needle may appear several times, a value >= n_slots is skipped), the
        three arrays as am_rules_create takes them.  The needles are taken as they are (under IGNORE_CASE: lower-cased already)."""
        rs = cls(case, [])
        rs.needles, rs.slots, rs.n_slots = [_as_bytes(n) for n in needles], [int(v) for v in slots], int(n_slots)
        rs.rule_off, rs.clause_off, rs.literals = np.asarray(rule_off, np.uint64), np.asarray(clause_off, np.uint64), np.asarray(literals, np.uint32)
        rs.rules = [None] * (len(rs.rule_off) - 1)
        return rs

    def __del__(self):
        if getattr(self, "_h", None):
            libam().am_rules_destroy(self._h)
            self._h = None

    @property
    def automaton(self):
        if self._a is None:
            self._a = Automaton(self.needles, values=self.slots)
        return self._a

    @property
    def handle(self):
        if self._h is None:
            self._t = ValuesTable(self.automaton, n_needles=self.n_slots)
            h = _vp()
            check(libam().am_rules_create(self._t.handle, self.rule_off.ctypes.data, self.clause_off.ctypes.data, self.literals.ctypes.data if self.literals.size else None,
                                          len(self.rules), C.byref(h)))
            self._h = h
        return self._h

    def eval_batch(self, batch):
        """am_rules_eval_batch on a device-resident batch (an am_batch* handle)."""
        h = _vp()
        check(libam().am_rules_eval_batch(self.handle, self.case, batch, C.byref(h)))
        return RuleHits(h)

    def eval(self, texts):
        """am_rules_eval: the one-shot form on host texts."""
        s = _Slices(texts)
        h = _vp()
        check(libam().am_rules_eval(self.handle, self.case, s.arr, s.n, C.byref(h)))
        return RuleHits(h)

    def eval_host_mirror(self, texts):
        """The same through the C++ host mirror (host/rules.hpp rulesFold over the fold steps of amh_run_list): (fired bool[n_rules, n_hay], labels, counts)."""
        hay, _, val = self.automaton.run_batch_with_case(self.case, texts)
        words, labels, counts = rules_fold_host(hay, val, len(texts), self.n_slots, self.rule_off, self.clause_off, self.literals)
        return _fired_bits(words, len(self.rules), len(texts)), labels, counts


def _grep_texts(texts, sel):
    """(indices, [bytes]) of a selection over host texts: the texts are the caller's already, only the indices come back."""
    def text(t):
        if isinstance(t, tuple):
            t, off, ln = t
            t = bytes(t)
            return t[off:] if ln is None else t[off:off + ln]
        return bytes(t) if isinstance(t, np.ndarray) else _as_bytes(t)
    idx = sel.indices
    return idx, [text(texts[int(i)]) for i in idx]


def substitute_geometry():
    """(group_bytes, tile_bytes) of the splice's gather (am_substitute_geometry)."""
    g, t = C.c_uint32(0), C.c_uint32(0)
    libam().am_substitute_geometry(C.byref(g), C.byref(t))
    return int(g.value), int(t.value)


def batch_offsets(batch):
    """The n_hay + 1 byte offsets of an am_batch* handle (am_batch_read_offsets)."""
    n = int(libam().am_batch_haystacks(batch))
    offs = np.zeros(n + 1, np.uint64)
    check(libam().am_batch_read_offsets(batch, offs.ctypes.data))
    return offs


def batch_read_text(batch, first, n):
    """Bytes [first, first + n) of the concatenated text of an am_batch* handle (am_batch_read_text)."""
    buf = C.create_string_buffer(max(int(n), 1))
    check(libam().am_batch_read_text(batch, int(first), int(n), buf))
    return buf.raw[:int(n)]


def batch_to_bytes(batch):
    """(offsets np.uint64[n_hay + 1], [bytes per haystack]) of an am_batch* handle, through the batch accessors."""
    offs = batch_offsets(batch)
    whole = batch_read_text(batch, 0, int(offs[-1]))
    return offs, [whole[int(offs[i]):int(offs[i + 1])] for i in range(len(offs) - 1)]


class SubstTable:
    """The replacements beside a SpanTable on the device (am_subst_table): replacements[v] = the bytes that replace a match of value handle v, or a template -- a
    list or tuple of bytes / str / am.MATCH.  A table of plain replacements only is made by am_subst_table_create, as ever; one template among them makes it a table of
    templates (am_subst_table_create_templates)."""

    def __init__(self, span_table, replacements):
        self._t = span_table                                 # (the am_span_table must outlive the table)
        self.n_needles = span_table.n_needles
        replacements = list(replacements)
        self.templates = any(_is_template(x) for x in replacements)
        h = _vp()
        if not self.templates:
            self._pool, self._off = _pack_replacements(replacements, self.n_needles)
            check(libam().am_subst_table_create(span_table.handle, self._off.ctypes.data, self._pool or None, C.byref(h)))
        else:
            self._off, self._kind, self._lit_off, self._pool = _pack_templates(replacements, self.n_needles)
            check(libam().am_subst_table_create_templates(span_table.handle, self._off.ctypes.data, self._kind.ctypes.data, self._lit_off.ctypes.data, self._pool or None,
                                                          C.byref(h)))
        self._h = h

    def __del__(self):
        if getattr(self, "_h", None):
            libam().am_subst_table_destroy(self._h)
            self._h = None

    @property
    def handle(self):
        return self._h

    def _texts(self, call, raw):
        b = _vp()
        check(call(C.byref(b)))
        if raw:
            return b
        try:
            return batch_to_bytes(b)[1]
        finally:
            libam().am_batch_destroy(b)

    def substitute_batch(self, case, batch, raw=False):
        """am_substitute_batch on a device-resident batch (an am_batch* handle): the rewritten texts as a list of bytes.  raw: the new am_batch* itself, in HBM
        (the next device stage takes it; free with am_batch_destroy)."""
        return self._texts(lambda out: libam().am_substitute_batch(self._h, case, batch, out, None), raw)

    def substitute_texts(self, case, texts):
        """am_substitute: the one-shot form on host texts, a list of bytes."""
        s = _Slices(texts)
        return self._texts(lambda out: libam().am_substitute(self._h, case, s.arr, s.n, out), False)

    def splice(self, batch, spans_raw, raw=False):
        """am_batch_substitute: the splice alone over an am_spans* the caller holds (SpanTable.spans_batch(..., SPANS_LEFTMOST_LONGEST, raw=True) on `batch`)."""
        return self._texts(lambda out: libam().am_batch_substitute(batch, spans_raw, self._h, out), raw)


def _lower_needle(needle, lower_pairs):
    """The needle as the automaton of a Cased holds it: lower_utf8 under the built-in table; under the caller's pairs ASCII lower-casing and those pairs, a code point
    at a time (what am_automaton_create_ex lowers the haystack with)."""
    if lower_pairs is None:
        return lower_utf8(needle)
    table = {int(a): int(b) for a, b in lower_pairs}
    text = _as_bytes(needle).decode("utf-8")
    return "".join(chr(table.get(ord(c), ord(c) + 32 if "A" <= c <= "Z" else ord(c))) for c in text).encode("utf-8")


class _CasedAutomaton(Automaton):
    """The automaton of a Cased: lower-cased needles, and every span table its methods make carries the spellings (include/am.h "exact case")."""

    def __init__(self, lowered, given, exact, lower_pairs):
        super().__init__(lowered, lower_pairs=lower_pairs)
        self._given, self._spellings = given, exact

    def _span_table(self, whole_words=False, n_needles=None):
        exact = self._spellings if self._spellings is None or n_needles is None else self._spellings[:n_needles]
        return SpanTable(self, n_needles=n_needles, word_bytes=whole_words, exact=exact)

    def _needs_span_table(self, whole_words):
        return bool(whole_words) or self._spellings is not None

    def _group_names(self):
        return self._given                                   # (the groups of near name the needles as given)


class Cased:
    """A dictionary whose needles are case-insensitive or exact, needle by needle, in ONE scan (include/am.h "exact case").  needles: as given, in the spelling
    that counts for the exact ones.  exact: a mask with one boolean per needle, or a set (any container) of the needles that are exact.  The automaton holds the
    lower-cased needles, every call scans under IGNORE_CASE, and the span table carries exact[v] = needle v as given for the flagged needles: a span of such a needle
    is a row only where the text spells it that way -- filtered before the leftmost-longest selection, so every stage that reads spans sees the kept rows only.
      am.Cased(["US", "Apple", "nike"], exact=[1, 1, 0]).highlight(["us, US and NIKE's apple"], "<b>", "</b>") == [b"us, <b>US</b> and <b>NIKE</b>'s apple"]
    RuleSet, count_matrix, contains_any / contains_all and Replacer do not go through a span table and stay single-mode."""

    def __init__(self, needles, exact, lower_pairs=None):
        given = [_as_bytes(n) for n in needles]
        exact = list(exact) if isinstance(exact, (list, tuple, np.ndarray)) else exact
        if isinstance(exact, list) and len(exact) == len(given) and all(isinstance(x, (bool, int, np.integer, np.bool_)) for x in exact):
            mask = [bool(x) for x in exact]
        else:
            if isinstance(exact, list) and any(isinstance(x, (bool, int, np.integer, np.bool_)) for x in exact):
                raise AmError(AM_ERR_INVALID, "Cased: an exact mask has one boolean per needle (%d given, %d needles)" % (len(exact), len(given)))
            chosen = set(_as_bytes(x) for x in exact)
            unknown = chosen - set(given)
            if unknown:
                raise AmError(AM_ERR_INVALID, "Cased: %r is exact and not among the needles" % (sorted(unknown)[0],))
            mask = [n in chosen for n in given]
        if any(m and not n for m, n in zip(mask, given)):
            raise AmError(AM_ERR_INVALID, "Cased: the empty needle cannot be exact")
        self.needles = given
        self.exact = [n if m else None for n, m in zip(given, mask)]
        self.automaton = _CasedAutomaton([_lower_needle(n, lower_pairs) for n in given], given, self.exact if any(mask) else None, lower_pairs)

    def table(self, whole_words=False):
        """The SpanTable of this dictionary (with a word class where asked for): what the *_batch calls of the device stages take."""
        return self.automaton._span_table(whole_words)

    def spans(self, texts, leftmost_longest=False, whole_words=False, unit=BYTES):
        return self.automaton.spans(IGNORE_CASE, texts, leftmost_longest=leftmost_longest, whole_words=whole_words, unit=unit)

    def substitute(self, texts, replacements, whole_words=False):
        return self.automaton.substitute(IGNORE_CASE, texts, replacements, whole_words=whole_words)

    def highlight(self, texts, before, after, whole_words=False):
        return self.automaton.highlight(IGNORE_CASE, texts, before, after, whole_words=whole_words)

    def grep(self, texts, invert=False, whole_words=False):
        return self.automaton.grep(IGNORE_CASE, texts, invert=invert, whole_words=whole_words)

    def extract(self, texts, before=0, after=0, merged=False, leftmost_longest=True, whole_words=False):
        return self.automaton.extract(IGNORE_CASE, texts, before=before, after=after, merged=merged, leftmost_longest=leftmost_longest, whole_words=whole_words)

    def count_by_needle(self, texts, whole_words=False):
        """How often every needle occurs, spelled as it must be: np.uint64[len(needles)], the bincount of the spans(texts) rows."""
        if not self.needles:
            return np.zeros(0, np.uint64)
        return self.table(whole_words).count_by_needle_texts(IGNORE_CASE, texts)

    def score(self, texts, weights, whole_words=False):
        return self.automaton.score(IGNORE_CASE, texts, weights, whole_words=whole_words)

    def postings(self, texts, leftmost_longest=False, whole_words=False):
        return self.automaton.postings(IGNORE_CASE, texts, leftmost_longest=leftmost_longest, whole_words=whole_words)

    def doc_freq(self, texts, whole_words=False):
        return self.automaton.doc_freq(IGNORE_CASE, texts, whole_words=whole_words)

    def near(self, texts, groups, queries, whole_words=False):
        """Automaton.near over the kept rows; groups name the needles as given."""
        return self.automaton.near(IGNORE_CASE, texts, groups, queries, whole_words=whole_words)


class ImageAutomaton:
    """A device automaton attached to a serialised image (am_automaton_from_host_image): no build, no
    flatten.  It serves the image's case mode and returns raw records; machineValues stay with whoever
    built the automaton."""

    def __init__(self, image_bytes):
        buf = bytes(image_bytes)
        h = _vp()
        check(libam().am_automaton_from_host_image(buf, len(buf), C.byref(h)))
        self._h = h

    @classmethod
    def load(cls, path):
        with open(path, "rb") as f:
            return cls(f.read())

    def __del__(self):
        if getattr(self, "_h", None):
            libam().am_automaton_destroy(self._h)
            self._h = None

    @property
    def device(self):
        return self._h.value

    def run_records(self, case, texts):
        s = _Slices(texts)
        m = _vp()
        check(libam().am_run(self._h, case, s.arr, s.n, C.byref(m)))
        try:
            return matches_to_numpy(m)
        finally:
            libam().am_matches_free(m)

    def count_matches(self, case, texts):
        s = _Slices(texts)
        out = np.zeros(max(s.n, 1), np.uint64)
        check(libam().am_count(self._h, case, s.arr, s.n, out.ctypes.data))
        return out[:s.n]


def matches_to_numpy(m):
    n = int(libam().am_matches_size(m))
    if n == 0:
        return np.zeros(0, MATCH_DTYPE)
    p = libam().am_matches_data(m)
    if not p:
        raise AmError(AM_ERR_HIP, (libam().am_last_error() or b"").decode())
    return np.frombuffer((C.c_char * (n * MATCH_DTYPE.itemsize)).from_address(p), dtype=MATCH_DTYPE).copy()


def _csr_to_numpy(x, prefix, dtype):
    """(offsets np.uint64[n_hay + 1], items dtype[n]) of a CSR result handle whose accessors are am_<prefix>_size / _haystacks / _offsets / _data (host copies)."""
    lib = libam()
    n, n_hay = int(getattr(lib, prefix + "_size")(x)), int(getattr(lib, prefix + "_haystacks")(x))
    po, pd = getattr(lib, prefix + "_offsets")(x), getattr(lib, prefix + "_data")(x)
    if not po or not pd:
        raise AmError(AM_ERR_HIP, (lib.am_last_error() or b"").decode())
    offs = np.frombuffer((C.c_char * ((n_hay + 1) * 8)).from_address(po), dtype=np.uint64).copy()
    items = np.frombuffer((C.c_char * (n * dtype.itemsize)).from_address(pd), dtype=dtype).copy() if n else np.zeros(0, dtype)
    return offs, items


def _csr_call(call, to_numpy, free, raw):
    """call(out) makes a CSR result handle: the handle itself (raw: the caller frees it), or its host copies with the handle freed."""
    x = _vp()
    check(call(C.byref(x)))
    if raw:
        return x
    try:
        return to_numpy(x)
    finally:
        free(x)


def fragments_to_numpy(f):
    """(offsets np.uint64[n_hay + 1], fragments FRAGMENT_DTYPE[n]) of an am_fragments* result (host copies)."""
    return _csr_to_numpy(f, "am_fragments", FRAGMENT_DTYPE)


def matrix_to_numpy(x):
    """(offsets np.uint64[n_hay + 1], entries NEEDLE_COUNT_DTYPE[n]) of an am_needle_matrix* result (host copies)."""
    return _csr_to_numpy(x, "am_needle_matrix", NEEDLE_COUNT_DTYPE)


def spans_to_numpy(x):
    """(offsets np.uint64[n_hay + 1], spans SPAN_DTYPE[n]) of an am_spans* result (host copies)."""
    return _csr_to_numpy(x, "am_spans", SPAN_DTYPE)


def ranges_to_numpy(x):
    """(offsets np.uint64[n_hay + 1], ranges SPAN_RANGE_DTYPE[n]) of an am_ranges* result (host copies)."""
    return _csr_to_numpy(x, "am_ranges", SPAN_RANGE_DTYPE)


def matches_of_haystack(m, haystack):
    """The records of ONE haystack of a (possibly huge, device-resident) result as a numpy array: binary search + one small copy (am_matches_haystack_range / am_matches_copy)."""
    first, count = C.c_uint64(0), C.c_uint64(0)
    check(libam().am_matches_haystack_range(m, int(haystack), C.byref(first), C.byref(count)))
    out = np.zeros(count.value, MATCH_DTYPE)
    if count.value:
        check(libam().am_matches_copy(m, first.value, count.value, out.ctypes.data))
    return out


class Searcher:
    def __init__(self, case, needles):
        blob, offs = pack_texts(needles)
        h = _vp()
        _hcheck(libhost().amh_searcher_build(case, blob, offs.ctypes.data, len(needles), C.byref(h)))
        self._h = h
        self.case = case
        self._needles = [_as_bytes(n) for n in needles]
        self._ids = None                                     # the needle-id table of the selects, made on first use

    build = classmethod(lambda cls, case, needles: cls(case, needles))

    def __del__(self):
        if getattr(self, "_h", None):
            libhost().amh_searcher_free(self._h)
            self._h = None

    def set_case_sensitivity(self, case):
        libhost().amh_searcher_set_case(self._h, case)
        self.case = case

    def contains_any_batch(self, texts):
        s = _Slices(texts)
        out = np.zeros(max(s.n, 1), np.uint8)
        _hcheck(libhost().amh_searcher_contains_any(self._h, s.arr, s.n, out.ctypes.data))
        return out[:s.n].astype(bool)

    def contains_any(self, text):
        return bool(self.contains_any_batch([text])[0])

    def contains_all_batch(self, texts, host_fold=False):
        """Searcher.containsAll per haystack.  host_fold=True folds the records on the host (cross-check)."""
        s = _Slices(texts)
        out = np.zeros(max(s.n, 1), np.uint8)
        fn = libhost().amh_searcher_contains_all_host_fold if host_fold else libhost().amh_searcher_contains_all
        _hcheck(fn(self._h, s.arr, s.n, out.ctypes.data))
        return out[:s.n].astype(bool)

    def contains_all(self, text):
        return bool(self.contains_all_batch([text])[0])

    def _id_table(self):
        """buildNeedleIdSearcher (Searcher.hs:167-169) as the C ABI takes it: the needles with their indices as values, and machineValues in flat form beside them."""
        if self._ids is None:
            self._ids = ValuesTable(Automaton(self._needles))
        return self._ids

    def select_batch(self, batch, all=False, invert=False):
        """am_select_any_batch / am_select_all_batch (all=True) on a device-resident batch (an am_batch* handle) in this searcher's case mode: the Selection of the
        haystacks for which containsAny / containsAll holds (invert: does not hold)."""
        t = self._id_table()
        if all:
            return t.select_all_batch(self.case, batch, invert)
        return _select(lambda out: libam().am_select_any_batch(t._a.device, self.case, int(bool(invert)), batch, out))

    def grep_batch(self, texts, all=False, invert=False):
        """The texts that contain any needle (all=True: every needle), or -- invert -- those that do not, as (indices np.uint32, [bytes]).  The one-shot forms
        am_select_any / am_select_all: decided and compacted in HBM, the indices come back."""
        t = self._id_table()
        s = _Slices(texts)
        if all:
            return _grep_texts(texts, t.select_all_texts(self.case, texts, invert))
        return _grep_texts(texts, _select(lambda out: libam().am_select_any(t._a.device, self.case, int(bool(invert)), s.arr, s.n, out)))


class Replacer:
    def __init__(self, case, pairs, lower_pairs=None):
        nb, no = pack_texts([p[0] for p in pairs])
        rb, ro = pack_texts([p[1] for p in pairs])
        h = _vp()
        la = _LowerArrays(lower_pairs)
        _hcheck(libhost().amh_replacer_build_ex(case, nb, no.ctypes.data, rb, ro.ctypes.data, len(pairs), la.from_ptr, la.to_ptr, la.n, C.byref(h)))
        self._h = h
        self.pairs = list(pairs)

    build = classmethod(lambda cls, case, pairs: cls(case, pairs))

    @classmethod
    def _wrap(cls, handle, pairs):
        r = cls.__new__(cls)
        r._h = handle
        r.pairs = pairs
        return r

    def map_replacement(self, f):
        """Replacer.mapReplacement (Replacer.hs:135-141): new replacements, same needles, no rebuild."""
        fresh = [f(_as_bytes(rep)) for _, rep in self.pairs]
        rb, ro = pack_texts(fresh)
        h = _vp()
        _hcheck(libhost().amh_replacer_with_replacements(self._h, rb, ro.ctypes.data, C.byref(h)))
        return Replacer._wrap(h, [(n, rep) for (n, _), rep in zip(self.pairs, fresh)])

    @staticmethod
    def compose(first, second):
        """Replacer.compose (Replacer.hs:120-133): `second` after `first` as ONE replacer (the second's priorities renumbered to
        come after the first's); None when the case sensitivities differ."""
        h = _vp()
        _hcheck(libhost().amh_replacer_compose(first._h, second._h, C.byref(h)))
        return Replacer._wrap(h, first.pairs + second.pairs) if h.value else None

    def set_case_sensitivity(self, case):
        """Replacer.setCaseSensitivity (Replacer.hs:148-153): needles untouched."""
        h = _vp()
        _hcheck(libhost().amh_replacer_set_case(self._h, case, C.byref(h)))
        return Replacer._wrap(h, self.pairs)

    def __del__(self):
        if getattr(self, "_h", None):
            libhost().amh_replacer_free(self._h)
            self._h = None

    def run_batch(self, texts, max_len=-1, host_splice=False):
        """Replacer.run / runWithLimit on a batch.  host_splice=True keeps only the scans on the GPU
        (fold, sort and splice on the host) -- an independent cross-check of the device passes."""
        s = _Slices(texts)
        blob = _vp()
        offs = np.zeros(s.n + 1, np.uint64)
        nothing = np.zeros(max(s.n, 1), np.uint8)
        fn = libhost().amh_replacer_run_batch_host_splice if host_splice else libhost().amh_replacer_run_batch
        _hcheck(fn(self._h, s.arr, s.n, max_len, C.byref(blob), offs.ctypes.data, nothing.ctypes.data))
        try:
            raw = C.string_at(blob, int(offs[-1]))
        finally:
            libhost().amh_free_blob(blob)
        return [None if nothing[i] else raw[int(offs[i]):int(offs[i + 1])] for i in range(s.n)]

    @property
    def device(self):
        """am_replacer* for the raw ABI (am_replacer_run_batch on device-resident batches)."""
        h = _vp()
        _hcheck(libhost().amh_replacer_device(self._h, C.byref(h)))
        return h.value

    def run_priority(self, texts, thresholds):
        """One pass of the Replacer fold on the device (am_run_priority): (best priority per haystack, selected matches)."""
        s = _Slices(texts)
        thr = np.ascontiguousarray(thresholds, dtype=np.int64)
        best = np.zeros(max(s.n, 1), np.int64)
        p, n = _vp(), _sz(0)
        check(libam().am_run_priority(self.device, s.arr, s.n, thr.ctypes.data, best.ctypes.data, C.byref(p), C.byref(n)))
        try:
            k = int(n.value)
            ms = np.frombuffer((C.c_char * (k * PRIO_MATCH_DTYPE.itemsize)).from_address(p.value), dtype=PRIO_MATCH_DTYPE).copy() if k else np.zeros(0, PRIO_MATCH_DTYPE)
        finally:
            libam().am_prio_matches_free(p)
        return best[:s.n], ms

    def last_stats(self):
        """(passes, haystack bytes scanned over all passes) of the last run_batch."""
        a = np.zeros(2, np.uint64)
        libhost().amh_replacer_last_stats(self._h, a[0:].ctypes.data, a[1:].ctypes.data)
        return int(a[0]), int(a[1])

    def run(self, text):
        return self.run_batch([text])[0]

    def run_with_limit(self, max_len, text):
        return self.run_batch([text], max_len)[0]


class Splitter:
    """Data.Text.AhoCorasick.Splitter (build :64-67, split :84-85, splitIgnoreCase :96-97)."""

    def __init__(self, separator):
        b = _as_bytes(separator)
        h = _vp()
        _hcheck(libhost().amh_splitter_build(b, len(b), C.byref(h)))
        self._h = h

    build = classmethod(lambda cls, separator: cls(separator))

    def __del__(self):
        if getattr(self, "_h", None):
            libhost().amh_splitter_free(self._h)
            self._h = None

    def split_batch(self, texts, ignore_case=False):
        """The fragments of every text with the fold on the host (host/splitter.hpp splitBatch)."""
        return self._blob_lists(libhost().amh_splitter_split_batch, texts, ignore_case)

    def _blob_lists(self, fn, texts, ignore_case):
        """Lists of fragments out of one of the facade's blob + offsets + per-haystack-count calls."""
        s = _Slices(texts)
        blob, offs = _vp(), _vp()
        nf = C.c_uint64(0)
        per = np.zeros(max(s.n, 1), np.uint32)
        _hcheck(fn(self._h, 1 if ignore_case else 0, s.arr, s.n, C.byref(blob), C.byref(offs), C.byref(nf), per.ctypes.data))
        try:
            o = np.ctypeslib.as_array(C.cast(offs, _u64p), shape=(nf.value + 1,)).copy()
            raw = C.string_at(blob, int(o[-1]))
        finally:
            libhost().amh_free_blob(blob)
            libhost().amh_free_u64(offs)
        out, k = [], 0
        for i in range(s.n):
            out.append([raw[int(o[k + j]):int(o[k + j + 1])] for j in range(int(per[i]))])
            k += int(per[i])
        return out

    def split_batch_device(self, texts, ignore_case=False):
        """The same lists of fragments with the fold on the device (am_split: stepAccum in HBM, csrc/am_split.hip); what crosses the wire is (start, length) per fragment."""
        return self._blob_lists(libhost().amh_splitter_split_batch_device, texts, ignore_case)

    def fragments_texts(self, texts, ignore_case=False):
        """TEST AID: (offsets[n + 1], fragments) of host texts through the C++ host mirror's splitBatchFragments (am_split)."""
        s = _Slices(texts)
        offs, frags = _vp(), _vp()
        nf = C.c_uint64(0)
        _hcheck(libhost().amh_splitter_fragments_batch(self._h, 1 if ignore_case else 0, s.arr, s.n, C.byref(offs), C.byref(frags), C.byref(nf)))
        try:
            o = np.ctypeslib.as_array(C.cast(offs, _u64p), shape=(s.n + 1,)).copy()
            fr = np.ctypeslib.as_array(C.cast(frags, _u64p), shape=(max(int(nf.value), 1) * 2,)).copy()[:int(nf.value) * 2].view(FRAGMENT_DTYPE)
        finally:
            libhost().amh_free_u64(offs)
            libhost().amh_free_u64(frags)
        return o, fr

    @property
    def device(self):
        """TEST AID (like Replacer.device): the am_splitter* for calls on the raw ABI."""
        h = _vp()
        _hcheck(libhost().amh_splitter_device(self._h, C.byref(h)))
        return h.value

    def set_kernel(self, k):
        """TEST AID: the scan route of the separator's automaton (am_automaton_set_kernel), so that the tests reach every route."""
        h = _vp()
        _hcheck(libhost().amh_splitter_automaton(self._h, C.byref(h)))
        check(libam().am_automaton_set_kernel(h, k))

    def split_fragments(self, batch, ignore_case=False):
        """TEST / MEASUREMENT AID: am_split_batch on an am_batch* handle, the raw am_fragments* result (free it with libam().am_fragments_free); fragments_batch and
        lines_batch are the front end."""
        f = _vp()
        check(libam().am_split_batch(self.device, IGNORE_CASE if ignore_case else CASE_SENSITIVE, batch, C.byref(f)))
        return f

    def fragments_batch(self, batch, ignore_case=False):
        """am_split_batch on a device-resident batch (an am_batch* handle): (offsets np.uint64[n_hay + 1], fragments FRAGMENT_DTYPE[offsets[-1]]); the fragments of
        haystack i are fragments[offsets[i]:offsets[i + 1]], start and len in bytes relative to the haystack."""
        f = self.split_fragments(batch, ignore_case)
        try:
            return fragments_to_numpy(f)
        finally:
            libam().am_fragments_free(f)

    def lines_batch(self, batch, ignore_case=False):
        """document -> lines without leaving HBM: splits the batch and gathers the fragments into a new batch (am_batch_from_fragments), one haystack per fragment.
        Returns (am_batch* handle of the new batch -- destroy it with libam().am_batch_destroy --, offsets np.uint64[n_hay + 1] that map a line back to its document)."""
        f = self.split_fragments(batch, ignore_case)
        try:
            nb = _vp()
            check(libam().am_batch_from_fragments(batch, f, C.byref(nb)))
            n_hay = int(libam().am_fragments_haystacks(f))
            p = libam().am_fragments_offsets(f)
            if not p:
                libam().am_batch_destroy(nb)
                raise AmError(AM_ERR_HIP, (libam().am_last_error() or b"").decode())
            return nb, np.frombuffer((C.c_char * ((n_hay + 1) * 8)).from_address(p), dtype=np.uint64).copy()
        finally:
            libam().am_fragments_free(f)

    def split(self, text):
        return self.split_batch([text], False)[0]

    def split_ignore_case(self, text):
        return self.split_batch([text], True)[0]


DEBUG_SWITCHES = ("AM_SF_TRACE", "AM_SF_POOL_BLOCKS", "AM_SF_NO_CHILDREN", "AM_DFA", "AM_DFA_CHUNK", "AM_DFA_RARE_PERMILLE", "AM_DFA_MIN_KIB", "AM_DFA_TUNE", "AM_DFA_NO_CHAINS", "AM_FLATTEN_TRACE", "AM_FLATTEN_SERIAL", "AM_NO_IDS_SCAN",
                  "AM_RP_FULL_SCANS", "AM_RP_PIECES", "AM_RP_PARALLEL_FOLD", "AM_RP_GROUPS", "AM_RP_NO_FUSE", "AM_RP_NO_SPIN",
                  "AM_RP_MAT_MAIN", "AM_RP_NO_RANGE_REUSE", "AM_RP_TRACE", "AM_RP_LDS", "AM_RP_LOOP", "AM_RUN_SEGMENTS", "AM_HIST_RECORDS_MIB", "AM_HIST_TRACE", "AM_HIST_FLUSH_TILES", "AM_SPLIT_CHAIN_LIMIT", "AM_SPANS_CHAIN_LIMIT", "AM_RULES_ROWS_MIB")


def debug_set(name, value):
    """A test / measurement switch of libam (csrc/am_config.h) by the name of its environment variable; -1 = unset.  No switch changes a result."""
    check(libam().am_debug_set(name.encode(), int(value)))


def debug_reset():
    for name in DEBUG_SWITCHES:
        debug_set(name, -1)


def resident_waves():
    """am_debug_resident_waves: (wavefronts a CU of the current device really runs at once -- 32 by the architecture, 16 on boxes where a second set of 16 waits for the
    first --, ms of the 16-per-CU launch, ms of the 32-per-CU launch)."""
    one, two = C.c_float(0), C.c_float(0)
    check(libam().am_debug_resident_waves(C.byref(one), C.byref(two)))
    return (32 if two.value < 1.5 * one.value else 16), round(one.value, 3), round(two.value, 3)


def hist_adds():
    """am_debug_hist_adds: (adds absorbed in LDS, adds that went to HBM one by one, flush adds) of the k_needle_hist launches under AM_HIST_TRACE since the last read."""
    a = np.zeros(3, np.uint64)
    check(libam().am_debug_hist_adds(a.ctypes.data))
    return int(a[0]), int(a[1]), int(a[2])


def needle_matrix_limits():
    """am_debug_needle_matrix_limits: {wave_row, lds_row, lds_slots, chunk_records} of csrc/am_matrix.hip."""
    out = (C.c_uint32 * 4)()
    check(libam().am_debug_needle_matrix_limits(out))
    return dict(zip(("wave_row", "lds_row", "lds_slots", "chunk_records"), (int(v) for v in out)))


def sf_unit_chunks(total_bytes, n_cu=0):
    """am_debug_sf_unit_chunks: KiB chunks per k_sf / k_dense work unit of a batch of total_bytes; n_cu = 0: the current device's compute units."""
    uc = int(libam().am_debug_sf_unit_chunks(int(total_bytes), int(n_cu)))
    if uc == 0:
        raise AmError(AM_ERR_NO_DEVICE, (libam().am_last_error() or b"").decode("utf-8", "replace"))
    return uc


SF_MODES = ("count", "emit", "any", "ids")


def decode_sf_variant(word):
    """The word of am_debug_sf_last_variant (include/am_debug.h) as a dict of k_sf's template arguments; None for 0 (no k_sf launch)."""
    word = int(word)
    if not word & 1:
        return None
    return {"ic": bool(word & 2), "mode": SF_MODES[(word >> 2) & 3], "ilp": (word >> 4) & 3, "lw": (word >> 16) & 255, "short": bool(word & 64), "dbg": bool(word & 128),
            "light": bool(word & 256), "children": bool(word & 512)}


def sf_last_variant():
    """am_debug_sf_last_variant: the k_sf instantiation this process launched last, as decode_sf_variant gives it; None when none ran since the last read (the read clears)."""
    return decode_sf_variant(libam().am_debug_sf_last_variant())


SF_VARIANT_W2 = 1 << 10


def sf_last_variant_w2():
    """One read of am_debug_sf_last_variant as (decode_sf_variant's dict, W2): W2 = the launch filtered with the derived two-word filter (bit 10, which the dict leaves out)."""
    word = int(libam().am_debug_sf_last_variant())
    return decode_sf_variant(word), bool(word & SF_VARIANT_W2)


def bounds_report():
    """(failed index assertions, line of the first, translation units that carry assertions) of a -DAM_BOUNDS_CHECK build; (0, 0, 0) in the product build."""
    f, l, u = C.c_uint64(0), C.c_uint32(0), C.c_uint32(0)
    check(libam().am_debug_bounds_report(C.byref(f), C.byref(l), C.byref(u)))
    return int(f.value), int(l.value), int(u.value)


def image_version():
    """kImageVersion of the flattened automaton image this build produces (am_image_version()), so that tools and bench.py can
    refuse measurements taken with another layout."""
    return int(libam().am_image_version())


def lower_code_point(cp):
    return int(libam().am_lower_code_point(cp))


def unlower_code_point(cp):
    buf = (C.c_uint32 * 16)()
    n = libam().am_unlower_code_point(cp, buf, 16)
    return [int(buf[i]) for i in range(n)]


def lower_utf8(text):
    b = _as_bytes(text)
    out = C.create_string_buffer(len(b) * 4 + 4)
    n = libhost().amh_lower_utf8(b, len(b), out, len(b) * 4 + 4)
    return out.raw[:n]


def is_case_invariant(text, lower_pairs=None):
    """Utf8.isCaseInvariant (Utf8.hs:169-171)."""
    b = _as_bytes(text)
    la = _LowerArrays(lower_pairs)
    r = libhost().amh_is_case_invariant(b, len(b), la.from_ptr, la.to_ptr, la.n)
    if r < 0:
        raise AmError(AM_ERR_INVALID, (libhost().amh_last_error() or b"").decode("utf-8", "replace"))
    return bool(r)


def needle_casings(text, lower_pairs=None):
    """Automaton.needleCasings (Automaton.hs:555-566): list[bytes], in the reference's order."""
    b = _as_bytes(text)
    la = _LowerArrays(lower_pairs)
    blob, offs, n = _vp(), _vp(), C.c_uint64(0)
    _hcheck(libhost().amh_needle_casings(b, len(b), la.from_ptr, la.to_ptr, la.n, C.byref(blob), C.byref(offs), C.byref(n)))
    try:
        o = np.ctypeslib.as_array(C.cast(offs, _u64p), shape=(n.value + 1,)).copy()
        raw = C.string_at(blob, int(o[-1]))
    finally:
        libhost().amh_free_blob(blob)
        libhost().amh_free_u64(offs)
    return [raw[int(o[i]):int(o[i + 1])] for i in range(int(n.value))]


def skip_code_points_backwards(text, index, n):
    b = _as_bytes(text)
    r = libhost().amh_skip_code_points_backwards(b, len(b), index, n)
    if r < 0:
        raise IndexError("Invalid use of skipCodePointsBackwards")
    return int(r)


def device_info():
    n_cu, hbm = C.c_int(0), C.c_size_t(0)
    name = C.create_string_buffer(64)
    check(libam().am_device_info(C.byref(n_cu), C.byref(hbm), name, 64))
    return {"n_cu": n_cu.value, "hbm_bytes": hbm.value, "arch": name.value.decode()}
