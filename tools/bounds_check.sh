#!/bin/bash
# Index assertions inside the kernels (csrc/am_bounds.h), run ON THE GPU BOX: GPU sanitizers are not available on this pool, so a -DAM_BOUNDS_CHECK build of libam
# checks its own LDS queue indices, pool slots and image offsets (k_sf, k_dfa / k_dfa_place, k_rp_lds, k_idset, k_fold_hash, k_needle_hist, k_split_*, k_mx_*, k_spans_*, k_subst_*, k_subst_tpl_*, k_needle_hist_words, k_select_*, k_hay_flags_spans, k_extract_*, k_coords_*, k_dense, k_rules_eval, k_rule_flags, k_score, k_score_words, k_topk_*, k_score_range, k_near_*, k_post_*) while the parity tests run over it; tests/conftest.py fails the
# session if am_debug_bounds_report counts anything.  The instrumented libraries live in build/bounds/ (AM_LIB_DIR), apart from the product's.
#   /usr/local/graft/bin/gpurun --timeout 1500 -- 'bash tools/bounds_check.sh'
set -e
R=$(cd "$(dirname "$0")/.." && pwd)
export AM_LIB_DIR=$R/build/bounds AM_BOUNDS_CHECK=1
mkdir -p "$AM_LIB_DIR"
cd "$R"
python -c "import alfred_margaret_amd as am; print(sorted(am.build.build_all()))"
python -m pytest tests/test_gpu_parity.py tests/test_gpu_dfa.py tests/test_gpu_dfa_tiers.py tests/test_gpu_rploop.py tests/test_gpu_replacer_priorities.py tests/test_gpu_configs.py tests/test_gpu_needle_counts.py tests/test_gpu_needle_matrix.py tests/test_gpu_splitter_device.py tests/test_gpu_spans.py tests/test_gpu_substitute.py tests/test_gpu_templates.py tests/test_gpu_words.py tests/test_gpu_select.py tests/test_gpu_extract.py tests/test_gpu_coords.py tests/test_gpu_derived_batches.py tests/test_gpu_dense_units.py tests/test_gpu_sf_variants.py tests/test_gpu_sf_chunk_loop.py tests/test_gpu_long_needles.py tests/test_gpu_rules.py tests/test_gpu_score.py tests/test_gpu_near.py tests/test_gpu_postings.py tests/test_gpu_postings_sort.py tests/test_gpu_record_folds.py tests/test_gpu_scan_sums.py -m gpu -x -q -k "fragment or soak or pool or dfa or loop or cfg5 or walk or priorit or needle or splitter_device or spans or substitute or templates or words or select or extract or coords or derived or dense_units or sf_variants or rule or score or near or postings or folds or scan_sums" "$@" | tail -15; exit ${PIPESTATUS[0]}
