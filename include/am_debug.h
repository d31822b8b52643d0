/*
 * am_debug.h -- the entry points libam.so exports for TESTS AND MEASUREMENTS, next to the product ABI of include/am.h.  Nothing here is
 * needed by (or meant for) a caller of the library: a Haskell / C host binds am.h only.  None of these functions changes a result (nor does any switch am_debug_set knows).
 */
#ifndef AM_DEBUG_H
#define AM_DEBUG_H

#include "am.h"

#ifdef __cplusplus
extern "C" {
#endif

/* A test / measurement switch of csrc/am_config.h by the name of its environment variable ("AM_RP_LOOP", "AM_SF_POOL_BLOCKS", ...);
 * value -1 = unset.  AM_ERR_INVALID: no such switch. */
AM_API int am_debug_set(const char* name, long value);
/* Page-locked staging memory of all threads, living or parked (the leak test). */
AM_API uint64_t am_debug_pinned_bytes(void);
/* Bytes of device memory in the library's own buffers (csrc/am_host.h DevBuf: batches and their workspaces, the tables of replacers and needle ids, cached
 * Replacer sessions, fragments): back at its earlier value once every handle and result is destroyed and am_release_device_memory was called (the leak test).
 * Automaton images, record arrays and result slabs are not counted. */
AM_API uint64_t am_debug_device_buffer_bytes(void);
/* Cycle sums per k_sf phase / per-wavefront record counts of launches made under AM_SF_TRACE (tools/phase_timing.py). */
AM_API int am_debug_sf_phase_cycles(uint64_t* out5);
AM_API int am_debug_sf_wave_records(uint64_t* out, size_t n_waves);
/* Haystacks the calling process's last one-kernel Replacer run finished with their lists in LDS (k_rp_lds); the rest took k_rp_loop. */
AM_API uint32_t am_debug_rp_lds_haystacks(void);
/* The general AC-walk kernel (k_ac) is test infrastructure and lives in libam_check.so (tests/native/am_ac.hip).  Loading that library
 * hands its launcher to libam through this call; `launcher` is am::dev::launch_ac of a build with the same csrc/am_device.h
 * (image_version must equal am_image_version()), NULL takes it away again.  Without a launcher am_automaton_set_kernel(a, 1) makes every
 * scan of `a` fail with AM_ERR_UNSUPPORTED. */
AM_API int am_debug_set_general_kernel(void* launcher, uint32_t image_version);
/* A -DAM_BOUNDS_CHECK build of the library (tools/bounds_check.sh) compiles index assertions into its kernels (csrc/am_bounds.h: LDS queue indices, pool slots,
 * image offsets).  *failed_out = assertions that failed on the current device since the library was loaded, *first_line_out = source line of the first one (0: none),
 * *checked_units_out = translation units that carry assertions: 0 in the product build, where the call reports nothing and costs nothing. */
AM_API int am_debug_bounds_report(uint64_t* failed_out, uint32_t* first_line_out, uint32_t* checked_units_out);
/* How many wavefronts does a CU of the current device really run at the same time?  A spinning kernel is launched with 16 and with 32 wavefronts per CU (workgroups of 1024 and of
 * 256 threads, 4 KiB of LDS, a handful of registers): *one_ms_out / *two_ms_out = the launch times.  Equal times: 32 are resident, as the architecture says; twice the time: the
 * second half waited for the first (seen on the GPU pool during round 6: k_dfa, k_rp_lds and the small-filter k_sf, which count on two workgroups per CU, lose 10-45 % there).
 * bench.py prints the answer as `machine.resident_waves_per_cu`. */
AM_API int am_debug_resident_waves(float* one_ms_out, float* two_ms_out);

/* Under AM_HIST_TRACE the launches of k_needle_hist (am_count_by_needle*, csrc/am_hist.hip) run their instrumented instantiation: out3[0] = adds the workgroups' LDS tables
 * absorbed, out3[1] = adds that went to HBM one by one (slot conflicts, values far down a long list), out3[2] = adds of the flushes (one per live slot), summed over the
 * calls since the last read; reading clears the sums (out3 NULL: only clears).  tests/measure/needle_counts.py. */
AM_API int am_debug_hist_adds(uint64_t* out3);

/* Rounds of pointer doubling the last am_split_batch / am_split of the process needed (csrc/am_split.hip k_split_double): 0 when no chain of overlapping matches was longer
 * than the walk limit (AM_SPLIT_CHAIN_LIMIT), else about log2 of the separators kept in the longest chain.  tests/measure/splitter.py. */
AM_API uint32_t am_debug_split_rounds(void);

/* The limits the design of am_count_matrix* (csrc/am_matrix.hip) turns on: out4[0] = entries up to which a row is ordered inside one wavefront, out4[1] = entries up to which
 * a workgroup orders it in LDS (longer rows are ranked through a bitmap of n_needles bits), out4[2] = slots of a workgroup's LDS table of (haystack, needle) keys,
 * out4[3] = records a workgroup combines between two flushes of that table.  The tests sit on these. */
AM_API int am_debug_needle_matrix_limits(uint32_t* out4);

/* The work-unit geometry of the suffix-filter route (csrc/am_kernels.hip sf_unit_chunks, and nothing else): KiB chunks per k_sf / k_dense work unit of a batch of
 * total_bytes on a device with n_cu compute units; n_cu <= 0: the current device's (0 is returned when there is none).  With n_cu > 0 the call is pure and needs no
 * device.  The tests of the dense pass (tests/test_gpu_dense_units.py) take their batch sizes from it. */
AM_API uint32_t am_debug_sf_unit_chunks(uint64_t total_bytes, int n_cu);

/* The k_sf instantiation the calling process's last suffix-filter launch ran (csrc/am_kernels.hip launch_sf_t chooses among about thirty from the image's header, the
 * mode and the batch size; a caller cannot see the choice).  Bit 0: valid; bit 1: IgnoreCase; bits 2-3: mode (0 count, 1 emit, 2 any, 3 ids); bits 4-5: ILP (1 or 2);
 * bit 6: SHORT (tier probes for needles of 1-3 bytes); bit 7: DBG (AM_SF_TRACE); bit 8: the light configuration (256-thread workgroups); bit 9: CHILDREN;
 * bits 16-23: LW (0 or 15).  Reading clears the word: 0 = no k_sf launch since the last read (another kernel took the call, or nothing was launched: an empty batch,
 * an automaton without suffix keys).  tests/test_gpu_sf_variants.py.  Bit 10: W2, the launch filtered with the two-word filter derived from the image's keys
 * (csrc/am_image.h scan2_mask; tests/test_gpu_scan2_filter.py). */
AM_API uint32_t am_debug_sf_last_variant(void);

#ifdef __cplusplus
}
#endif
#endif /* AM_DEBUG_H */
