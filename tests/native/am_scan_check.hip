// am_scan_check.hip -- TEST-ONLY (libam_scancheck.so, build.build_scancheck): csrc/am_scan.hip included TEXTUALLY and compiled with the flags libam.so gives it, so
// the kernels the tests below run are the kernels the product carries, and its launchers behind a C interface that takes host arrays.  The product exports none of
// them: about forty call sites use them, always on what other kernels hand them.  tests/test_gpu_scan_sums.py holds them to numpy's cumsum on uint64.
//
// Every call allocates its device buffers, uploads the caller's `out` array -- n elements and a GUARD of amsc_guard_items() more, filled by the caller -- runs ONE
// launcher on the null stream and downloads all of `out` again: what lies beyond n, and with n == 0 everything, must come back as it went in.
// Return value: the launcher's hipError_t; a failure of the plumbing around it (allocation, copies, synchronisation) as -(its hipError_t).
// amsc_limits reports the constants the seams of three test files sit on, so that no test writes one of them down.
#include "am_scan.hip"

#include <vector>

#include "am_near.h"

#define AMSC_API extern "C" __attribute__((visibility("default")))

namespace {

constexpr uint64_t kGuard = 64;

// a device buffer of at least one element that frees itself
struct Buf {
    void* p = nullptr;
    hipError_t err;
    explicit Buf(size_t bytes) { err = hipMalloc(&p, bytes ? bytes : 8); }
    ~Buf() { if (p) (void)hipFree(p); }
    Buf(const Buf&) = delete;
    Buf& operator=(const Buf&) = delete;
};

inline hipError_t up(const Buf& b, const void* src, size_t bytes) { return bytes ? hipMemcpy(b.p, src, bytes, hipMemcpyHostToDevice) : hipSuccess; }
inline hipError_t down(void* dst, const Buf& b, size_t bytes) { return bytes ? hipMemcpy(dst, b.p, bytes, hipMemcpyDeviceToHost) : hipSuccess; }

#define AMSC_TRY(expr) do { const hipError_t e_ = (expr); if (e_ != hipSuccess) return -(int)e_; } while (0)

// the launch itself and everything behind it: the launcher's own error first, then what the stream reports
inline int finish(hipError_t launched)
{
    const hipError_t sync = hipDeviceSynchronize();
    if (launched != hipSuccess) { (void)hipGetLastError(); return (int)launched; }
    return sync == hipSuccess ? 0 : -(int)sync;
}

template <class T>
int scan_call(const T* in, uint64_t n, int64_t temp_bytes, uint64_t* out,
              hipError_t (*launch)(void*, size_t, const T*, uint64_t*, uint64_t, hipStream_t))
{
    size_t full = 0;
    AMSC_TRY(am::dev::scan_temp_bytes(n, &full));
    const size_t claimed = temp_bytes < 0 ? full : (size_t)temp_bytes;      // what the launcher is told; the buffer itself is never smaller than `full`
    Buf d_in(n * sizeof(T)), d_out((n + kGuard) * sizeof(uint64_t)), d_tmp(claimed > full ? claimed : full);
    AMSC_TRY(d_in.err); AMSC_TRY(d_out.err); AMSC_TRY(d_tmp.err);
    AMSC_TRY(up(d_in, in, n * sizeof(T)));
    AMSC_TRY(up(d_out, out, (n + kGuard) * sizeof(uint64_t)));
    const int rc = finish(launch(d_tmp.p, claimed, (const T*)d_in.p, (uint64_t*)d_out.p, n, nullptr));
    AMSC_TRY(down(out, d_out, (n + kGuard) * sizeof(uint64_t)));
    return rc;
}

}  // namespace

AMSC_API uint64_t amsc_guard_items() { return kGuard; }

// out7: elements per tile of launch_scan / launch_scan64 (and per sweep of k_scan_jobs), tiles per sweep of k_scan_tiles, candidates per tile of the spans' prefix
// maximum, its lanes per workgroup, tiles per sweep of k_spans_tiles_max, the needles whose masks k_near_bits stages in LDS, jobs per launch_scan_jobs
AMSC_API void amsc_limits(uint64_t* out7)
{
    using namespace am::dev;
    out7[0] = scan_tile_items();
    out7[1] = kScanThreads;                                 // (k_scan_tiles: one tile sum per lane and sweep)
    out7[2] = kSpansMaxTile;
    out7[3] = kSpThreads;
    out7[4] = kSpThreads;                                   // (k_spans_tiles_max: one tile maximum per lane and sweep)
    out7[5] = kNearLdsNeedles;
    out7[6] = sizeof(ScanJobs::j) / sizeof(ScanJob);
}

// bytes of temporary storage scan_temp_bytes asks for
AMSC_API uint64_t amsc_scan_temp_bytes(uint64_t n)
{
    size_t b = 0;
    (void)am::dev::scan_temp_bytes(n, &b);
    return b;
}

// temp_bytes < 0: what scan_temp_bytes says; otherwise the size the launcher is told it has
AMSC_API int amsc_scan32(const uint32_t* in, uint64_t n, int64_t temp_bytes, uint64_t* out) { return scan_call<uint32_t>(in, n, temp_bytes, out, am::dev::launch_scan); }
AMSC_API int amsc_scan64(const uint64_t* in, uint64_t n, int64_t temp_bytes, uint64_t* out) { return scan_call<uint64_t>(in, n, temp_bytes, out, am::dev::launch_scan64); }

// one job of a launch_scan_jobs call.  The job sums n_dev_value + n elements when has_n_dev (n_dev_value goes into a device word of its own), n otherwise; `in`
// holds that many elements of 4 (kind 0) or 8 (kind 1) bytes, `out` that many and the guard
struct AmscJob { const void* in; uint64_t* out; uint64_t n; uint64_t n_dev_value; uint32_t kind; uint32_t has_n_dev; };

AMSC_API int amsc_scan_jobs(const AmscJob* jobs, uint32_t n_jobs)
{
    am::dev::ScanJobs sj{};
    if (n_jobs > sizeof(sj.j) / sizeof(sj.j[0])) return -(int)hipErrorInvalidValue;
    std::vector<Buf*> held;
    struct Release { std::vector<Buf*>& v; ~Release() { for (Buf* b : v) delete b; } } release{held};
    std::vector<Buf*> outs;
    for (uint32_t k = 0; k < n_jobs; k++) {
        const AmscJob& j = jobs[k];
        const uint64_t total = j.n + (j.has_n_dev ? j.n_dev_value : 0), width = j.kind ? 8 : 4;
        Buf* d_in = new Buf(total * width); held.push_back(d_in);
        Buf* d_out = new Buf((total + kGuard) * sizeof(uint64_t)); held.push_back(d_out); outs.push_back(d_out);
        Buf* d_n = new Buf(sizeof(uint64_t)); held.push_back(d_n);
        AMSC_TRY(d_in->err); AMSC_TRY(d_out->err); AMSC_TRY(d_n->err);
        AMSC_TRY(up(*d_in, j.in, total * width));
        AMSC_TRY(up(*d_out, j.out, (total + kGuard) * sizeof(uint64_t)));
        AMSC_TRY(up(*d_n, &j.n_dev_value, sizeof(uint64_t)));
        am::dev::ScanJob& d = sj.j[k];
        d.in32 = j.kind ? nullptr : (const uint32_t*)d_in->p;
        d.in64 = j.kind ? (const uint64_t*)d_in->p : nullptr;
        d.out = (uint64_t*)d_out->p;
        d.n = j.n;
        d.n_dev = j.has_n_dev ? (const uint64_t*)d_n->p : nullptr;
    }
    sj.n_jobs = n_jobs;
    const int rc = finish(am::dev::launch_scan_jobs(sj, nullptr));
    for (uint32_t k = 0; k < n_jobs; k++) {
        const uint64_t total = jobs[k].n + (jobs[k].has_n_dev ? jobs[k].n_dev_value : 0);
        AMSC_TRY(down(jobs[k].out, *outs[k], (total + kGuard) * sizeof(uint64_t)));
    }
    return rc;
}

// out[i] = base + local[i] (local null: base); `out` has n elements and the guard
AMSC_API int amsc_offsets_rebase(const uint64_t* local, uint64_t n, uint64_t base, uint64_t* out)
{
    Buf d_local(n * sizeof(uint64_t)), d_out((n + kGuard) * sizeof(uint64_t));
    AMSC_TRY(d_local.err); AMSC_TRY(d_out.err);
    if (local) AMSC_TRY(up(d_local, local, n * sizeof(uint64_t)));
    AMSC_TRY(up(d_out, out, (n + kGuard) * sizeof(uint64_t)));
    const int rc = finish(am::dev::launch_offsets_rebase(local ? (const uint64_t*)d_local.p : nullptr, n, base, (uint64_t*)d_out.p, nullptr));
    AMSC_TRY(down(out, d_out, (n + kGuard) * sizeof(uint64_t)));
    return rc;
}
