// am_post_check.hip -- TEST-ONLY (libam_postcheck.so, build.build_postcheck): csrc/am_postings.hip included TEXTUALLY and compiled with the flags libam.so gives it,
// so the kernels the tests below run are the kernels the product carries, and its seven launchers behind a C interface that takes host arrays.  The product exports
// none of them: am_postings.cpp runs them in one fixed sequence, always on what the launcher before handed on.  tests/test_gpu_postings_sort.py holds each of them to
// its contract in am_postings.h, written in numpy (tests/postings_cases.py).
//
// Every call allocates its device buffers, uploads the inputs and every OUTPUT array -- its elements and a GUARD of ampc_guard_items() more, filled by the caller --
// runs ONE launcher on the null stream, synchronises and downloads the outputs whole: what the launcher does not own must come back as it went in.
// `n` is what the launcher is told; `n_buf` is what the arrays of n elements really hold.  They are equal except where a launcher is to refuse a count before it
// touches anything (n >= kPostMaxSpans): a count the launcher would accept and the arrays do not hold is turned away HERE, as is a count table smaller than the pass
// needs, so that no call can make a kernel write beyond a buffer.
// Return value: the launcher's hipError_t; a failure of the plumbing around it (arguments, allocation, copies, synchronisation) as -(its hipError_t).
// In an AM_BOUNDS_CHECK build (tools/bounds_check.sh) the kernels' index assertions count into words of this library, which ampc_bounds reads.
// ampc_limits and ampc_plan report the constants and the plan the seams of the tests sit on, so that no test writes one of them down.
#include "am_postings.hip"

#define AMPC_API extern "C" __attribute__((visibility("default")))

namespace {

using namespace am::dev;

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

#define AMPC_TRY(expr) do { const hipError_t e_ = (expr); if (e_ != hipSuccess) return -(int)e_; } while (0)
#define AMPC_REQUIRE(cond) do { if (!(cond)) return -(int)hipErrorInvalidValue; } while (0)

// the launch itself and everything behind it: the launcher's own error first, then what the stream reports
inline int finish(hipError_t launched)
{
    const hipError_t sync = hipDeviceSynchronize();
    if (launched != hipSuccess) { (void)hipGetLastError(); return (int)launched; }
    return sync == hipSuccess ? 0 : -(int)sync;
}

// plan9: passes, bits[4], shift[4]
inline PostPlan plan_of(const uint32_t* plan9)
{
    PostPlan p{};
    p.passes = plan9[0];
    for (uint32_t k = 0; k < kPostMaxPasses; k++) { p.bits[k] = plan9[1 + k]; p.shift[k] = plan9[1 + kPostMaxPasses + k]; }
    return p;
}

// a pass the launchers run: then the arrays must hold what the kernels index
inline bool runs(const PostPlan& p, uint32_t pass, uint64_t n)
{
    return n != 0 && n < kPostMaxSpans && pass < p.passes && pass < kPostMaxPasses && p.bits[pass] != 0 && p.bits[pass] <= kPostMaxDigitBits;
}

#ifdef AM_BOUNDS_CHECK
hipError_t (*g_bounds_reader)(uint32_t* out2) = nullptr;    // reads the assertion words of THIS library's copy of the kernels (am_bounds.h)
#endif

}  // namespace

#ifdef AM_BOUNDS_CHECK
// libam.so keeps its own list (am_abi.cpp) and does not export it: the copy of am_postings.hip in here registers with this one
namespace am { namespace dev { void bounds_register(const char*, hipError_t (*read)(uint32_t* out2)) { g_bounds_reader = read; } } }
#endif

// out2: the index assertions (am_bounds.h) that failed in this library's kernels so far and the line of the first; zeros in a build without them
AMPC_API int ampc_bounds(uint32_t* out2)
{
    out2[0] = out2[1] = 0;
#ifdef AM_BOUNDS_CHECK
    if (g_bounds_reader) AMPC_TRY(g_bounds_reader(out2));
#endif
    return 0;
}

AMPC_API uint64_t ampc_guard_items() { return kGuard; }

// out5: spans per tile, spans per wavefront portion, lanes per workgroup of the sort, lanes per workgroup of the row kernels, the first span count refused
AMPC_API void ampc_limits(uint64_t* out5)
{
    out5[0] = kPostTileSpans;
    out5[1] = kPostWaveSpans;
    out5[2] = kPostThreads;
    out5[3] = kRowThreads;
    out5[4] = kPostMaxSpans;
}

// post_plan(n_needles) as plan9
AMPC_API void ampc_plan(uint64_t n_needles, uint32_t* plan9)
{
    const PostPlan p = post_plan(n_needles);
    plan9[0] = p.passes;
    for (uint32_t k = 0; k < kPostMaxPasses; k++) { plan9[1 + k] = p.bits[k]; plan9[1 + kPostMaxPasses + k] = p.shift[k]; }
}

// spans: n_buf rows of 24 bytes; keys, idx: n_buf elements and the guard
AMPC_API int ampc_keys(const void* spans, uint64_t n, uint64_t n_buf, uint32_t* keys, uint32_t* idx)
{
    AMPC_REQUIRE(n <= n_buf || n >= kPostMaxSpans);
    Buf d_spans(n_buf * sizeof(Span)), d_keys((n_buf + kGuard) * 4), d_idx((n_buf + kGuard) * 4);
    AMPC_TRY(d_spans.err); AMPC_TRY(d_keys.err); AMPC_TRY(d_idx.err);
    AMPC_TRY(up(d_spans, spans, n_buf * sizeof(Span)));
    AMPC_TRY(up(d_keys, keys, (n_buf + kGuard) * 4));
    AMPC_TRY(up(d_idx, idx, (n_buf + kGuard) * 4));
    const int rc = finish(launch_post_keys((const Span*)d_spans.p, n, (uint32_t*)d_keys.p, (uint32_t*)d_idx.p, nullptr));
    AMPC_TRY(down(keys, d_keys, (n_buf + kGuard) * 4));
    AMPC_TRY(down(idx, d_idx, (n_buf + kGuard) * 4));
    return rc;
}

// keys: n_buf elements; counts: cells elements and the guard
AMPC_API int ampc_hist(const uint32_t* plan9, uint32_t pass, const uint32_t* keys, uint64_t n, uint64_t n_buf, uint32_t* counts, uint64_t cells)
{
    const PostPlan plan = plan_of(plan9);
    if (runs(plan, pass, n)) AMPC_REQUIRE(n <= n_buf && (uint64_t)post_digits(plan, pass) * post_tiles(n) <= cells);
    Buf d_keys(n_buf * 4), d_counts((cells + kGuard) * 4);
    AMPC_TRY(d_keys.err); AMPC_TRY(d_counts.err);
    AMPC_TRY(up(d_keys, keys, n_buf * 4));
    AMPC_TRY(up(d_counts, counts, (cells + kGuard) * 4));
    const int rc = finish(launch_post_hist(plan, pass, (const uint32_t*)d_keys.p, n, (uint32_t*)d_counts.p, nullptr));
    AMPC_TRY(down(counts, d_counts, (cells + kGuard) * 4));
    return rc;
}

// keys_in, idx_in: n_buf elements; base: cells elements; keys_out, idx_out: n_buf elements and the guard
AMPC_API int ampc_scatter(const uint32_t* plan9, uint32_t pass, const uint32_t* keys_in, const uint32_t* idx_in, uint64_t n, uint64_t n_buf, const uint64_t* base,
                          uint64_t cells, uint32_t* keys_out, uint32_t* idx_out)
{
    const PostPlan plan = plan_of(plan9);
    if (runs(plan, pass, n)) AMPC_REQUIRE(n <= n_buf && (uint64_t)post_digits(plan, pass) * post_tiles(n) <= cells);
    Buf d_kin(n_buf * 4), d_iin(n_buf * 4), d_base(cells * 8), d_kout((n_buf + kGuard) * 4), d_iout((n_buf + kGuard) * 4);
    AMPC_TRY(d_kin.err); AMPC_TRY(d_iin.err); AMPC_TRY(d_base.err); AMPC_TRY(d_kout.err); AMPC_TRY(d_iout.err);
    AMPC_TRY(up(d_kin, keys_in, n_buf * 4));
    AMPC_TRY(up(d_iin, idx_in, n_buf * 4));
    AMPC_TRY(up(d_base, base, cells * 8));
    AMPC_TRY(up(d_kout, keys_out, (n_buf + kGuard) * 4));
    AMPC_TRY(up(d_iout, idx_out, (n_buf + kGuard) * 4));
    const int rc = finish(launch_post_scatter(plan, pass, (const uint32_t*)d_kin.p, (const uint32_t*)d_iin.p, n, (const uint64_t*)d_base.p, (uint32_t*)d_kout.p,
                                              (uint32_t*)d_iout.p, nullptr));
    AMPC_TRY(down(keys_out, d_kout, (n_buf + kGuard) * 4));
    AMPC_TRY(down(idx_out, d_iout, (n_buf + kGuard) * 4));
    return rc;
}

// spans: n_buf rows; idx: n_buf elements; data: n_buf rows and the guard (in rows); source: n_buf elements and the guard
AMPC_API int ampc_gather(const void* spans, const uint32_t* idx, uint64_t n, uint64_t n_buf, void* data, uint64_t* source)
{
    AMPC_REQUIRE(n <= n_buf || n >= kPostMaxSpans);
    Buf d_spans(n_buf * sizeof(Span)), d_idx(n_buf * 4), d_data((n_buf + kGuard) * sizeof(Span)), d_source((n_buf + kGuard) * 8);
    AMPC_TRY(d_spans.err); AMPC_TRY(d_idx.err); AMPC_TRY(d_data.err); AMPC_TRY(d_source.err);
    AMPC_TRY(up(d_spans, spans, n_buf * sizeof(Span)));
    AMPC_TRY(up(d_idx, idx, n_buf * 4));
    AMPC_TRY(up(d_data, data, (n_buf + kGuard) * sizeof(Span)));
    AMPC_TRY(up(d_source, source, (n_buf + kGuard) * 8));
    const int rc = finish(launch_post_gather((const Span*)d_spans.p, (const uint32_t*)d_idx.p, n, (Span*)d_data.p, (uint64_t*)d_source.p, nullptr));
    AMPC_TRY(down(data, d_data, (n_buf + kGuard) * sizeof(Span)));
    AMPC_TRY(down(source, d_source, (n_buf + kGuard) * 8));
    return rc;
}

// keys: n elements, ascending; offsets: n_needles + 1 elements and the guard
AMPC_API int ampc_offsets(const uint32_t* keys, uint64_t n, uint64_t n_needles, uint64_t* offsets)
{
    AMPC_REQUIRE(n_needles < (1ull << 28));
    Buf d_keys(n * 4), d_off((n_needles + 1 + kGuard) * 8);
    AMPC_TRY(d_keys.err); AMPC_TRY(d_off.err);
    AMPC_TRY(up(d_keys, keys, n * 4));
    AMPC_TRY(up(d_off, offsets, (n_needles + 1 + kGuard) * 8));
    const int rc = finish(launch_post_offsets((const uint32_t*)d_keys.p, n, n_needles, (uint64_t*)d_off.p, nullptr));
    AMPC_TRY(down(offsets, d_off, (n_needles + 1 + kGuard) * 8));
    return rc;
}

// data: n_buf rows; keys: n_buf elements; doc_freq: n_needles elements and the guard, ADDED to
AMPC_API int ampc_df(const void* data, const uint32_t* keys, uint64_t n, uint64_t n_buf, uint64_t n_needles, uint64_t* doc_freq)
{
    AMPC_REQUIRE((n <= n_buf || n >= kPostMaxSpans) && n_needles < (1ull << 28));
    Buf d_data(n_buf * sizeof(Span)), d_keys(n_buf * 4), d_df((n_needles + kGuard) * 8);
    AMPC_TRY(d_data.err); AMPC_TRY(d_keys.err); AMPC_TRY(d_df.err);
    AMPC_TRY(up(d_data, data, n_buf * sizeof(Span)));
    AMPC_TRY(up(d_keys, keys, n_buf * 4));
    AMPC_TRY(up(d_df, doc_freq, (n_needles + kGuard) * 8));
    const int rc = finish(launch_post_df((const Span*)d_data.p, (const uint32_t*)d_keys.p, n, n_needles, (uint64_t*)d_df.p, nullptr));
    AMPC_TRY(down(doc_freq, d_df, (n_needles + kGuard) * 8));
    return rc;
}

// row: n_row rows, haystacks ascending; out_off: n_hay + 1 elements and the guard
AMPC_API int ampc_row_offsets(const void* row, uint64_t n_row, uint64_t n_hay, uint64_t* out_off)
{
    AMPC_REQUIRE(n_hay < (1ull << 28));
    Buf d_row(n_row * sizeof(Span)), d_off((n_hay + 1 + kGuard) * 8);
    AMPC_TRY(d_row.err); AMPC_TRY(d_off.err);
    AMPC_TRY(up(d_row, row, n_row * sizeof(Span)));
    AMPC_TRY(up(d_off, out_off, (n_hay + 1 + kGuard) * 8));
    const int rc = finish(launch_post_row_offsets((const Span*)d_row.p, n_row, n_hay, (uint64_t*)d_off.p, nullptr));
    AMPC_TRY(down(out_off, d_off, (n_hay + 1 + kGuard) * 8));
    return rc;
}
