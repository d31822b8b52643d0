// am_coords.hip -- match coordinates on the device (include/am.h "coordinates"): the tile pass behind the index and the four consumers.  The class masks and the lookup
// are am_coords.h's, shared with the CPU test program; the prefix sums between the tile pass and the consumers are am_scan.hip's launch_scan, one per class.
//
// k_coords_tiles reads the text once in aligned 16-byte groups, one group per lane and load (64 lanes: 1 KiB per instruction, four loads in flight per lane); the
// eight lanes of a tile add their counts up with three shuffles and the first of them writes the tile's uint32 counts.  It knows nothing about haystacks.
// k_coords_spans / _fragments / _ranges / _positions take one lane per row and call the lookup: a prefix entry and at most eight group loads of the position's own
// tile per class and position.  The rows of a haystack ascend, so neighbouring lanes read the same tiles.  No kernel talks to another workgroup; all positions are
// 64-bit; plain C++ and vector stores only.
#include <hip/hip_runtime.h>

#include "am_bounds.h"
#include "am_coords.h"

AM_BOUNDS_TU("am_coords.hip")

namespace am {
namespace dev {

namespace {

constexpr uint32_t kCoThreads = 256;                        // lanes of a k_coords_tiles workgroup
constexpr uint32_t kCoLoads = 4;                            // groups per lane of the tile pass
constexpr uint32_t kCoGroupsPerTile = kCoordsTile / kCoordsGroup;

// a workgroup takes kCoThreads * kCoLoads consecutive groups (128 tiles); n_groups = ceil(total / 16): every group read ends at or before round_up(total, 16)
__global__ void __launch_bounds__(kCoThreads) k_coords_tiles(const uint8_t* __restrict__ text, uint64_t total, uint64_t n_groups, uint32_t* __restrict__ c_start,
                                                             uint32_t* __restrict__ c_four, uint32_t* __restrict__ c_newline)
{
    const uint64_t g0 = (uint64_t)blockIdx.x * (kCoThreads * kCoLoads) + threadIdx.x;
    CoordsWords v[kCoLoads];
#pragma unroll
    for (uint32_t k = 0; k < kCoLoads; k++) {
        const uint64_t gi = g0 + (uint64_t)k * kCoThreads;
        v[k] = gi < n_groups ? coords_load(text, gi * kCoordsGroup) : CoordsWords{0, 0, 0, 0};
    }
#pragma unroll
    for (uint32_t k = 0; k < kCoLoads; k++) {
        const uint64_t gi = g0 + (uint64_t)k * kCoThreads, q = gi * kCoordsGroup;
        uint32_t packed = 0;                                // three counts of at most 16 each, at most 128 per tile: a byte each
        if (gi < n_groups) {
            if (c_start) packed |= coords_group_count<kCoordsStart>(v[k], q, total);
            if (c_four) packed |= coords_group_count<kCoordsFour>(v[k], q, total) << 8;
            if (c_newline) packed |= coords_group_count<kCoordsNewline>(v[k], q, total) << 16;
        }
        packed += __shfl_xor(packed, 1);
        packed += __shfl_xor(packed, 2);
        packed += __shfl_xor(packed, 4);
        if ((threadIdx.x & (kCoGroupsPerTile - 1)) == 0 && gi < n_groups) {      // (gi is a multiple of 8 here: the first group of tile gi / 8)
            const uint64_t t = gi / kCoGroupsPerTile;
            if (c_start) c_start[t] = packed & 0xFFu;
            if (c_four) c_four[t] = (packed >> 8) & 0xFFu;
            if (c_newline) c_newline[t] = (packed >> 16) & 0xFFu;
        }
    }
}

// the haystack of a row, or false: a row that does not lie inside its haystack (not reachable for a result made over this batch) reads no text
__device__ __forceinline__ bool row_in_haystack(const CoordsIn& in, uint32_t hay, uint64_t start, uint64_t len, uint64_t* base)
{
    AM_BOUNDS(hay < in.n_hay);
    if (hay >= in.n_hay) return false;
    const uint64_t b = in.offsets[hay], next = in.offsets[hay + 1];
    const bool ok = b <= next && next <= in.total && start <= next - b && len <= next - b - start;
    AM_BOUNDS(ok);
    *base = b;
    return ok;
}

// (U(start), U(start + len) - U(start)) of a row of the haystack at base
__device__ __forceinline__ void convert_row(const CoordsIn& in, int unit, uint64_t base, uint64_t start, uint64_t len, uint64_t* u_start, uint64_t* u_len)
{
    const uint64_t ub = coords_units(in, unit, base), us = coords_units(in, unit, base + start);
    const uint64_t ue = len ? coords_units(in, unit, base + start + len) : us;
    *u_start = us - ub;
    *u_len = ue - us;
}

__global__ void __launch_bounds__(kRowThreads) k_coords_spans(CoordsIn in, int unit, const Span* __restrict__ spans, uint64_t n, Span* __restrict__ out)
{
    const uint64_t i = global_row();
    if (i >= n) return;
    const Span sp = spans[i];
    Span o{0, 0, sp.haystack, sp.needle};
    uint64_t base;
    if (row_in_haystack(in, sp.haystack, sp.start, sp.len, &base)) convert_row(in, unit, base, sp.start, sp.len, &o.start, &o.len);
    out[i] = o;
}

// fragments carry no haystack: row i belongs to the last haystack whose offset is <= i (empty rows share an offset with the next one)
__global__ void __launch_bounds__(kRowThreads) k_coords_fragments(CoordsIn in, int unit, const Fragment* __restrict__ frags, const uint64_t* __restrict__ frag_off, uint64_t n,
                                                                 Fragment* __restrict__ out)
{
    const uint64_t i = global_row();
    if (i >= n) return;
    const Fragment f = frags[i];
    const uint32_t hay = (uint32_t)last_at_or_before(frag_off, (uint64_t)0, (uint64_t)in.n_hay - 1, i);      // (frag_off ascends and frag_off[0] = 0 <= i)
    Fragment o{0, 0};
    uint64_t base;
    if (row_in_haystack(in, hay, f.start, f.len, &base)) convert_row(in, unit, base, f.start, f.len, &o.start, &o.len);
    out[i] = o;
}

__global__ void __launch_bounds__(kRowThreads) k_coords_ranges(CoordsIn in, int unit, const Span* __restrict__ spans, uint64_t n, SpanRange* __restrict__ out)
{
    const uint64_t i = global_row();
    if (i >= n) return;
    const Span sp = spans[i];
    SpanRange o{0, 0, 0, 0};
    uint64_t base;
    if (row_in_haystack(in, sp.haystack, sp.start, sp.len, &base)) {
        const uint64_t n_base = coords_count<kCoordsNewline>(in.text, in.prefix[kCoordsNewline], base, in.padded);
        const CoordsLineCol s = coords_line_col(in, unit, base, n_base, base + sp.start, nullptr);
        const CoordsLineCol e = sp.len ? coords_line_col(in, unit, base, n_base, base + sp.start + sp.len, &s) : s;      // (one line: the line start is reused)
        o = SpanRange{s.line, s.col, e.line, e.col};
    }
    out[i] = o;
}

__global__ void __launch_bounds__(kRowThreads) k_coords_positions(CoordsIn in, int unit, const uint32_t* __restrict__ hay, const uint64_t* __restrict__ pos, uint64_t n,
                                                                 uint64_t* __restrict__ out, uint64_t* __restrict__ flag)
{
    const uint64_t i = global_row();
    if (i >= n) return;
    const uint32_t h = hay[i];
    const uint64_t p = pos[i];
    bool ok = h < in.n_hay;
    uint64_t base = 0;
    if (ok) {
        const uint64_t next = in.offsets[h + 1];
        base = in.offsets[h];
        ok = base <= next && next <= in.total && p <= next - base;
    }
    if (!ok) { *flag = 1; return; }                         // (every lane that raises it stores the same word)
    out[i] = coords_units(in, unit, base + p) - coords_units(in, unit, base);
}

}  // namespace

hipError_t launch_coords_tiles(const uint8_t* text, uint64_t total, uint32_t* const counts[kCoordsClasses], hipStream_t st)
{
    if (total == 0) return hipSuccess;
    const uint64_t n_groups = (total + kCoordsGroup - 1) / kCoordsGroup, per_block = (uint64_t)kCoThreads * kCoLoads;
    const uint64_t blocks = (n_groups + per_block - 1) / per_block;
    if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_coords_tiles, dim3((uint32_t)blocks), dim3(kCoThreads), 0, st, text, total, n_groups, counts[kCoordsStart], counts[kCoordsFour], counts[kCoordsNewline]);
    return hipGetLastError();
}

hipError_t launch_coords_spans(const CoordsIn& in, int unit, const Span* spans, uint64_t n, Span* out, hipStream_t st)
{
    return launch_rows(k_coords_spans, n, st, in, unit, spans, n, out);
}

hipError_t launch_coords_fragments(const CoordsIn& in, int unit, const Fragment* frags, const uint64_t* frag_off, uint64_t n, Fragment* out, hipStream_t st)
{
    return launch_rows(k_coords_fragments, n, st, in, unit, frags, frag_off, n, out);
}

hipError_t launch_coords_ranges(const CoordsIn& in, int unit, const Span* spans, uint64_t n, SpanRange* out, hipStream_t st)
{
    return launch_rows(k_coords_ranges, n, st, in, unit, spans, n, out);
}

hipError_t launch_coords_positions(const CoordsIn& in, int unit, const uint32_t* hay, const uint64_t* pos, uint64_t n, uint64_t* out, uint64_t* flag, hipStream_t st)
{
    return launch_rows(k_coords_positions, n, st, in, unit, hay, pos, n, out, flag);
}

}  // namespace dev
}  // namespace am
