// am_wave.h -- device helpers shared by the HIP kernels of libam (gfx950): lane id, DPP prefix sum and maximum, the 64-bit wave sums and maxima, uniform values,
// LDS by absolute address (wave64), and the backward code-point walk of the IgnoreCase folds (AM_HD: the plain g++ programs under tests/native run it too, so
// nothing but the walk is declared without __HIPCC__)
#pragma once
#include <stdint.h>

#include "am_rows.h"

namespace am {
namespace dev {

#if defined(__HIPCC__)
// ------------------------------------------------------------------ wave helpers (wave64)

__device__ __forceinline__ uint32_t lane_id() { return __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)); }

// inclusive prefix sum over the 64 lanes with DPP adds (no LDS round trips): Kogge-Stone inside each
// 16-lane row (row_shr 1,2,4,8), then row_bcast:15 into rows 1 and 3, row_bcast:31 into rows 2 and 3
__device__ __forceinline__ uint32_t wave_inclusive_sum(uint32_t x, uint32_t /*lane*/)
{
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x111, 0xf, 0xf, false);   // row_shr:1
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x112, 0xf, 0xf, false);   // row_shr:2
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x114, 0xf, 0xf, false);   // row_shr:4
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x118, 0xf, 0xf, false);   // row_shr:8
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x142, 0xa, 0xf, false);   // row_bcast:15 -> rows 1, 3
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x143, 0xc, 0xf, false);   // row_bcast:31 -> rows 2, 3
    return x;
}

// maximum over the 64 lanes with DPP (the shape of the prefix sum above: inside each row of 16, then across the rows); uniform result
__device__ __forceinline__ int32_t wave_max_i32(int32_t x)
{
    x = [&] { const int32_t o = __builtin_amdgcn_update_dpp(INT32_MIN, x, 0x111, 0xf, 0xf, false); return o > x ? o : x; }();      // row_shr:1
    x = [&] { const int32_t o = __builtin_amdgcn_update_dpp(INT32_MIN, x, 0x112, 0xf, 0xf, false); return o > x ? o : x; }();      // row_shr:2
    x = [&] { const int32_t o = __builtin_amdgcn_update_dpp(INT32_MIN, x, 0x114, 0xf, 0xf, false); return o > x ? o : x; }();      // row_shr:4
    x = [&] { const int32_t o = __builtin_amdgcn_update_dpp(INT32_MIN, x, 0x118, 0xf, 0xf, false); return o > x ? o : x; }();      // row_shr:8
    x = [&] { const int32_t o = __builtin_amdgcn_update_dpp(INT32_MIN, x, 0x142, 0xa, 0xf, false); return o > x ? o : x; }();      // row_bcast:15 -> rows 1, 3
    x = [&] { const int32_t o = __builtin_amdgcn_update_dpp(INT32_MIN, x, 0x143, 0xc, 0xf, false); return o > x ? o : x; }();      // row_bcast:31 -> rows 2, 3
    return __builtin_amdgcn_readlane(x, 63);
}

// the wave's total of an inclusive prefix sum = lane 63's value, as a scalar (v_readlane_b32): whatever is computed or decided from it stays on the scalar
// side -- an `if` on it is a scalar branch.  (__shfl(x, 63) is a ds_bpermute: an LDS round trip, and a result in a VGPR that turns every `if` on it into an
// exec-masked region.)
__device__ __forceinline__ uint32_t wave_last_lane(uint32_t x) { return (uint32_t)__builtin_amdgcn_readlane((int)x, 63); }
// the value of lane l, l uniform (the index of a ballot's bit), as a scalar
__device__ __forceinline__ uint32_t wave_read_lane(uint32_t x, int l) { return (uint32_t)__builtin_amdgcn_readlane((int)x, l); }
__device__ __forceinline__ uint64_t wave_read_lane(uint64_t x, int l) { return ((uint64_t)wave_read_lane((uint32_t)(x >> 32), l) << 32) | wave_read_lane((uint32_t)x, l); }

// (acc << 1) | (a == b) in two VOP2/VOPC instructions: the comparison's result goes in as the carry of acc + acc.  The compiler's own code for the C
// expression is v_cmp + v_cndmask (VOP3) + half a v_lshlrev / v_or3 per step, and no C form of the addition makes it use the carry (tried: acc + (acc +
// (a == b)) and __builtin_addc both come out as the above).
__device__ __forceinline__ uint32_t shift_in_eq(uint32_t acc, uint32_t a, uint32_t b)
{
    asm("v_cmp_eq_u32 vcc, %1, %2\n\tv_addc_co_u32 %0, vcc, %0, %0, vcc" : "+v"(acc) : "v"(a), "v"(b) : "vcc");
    return acc;
}

// a value that is the same in every lane, moved to scalar registers (the two v_readfirstlane also force any load that
// produces it to be waited for right here)
__device__ __forceinline__ uint64_t uniform_u64(uint64_t x)
{
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)x), hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(x >> 32));
    return ((uint64_t)hi << 32) | lo;
}

__device__ __forceinline__ uint32_t uniform_u32(uint32_t x) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)x); }

// A by-value kernel argument (a struct `offset` bytes into the kernel's argument segment) read again where the call stands: the segment is in the constant
// address space, so the fields the caller goes on to use arrive by s_load, and the empty asm hides the segment's address from the compiler at this point --
// it cannot take the loads back to the kernel's entry, where their results would occupy scalar registers for the whole kernel.
template <class T>
__device__ __forceinline__ T kernarg_reload(uint32_t offset)
{
    typedef const __attribute__((address_space(4))) char* kernarg_bytes;
    kernarg_bytes p = (kernarg_bytes)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(p));
    typedef const __attribute__((address_space(4))) T* kernarg_t;      // (typed: a copy of unknown alignment is made with vector loads, not with s_load)
    T out;
    __builtin_memcpy(&out, (kernarg_t)(p + offset), sizeof(T));
    return out;
}

__device__ __forceinline__ uint64_t wave_sum_u64(uint64_t x)
{
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) x += __shfl_down(x, d, 64);
    return x;   // valid in lane 0
}

// maximum / sum over the 64 lanes, in every lane (xor butterflies)
__device__ __forceinline__ int64_t wave_max_i64(int64_t v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { const int64_t o = __shfl_xor(v, d, 64); v = o > v ? o : v; }
    return v;
}
__device__ __forceinline__ int64_t wave_sum_i64(int64_t v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}
// inclusive prefix sum of 64-bit values over the 64 lanes
__device__ __forceinline__ uint64_t wave_inclusive_sum_u64(uint64_t x, uint32_t lane)
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const uint64_t y = __shfl_up(x, d, 64); if (lane >= (uint32_t)d) x += y; }
    return x;
}

// order LDS traffic between lanes of one wavefront (DS ops of a wave execute in issue order;
// this only stops the compiler from moving them)
__device__ __forceinline__ void wave_lds_fence()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// what the lanes of this wavefront wrote to GLOBAL memory is visible to its other lanes (one L1 per workgroup: a wait, no cache control)
__device__ __forceinline__ void wave_global_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// LDS by absolute byte address.  k_sf declares no static LDS, so its dynamic LDS starts at address 0; reading through an
// address-space-3 pointer made from an integer lets the compiler put constant parts into the instruction's offset field
// instead of adding the (relocatable, always zero) base of the extern array to every address (16 v_add per chunk).
typedef __attribute__((address_space(3))) uint32_t lds_u32_t;
typedef __attribute__((address_space(3))) uint16_t lds_u16_t;
typedef uint32_t u32x2_n __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4_n __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) u32x2_n lds_u32x2_t;
typedef __attribute__((address_space(3))) u32x4_n lds_u32x4_t;
__device__ __forceinline__ uint32_t lds_read_u32(uint32_t byte_addr) { return *reinterpret_cast<const lds_u32_t*>((uintptr_t)byte_addr); }
__device__ __forceinline__ uint32_t lds_read_u16(uint32_t byte_addr) { return *reinterpret_cast<const lds_u16_t*>((uintptr_t)byte_addr); }
__device__ __forceinline__ void lds_write_u16(uint32_t byte_addr, uint32_t v) { *reinterpret_cast<lds_u16_t*>((uintptr_t)byte_addr) = (uint16_t)v; }
__device__ __forceinline__ void lds_write_u32x2(uint32_t byte_addr, uint2 v) { u32x2_n t; t.x = v.x; t.y = v.y; *reinterpret_cast<lds_u32x2_t*>((uintptr_t)byte_addr) = t; }
__device__ __forceinline__ void lds_write_u32x4(uint32_t byte_addr, uint4 v) { u32x4_n t; t.x = v.x; t.y = v.y; t.z = v.z; t.w = v.w; *reinterpret_cast<lds_u32x4_t*>((uintptr_t)byte_addr) = t; }

#endif  // __HIPCC__

// ------------------------------------------------------------------ UTF-8
// Utf8.hs:256-276 skipCodePointsBackwards hay (end_pos - 1) n: the index of the first byte of the code point n code points before the one whose last byte is
// hay[end_pos - 1].  The start of an IgnoreCase match of cps code points that ends at end_pos is n = cps - 1 (Splitter.hs:117-121, Replacer.hs:268-274).  Reads at
// most 4 bytes per code point, all of them in hay[0, end_pos): the caller has checked that these lie in its text.  A walk that would leave the haystack answers 0.
// The text is whatever byte_at(position) reads -- plain bytes, or a piece list behind a cursor (am_rp_fold.h): positions only ever fall.  Pos: uint64_t, or uint32_t
// where the caller's positions are below 2^31 (k_rp_lds).
template <class Pos, class ByteAt>
AM_HD Pos skip_code_points_backwards_by(ByteAt&& byte_at, Pos end_pos, uint32_t n)
{
    int64_t i = (int64_t)end_pos - 1;
    for (;;) {
        while (i > 0 && (byte_at((Pos)i) & 0xC0u) == 0x80u) i--;      // atTrailingByte (byte 0 is where the walk ends whatever it holds: not read)
        if (n == 0 || i <= 0) return (Pos)(i < 0 ? 0 : i);             // (the reference calls `error` where the walk leaves the text: not reachable for a match the automaton reported)
        i--; n--;
    }
}
AM_HD uint64_t skip_code_points_backwards(const uint8_t* hay, uint64_t end_pos, uint32_t n)
{
    return skip_code_points_backwards_by([hay](uint64_t i) -> uint32_t { return hay[i]; }, end_pos, n);
}

}  // namespace dev
}  // namespace am
