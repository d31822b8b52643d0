// am_cased.h -- the comparator of include/am.h "exact case": are the bytes [start, start + len) of the batch text the spelling that lies at `at` in the table's pool?
// One __host__ __device__ function, so that the CPU runs the very code the kernels run (tests/native/cased_compare_main.cpp).
// THE POOL holds every spelling at a multiple of kCasedGroup bytes, zero-filled to the next one: a group of a spelling is four aligned dwords.  THE TEXT side is
// unaligned, and the span may end on the last byte of its haystack or of the text.  As load_piece of am_subst.hip does, the comparator reads only the ALIGNED dwords
// that hold a byte of the span -- they lie inside round_up(start + len, 4) <= round_up(total, 16), the text's own padding --, shifts them into place and masks the
// bytes beyond the span's end: what a neighbouring haystack or the padding holds in the same dword never reaches the result.  A span that does not lie inside
// [lo, hi), the bounds of its haystack in the text, is unequal without a read.
// One group per step, out at the first group that differs: a natural-text span is about 5 bytes, one step; a 66 000-byte spelling is 4 125 steps of a single lane,
// reached only where the IgnoreCase scan has already matched all of them.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define AM_CASED_HD __host__ __device__ __forceinline__
#else
#define AM_CASED_HD inline
#endif

namespace am {

constexpr uint32_t kCasedGroup = 16;                        // bytes per step of the comparator; every spelling starts at a multiple of it in the pool
constexpr uint32_t kCasedPoolPad = 16;                      // zero bytes behind the last group of the pool (as the replacement pool of am_subst_table_create has them)

// where a spelling of `len` bytes ends in the pool, rounded up to the next spelling's start
constexpr uint64_t cased_padded(uint64_t len) { return (len + kCasedGroup - 1) & ~(uint64_t)(kCasedGroup - 1); }

// the aligned dword at byte d of p (d a multiple of 4).  PRECONDITION: p is 4-byte aligned and readable to round_up(total, 16) -- true of every text an am_batch
// holds: am_batch_upload and sub_batch (am_fold.h) place the text at a 16-byte boundary of their own allocation and pad it, and am_batch_from_device refuses a
// d_bytes that is not 16-byte aligned (am_abi.cpp) and documents the padding the caller owes (include/am.h); the pool is the table's own allocation
AM_CASED_HD uint32_t cased_dword(const uint8_t* p, uint64_t d)
{
    uint32_t w;
    __builtin_memcpy(&w, __builtin_assume_aligned(p + d, 4), 4);
    return w;
}

// bytes a .. a + 3 of the eight bytes lo, hi (a in 0 .. 3): v_alignbyte_b32
AM_CASED_HD uint32_t cased_align(uint32_t hi, uint32_t lo, uint32_t a)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_alignbyte(hi, lo, a);
#else
    return (uint32_t)(((((uint64_t)hi) << 32) | lo) >> (8 * a));
#endif
}

// the first n bytes of a dword (n <= 0: none, n >= 4: all)
AM_CASED_HD uint32_t cased_below(int64_t n) { return n <= 0 ? 0u : n >= 4 ? 0xFFFFFFFFu : (1u << (8 * (uint32_t)n)) - 1u; }

// text[start, start + len) == pool[at, at + len), for a span inside the haystack text[lo, hi).  at: a multiple of kCasedGroup; the pool is readable to
// at + cased_padded(len).  len == 0: equal.
AM_CASED_HD bool cased_equal(const uint8_t* text, uint64_t lo, uint64_t hi, uint64_t start, const uint8_t* pool, uint64_t at, uint64_t len)
{
    if (start < lo || start > hi || len > hi - start) return false;
    for (uint64_t g = 0; g < len; g += kCasedGroup) {
        const uint64_t t = start + g, left = len - g;                  // left >= 1: bytes of the span from this group on
        const uint32_t a = (uint32_t)(t & 3u);
        const uint64_t first = t - a, end = t + (left < kCasedGroup ? left : kCasedGroup);      // end <= hi: dword j is read only where it begins below `end`
        uint32_t w[5];
#pragma unroll
        for (uint32_t j = 0; j < 5; j++) w[j] = first + 4 * j < end ? cased_dword(text, first + 4 * j) : 0u;
        uint32_t diff = 0;
#pragma unroll
        for (uint32_t j = 0; j < 4; j++)
            diff |= (cased_align(w[j + 1], w[j], a) ^ cased_dword(pool, at + g + 4 * j)) & cased_below((int64_t)left - 4 * (int64_t)j);
        if (diff != 0) return false;
    }
    return true;
}

}  // namespace am
