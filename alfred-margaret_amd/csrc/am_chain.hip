// am_chain.hip -- the kernels of the chain selector (am_chain.h): one lane per element around chain_walk, chain_next and chain_double, for the Splitter's records
// and the spans' candidates.  Plain C++ and vector stores only.
#include "am_chain.h"

AM_BOUNDS_TU("am_chain.hip")

namespace am {
namespace dev {

namespace {

template <class View>
__global__ void __launch_bounds__(kRowThreads) k_chain_walk(View v, const uint8_t* __restrict__ head, uint32_t* __restrict__ kept, uint32_t limit, uint32_t* __restrict__ long_chains)
{
    const uint64_t i = global_row();
    if (i >= v.n || !head[i]) return;
    if (chain_walk(v, head, kept, limit, i)) *long_chains = 1;
}

template <class View>
__global__ void __launch_bounds__(kRowThreads) k_chain_next(View v, const uint8_t* __restrict__ head, uint64_t* __restrict__ jump)
{
    const uint64_t i = global_row();
    if (i >= v.n) return;
    jump[i] = chain_next(v, head, i);
}

__global__ void __launch_bounds__(kRowThreads) k_chain_double(const uint64_t* __restrict__ jump_in, uint64_t* __restrict__ jump_out, uint64_t n, uint32_t* __restrict__ kept,
                                                              uint32_t* __restrict__ marked)
{
    const uint64_t i = global_row();
    if (i >= n) return;
    if (chain_double(jump_in, jump_out, n, kept, i)) *marked = 1;
}

}  // namespace

template <class View>
hipError_t launch_chain_walk(const View& v, const uint8_t* head, uint32_t* kept, uint32_t limit, uint32_t* long_chains, hipStream_t st)
{
    return launch_rows(k_chain_walk<View>, v.n, st, v, head, kept, limit, long_chains);
}

template <class View>
hipError_t launch_chain_next(const View& v, const uint8_t* head, uint64_t* jump, hipStream_t st)
{
    return launch_rows(k_chain_next<View>, v.n, st, v, head, jump);
}

hipError_t launch_chain_double(const uint64_t* jump_in, uint64_t* jump_out, uint64_t n, uint32_t* kept, uint32_t* marked, hipStream_t st)
{
    return launch_rows(k_chain_double, n, st, jump_in, jump_out, n, kept, marked);
}

template hipError_t launch_chain_walk(const SplitChain&, const uint8_t*, uint32_t*, uint32_t, uint32_t*, hipStream_t);
template hipError_t launch_chain_walk(const SpansChain&, const uint8_t*, uint32_t*, uint32_t, uint32_t*, hipStream_t);
template hipError_t launch_chain_next(const SplitChain&, const uint8_t*, uint64_t*, hipStream_t);
template hipError_t launch_chain_next(const SpansChain&, const uint8_t*, uint64_t*, hipStream_t);

}  // namespace dev
}  // namespace am
