// spl_tally_dev.h -- the predicate tally of the per-read kernels (spl_coverage.hip, spl_strand.hip, and the ending of
// spl_genemap_dev.h's CountFrame); device code only.  Every counter is a 0/1 predicate of a read, a read a lane: a ballot and a
// popcount per wave and step, lane c of a wave keeping the wave's share of counter c (at most 64 a step: 32 bits hold any read
// set's); the waves' shares meet in LDS, and the workgroup ends with one 64-bit atomic per counter that is not zero.  Integer sums.
#ifndef SPL_TALLY_DEV_H
#define SPL_TALLY_DEV_H
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "spl_wave.h"

namespace {

struct SlotSame {
    __device__ __forceinline__ uint32_t operator()(uint32_t c) const { return c; }
};

// The ending, by all lanes of the workgroup.  mine: lane c of every wave holds the wave's share of counter c; s_sum: N words of
// LDS, cleared before a barrier; counter c is added to out[slot(c)].
template <uint32_t N, class Slot>
__device__ __forceinline__ void tally_finish(uint32_t *s_sum, uint32_t mine, unsigned long long *out, const Slot &slot)
{
    const uint32_t t = threadIdx.x;
    if (wv::lane() < N && mine) atomicAdd(&s_sum[wv::lane()], mine);
    __syncthreads();
    if (t < N && s_sum[t]) atomicAdd(&out[slot(t)], (unsigned long long)s_sum[t]);
}

// N counters.  A kernel makes one (it ends in a barrier, which also serves what the kernel put into LDS before), calls add() once
// per step and finish() once -- all three by ALL lanes of the workgroup from uniform control flow, a lane without a read adding 0.
template <uint32_t N>
struct PredicateTally {
    static_assert(N <= 64, "lane c keeps counter c");
    uint32_t *s_sum; // LDS
    uint32_t mine;

    __device__ __forceinline__ PredicateTally() : mine(0u)
    {
        __shared__ uint32_t sums[N];
        if (threadIdx.x < N) sums[threadIdx.x] = 0u;
        __syncthreads();
        s_sum = sums;
    }
    __device__ __forceinline__ void add(uint32_t bits) // bit c: this lane's read adds to counter c
    {
#pragma unroll
        for (uint32_t c = 0; c < N; ++c) {
            const uint64_t b = wv::ballot((bits >> c) & 1u);
            if (wv::lane() == c) mine += wv::popc64(b);
        }
    }
    template <class Slot = SlotSame>
    __device__ __forceinline__ void finish(unsigned long long *out, const Slot &slot = Slot{}) { tally_finish<N>(s_sum, mine, out, slot); }
};

// A 64-bit sum of the lanes' own values (the coverage's covered bases): summed across the wave, one atomic a wave that has any.
__device__ __forceinline__ void wave_add64(unsigned long long *out, unsigned long long v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    if (wv::lane() == 0u && v) atomicAdd(out, v);
}

} // namespace
#endif
