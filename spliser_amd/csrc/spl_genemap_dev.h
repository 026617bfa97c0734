// spl_genemap_dev.h -- what the four counting kernels of spl_genecount.hip and spl_exoncount.hip share; device code only.
//
// A MAP (a gene map of spl_genecount_rule.h; a bin map of spl_exoncount_rule.h has the same shape) as a workgroup has it: the top
// level -- every stride-th start -- in LDS, the entries in global memory (DevMap).
//
// THE FRAME of a counting kernel (CountFrame): both maps' top levels go into LDS and the special counters' sums are cleared; a
// grid-stride loop gives every lane of the workgroup a read of the segment per step, or none; a kernel's own per-step body says
// what a read comes to and commits it wave by wave, gathering the special counters in `mine` (lane c of a wave: the wave's reads
// that add to special counter c); the frame ends as the predicate tally does (spl_tally_dev.h: tally_finish), behind the kernel's
// n_codes ordinary counters.
#ifndef SPL_GENEMAP_DEV_H
#define SPL_GENEMAP_DEV_H
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "spl_genecount.h" // spl_count_maps
#include "spl_genecount_rule.h"
#include "spl_strand_rule.h"
#include "spl_tally_dev.h" // tally_finish: the frame's ending
#include "spl_wave.h"

namespace {

struct DevMap {
    const int32_t *top; // LDS
    uint32_t n_top, stride;
    int64_t n;
    const int32_t *start;
    const uint32_t *code;
    __device__ __forceinline__ int64_t size() const { return n; }
    __device__ __forceinline__ int64_t find(int64_t pos) const
    {
        const int64_t j = spl_cover_find(top, 0, n_top, pos);
        if (j < 0) return -1;
        const int64_t lo = j * stride, hi = lo + stride < n ? lo + stride : n;
        return spl_cover_find(start, lo, hi, pos); // (start[lo] <= pos: the answer is lo at least)
    }
    __device__ __forceinline__ int64_t start_at(int64_t k) const { return (int64_t)start[k]; }
    __device__ __forceinline__ uint32_t code_at(int64_t k) const { return code[k]; }
};

// The frame.  TILE: the workgroup's lanes (whole waves); TOP: a map's top level at most; SPECIALS: the special counters.  A kernel
// makes one (all lanes: it ends in a barrier), runs its per-step body in the frame's loop -- for ALL lanes of the workgroup, also
// those past the segment's end: the wave-wide commits want whole waves, and the loop's bound is uniform over the workgroup -- and
// calls finish() (all lanes again).
template <uint32_t TILE, uint32_t TOP, uint32_t SPECIALS>
struct CountFrame {
    static_assert(TILE % 64 == 0, "whole waves: the wave-wide commits are called by all 64 lanes");
    DevMap map_a, map_b;
    uint32_t *s_sum; // LDS
    uint32_t mine;   // lane c of a wave: the wave's reads that add to special counter c

    __device__ __forceinline__ CountFrame(const spl_count_maps &m)
    {
        __shared__ int32_t s_top[2 * TOP];
        __shared__ uint32_t sums[SPECIALS];
        const uint32_t t = threadIdx.x;
        for (uint32_t j = t; j < m.a.top; j += TILE) s_top[j] = m.a.start[(int64_t)j * m.a.stride];
        for (uint32_t j = t; j < m.b.top; j += TILE) s_top[TOP + j] = m.b.start[(int64_t)j * m.b.stride];
        if (t < SPECIALS) sums[t] = 0u;
        __syncthreads();
        map_a = DevMap{s_top, m.a.top, m.a.stride, m.a.n, m.a.start, m.a.code};
        map_b = DevMap{s_top + TOP, m.b.top, m.b.stride, m.b.n, m.b.start, m.b.code};
        s_sum = sums;
        mine = 0u;
    }
    // the grid-stride loop: for (int64_t base = f.first(); base < n; base += f.stride()) -- read r = base + threadIdx.x, if r < n
    __device__ __forceinline__ int64_t first() const { return (int64_t)blockIdx.x * TILE; }
    __device__ __forceinline__ int64_t stride() const { return (int64_t)gridDim.x * TILE; }
    // the special counters behind the kernel's n_codes ordinary ones
    __device__ __forceinline__ void finish(uint32_t n_codes, unsigned long long *counts)
    {
        tally_finish<SPECIALS>(s_sum, mine, counts + n_codes, SlotSame{});
    }
};

// The two levels of a map of n entries whose top level has at most `top` of them.
inline void levels(int64_t n, uint32_t top, uint32_t *stride, uint32_t *n_top)
{
    *stride = n ? (uint32_t)((n + top - 1) / top) : 1u;
    *n_top = n ? (uint32_t)((n + *stride - 1) / *stride) : 0u;
}

// A launcher's check of what every counting launch takes, and -- where it passes -- *out: the maps with their levels, as the kernel
// takes them.  n_codes: the genes or the bins.
inline bool count_launch_fits(const spl_devreads *src, int64_t n_rec, int64_t first, int64_t n, int stranded, const spl_count_maps *maps, uint32_t n_codes, const unsigned long long *counts,
                              uint32_t top, spl_count_maps *out)
{
    if (!src || !counts || !maps || first < 0 || first + n > n_rec || stranded < 0 || stranded > 2 || n_codes > SPL_GENE_INDEX_MAX) return false;
    *out = *maps;
    for (spl_count_map *m : {&out->a, &out->b}) {
        if (m->n < 0 || (m->n && (!m->start || !m->code))) return false;
        levels(m->n, top, &m->stride, &m->top);
    }
    return true;
}

} // namespace
#endif
