// spl_genemap_dev.h -- a gene map (spl_genecount_rule.h; a bin map of spl_exoncount_rule.h has the same shape) as a workgroup has
// it: the top level -- every stride-th start -- in LDS, the entries in global memory.  Shared by spl_genecount.hip and
// spl_exoncount.hip; device code only.
#ifndef SPL_GENEMAP_DEV_H
#define SPL_GENEMAP_DEV_H
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "spl_strand_rule.h"

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

struct DevOps {
    const uint32_t *p;
    __device__ __forceinline__ uint32_t operator()(uint32_t k) const { return p[k]; }
};

// The two levels of a map of n entries whose top level has at most `top` of them.
inline void levels(int64_t n, uint32_t top, uint32_t *stride, uint32_t *n_top)
{
    *stride = n ? (uint32_t)((n + top - 1) / top) : 1u;
    *n_top = n ? (uint32_t)((n + *stride - 1) / *stride) : 0u;
}

} // namespace
#endif
