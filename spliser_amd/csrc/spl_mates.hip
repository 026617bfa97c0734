// spl_mates.hip -- the mate table of one segment of a fused read set (spl_mate_table), from the reads' name keys.  The rule --
// who is pairable, the sort key, the pair stage's body -- is spl_mate_rule.h, which the host compiles too.  gfx950.
//
// Replaces the name-sorted pass in front of `htseq-count` / `featureCounts -p --countReadPairs`: which two records of a
// coordinate-sorted file are one fragment.  The reference has no counterpart.
//
// Three stages.  COMPACT: a read a lane marks itself pairable or not (spl_mate_mark_kernel), the marks become their prefix sums by
// spl_sort.hip's scan, and every pairable read writes (sort key, index) to the place its sum names (spl_mate_compact_kernel): the
// segment's order is kept.  SORT: eight stable passes of spl_dev_launch_sort_pass over the 64-bit keys, by the caller.  PAIR: an
// element a lane, three binary searches over the sorted keys and one store (spl_mate_pair_kernel); the two counters are a ballot
// and a popcount per wave and step, the waves' sums meeting in LDS and a workgroup ending with one atomic per counter.
// The geometry is spl_genecount.hip's: a grid-stride loop, SPL_MATE_TILE a workgroup and step, in whatever order the reads are.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#define SPL_HD __device__ __forceinline__
#include "spl_mate_rule.h"
#include "spl_mates.h"
#include "spl_wave.h"

static_assert(SPL_MATE_TILE % 64 == 0, "whole waves: the ballots are called by all 64 lanes");

namespace {

// -> whether read i of the arrays is pairable, and its flag and key for the caller
__device__ __forceinline__ bool pairable_at(const spl_devreads &src, const uint64_t *name_key, int64_t i, uint32_t *flag, uint64_t *key)
{
    *flag = src.flag[i];
    *key = name_key[i];
    const uint32_t c0 = src.cig_off[i], c1 = src.cig_off[i + 1];
    return spl_mate_pairable(*flag, (int64_t)src.pos[i], c1 > c0 ? c1 - c0 : 0u, *key);
}

__global__ __launch_bounds__(SPL_MATE_TILE) void spl_mate_mark_kernel(const spl_devreads src, const uint64_t *name_key, int64_t first, int64_t n, uint32_t *mark)
{
    for (int64_t r = (int64_t)blockIdx.x * SPL_MATE_TILE + threadIdx.x; r < n; r += (int64_t)gridDim.x * SPL_MATE_TILE) {
        uint32_t flag;
        uint64_t key;
        mark[r] = pairable_at(src, name_key, first + r, &flag, &key) ? 1u : 0u;
    }
}

__global__ __launch_bounds__(SPL_MATE_TILE) void spl_mate_compact_kernel(const spl_devreads src, const uint64_t *name_key, int64_t first, int64_t n, const uint32_t *scan, uint64_t *keys,
                                                                          uint32_t *index)
{
    for (int64_t r = (int64_t)blockIdx.x * SPL_MATE_TILE + threadIdx.x; r < n; r += (int64_t)gridDim.x * SPL_MATE_TILE) {
        const uint32_t here = scan[r], before = r ? scan[r - 1] : 0u;
        if (here == before) continue;
        uint32_t flag;
        uint64_t key;
        (void)pairable_at(src, name_key, first + r, &flag, &key);
        keys[before] = spl_mate_sort_key(key, flag); // (before < scan[n - 1], the elements the caller made room for)
        index[before] = (uint32_t)r;
    }
}

__global__ __launch_bounds__(SPL_MATE_TILE) void spl_mate_pair_kernel(const uint64_t *keys, const uint32_t *index, int64_t n_pairable, const uint16_t *flag, int64_t n, uint32_t *mate,
                                                                       unsigned long long *counters)
{
    __shared__ uint32_t s_sum[2];
    const uint32_t t = threadIdx.x;
    if (t < 2u) s_sum[t] = 0u;
    __syncthreads();
    uint32_t paired = 0, lonely = 0; // lane 0 of a wave: the wave's sums (at most 64 a step: 32 bits hold any segment's)
    for (int64_t base = (int64_t)blockIdx.x * SPL_MATE_TILE; base < n_pairable; base += (int64_t)gridDim.x * SPL_MATE_TILE) { // (uniform over the workgroup)
        const int64_t j = base + t;
        bool has = false, alone = false;
        if (j < n_pairable) {
            has = spl_mate_pair_element(keys, index, n_pairable, j, mate, n);
            const uint32_t me = index[j];
            alone = !has && (int64_t)me < n && !(flag[me] & 0x8u);
        }
        paired += wv::popc64(wv::ballot(has));
        lonely += wv::popc64(wv::ballot(alone));
    }
    if (wv::lane() == 0u) {
        if (paired) atomicAdd(&s_sum[0], paired);
        if (lonely) atomicAdd(&s_sum[1], lonely);
    }
    __syncthreads();
    if (t < 2u && s_sum[t]) atomicAdd(&counters[1 + t], (unsigned long long)s_sum[t]);
}

__global__ __launch_bounds__(SPL_MATE_TILE) void spl_gather_u64_kernel(const uint32_t *perm, uint64_t n, const uint64_t *in, uint64_t *out)
{
    for (uint64_t i = (uint64_t)blockIdx.x * SPL_MATE_TILE + threadIdx.x; i < n; i += (uint64_t)gridDim.x * SPL_MATE_TILE) {
        const uint32_t p = perm[i];
        out[i] = (uint64_t)p < n ? in[p] : 0ull; // (a permutation of [0, n): said for the memory's sake)
    }
}

} // namespace

extern "C" uint32_t spl_dev_mate_grid(int64_t n)
{
    const int64_t g = (n + SPL_MATE_TILE - 1) / SPL_MATE_TILE;
    return (uint32_t)(g < 1 ? 1 : g > SPL_MATE_GRID_MAX ? SPL_MATE_GRID_MAX : g);
}

extern "C" int spl_dev_launch_mate_mark(const spl_devreads *src, const uint64_t *name_key, int64_t n_rec, int64_t first, int64_t n, uint32_t *mark, void *stream)
{
    if (n <= 0) return 0;
    if (!src || !name_key || !mark || first < 0 || first + n > n_rec) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(spl_mate_mark_kernel, dim3(spl_dev_mate_grid(n)), dim3(SPL_MATE_TILE), 0, (hipStream_t)stream, *src, name_key, first, n, mark);
    return (int)hipGetLastError();
}

extern "C" int spl_dev_launch_mate_compact(const spl_devreads *src, const uint64_t *name_key, int64_t n_rec, int64_t first, int64_t n, const uint32_t *scan, uint64_t *keys,
                                           uint32_t *index, void *stream)
{
    if (n <= 0) return 0;
    if (!src || !name_key || !scan || !keys || !index || first < 0 || first + n > n_rec) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(spl_mate_compact_kernel, dim3(spl_dev_mate_grid(n)), dim3(SPL_MATE_TILE), 0, (hipStream_t)stream, *src, name_key, first, n, scan, keys, index);
    return (int)hipGetLastError();
}

extern "C" int spl_dev_launch_mate_pair(const uint64_t *keys, const uint32_t *index, int64_t n_pairable, const uint16_t *flag, int64_t n, uint32_t *mate, unsigned long long *counters,
                                        void *stream)
{
    if (n_pairable <= 0) return 0;
    if (!keys || !index || !flag || !mate || !counters || n_pairable > n) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(spl_mate_pair_kernel, dim3(spl_dev_mate_grid(n_pairable)), dim3(SPL_MATE_TILE), 0, (hipStream_t)stream, keys, index, n_pairable, flag, n, mate, counters);
    return (int)hipGetLastError();
}

extern "C" int spl_dev_launch_gather_u64(const uint32_t *perm, uint64_t n, const uint64_t *in, uint64_t *out, void *stream)
{
    if (n == 0) return 0;
    if (!perm || !in || !out || (const void *)in == (const void *)out) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(spl_gather_u64_kernel, dim3(spl_dev_mate_grid((int64_t)std::min<uint64_t>(n, (uint64_t)SPL_MATE_GRID_MAX * SPL_MATE_TILE))), dim3(SPL_MATE_TILE), 0,
                       (hipStream_t)stream, perm, n, in, out);
    return (int)hipGetLastError();
}
