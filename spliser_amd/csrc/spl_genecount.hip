// spl_genecount.hip -- per-gene read counts over the BAM-native arrays of a fused read set (spl_gene_count: the `genecounts`
// command).  The per-read rule is spl_genecount_rule.h, which the host compiles too; the histogram is spl_genecount_wave.h, which
// the wave emulator runs.  gfx950.
//
// Replaces a second pass over the file this library has just decoded by `htseq-count` (--mode union --nonunique none) or
// `featureCounts`: the gene's expression beside a change in SSE, for the edgeR session of the diffSpliSER analysis.  The reference
// has no counterpart.
//
// The geometry is spl_strand.hip's: one launch per segment of the set, a grid-stride loop over its reads, SPL_GENE_TILE reads a
// workgroup and step, a read a lane, in whatever order the reads are.  A lane walks its eligible read's ops where they lie
// (spl_cov_walk) and folds every block over the gene map of its strand.  A map is searched in two steps: its top level -- every
// stride-th start, at most SPL_GENE_TOP of them -- is in LDS (both maps': 8 KB), the stretch of `stride` entries below the hit is
// searched where it is, in global memory; the stretches a block runs over behind the hit are read in turn.  A map of any size
// takes this path.
//
// The lane's result -- a gene, no feature, ambiguous, not counted -- goes into the counts by splgene::wave_count: one 64-bit
// atomic per RUN of equal gene results in a wave, and for the three special counters a ballot and a popcount per wave and step, the
// waves' sums meeting in LDS and a workgroup ending with one atomic per special counter.  Integer sums: exact, whatever the order.
#include <hip/hip_runtime.h>
#include <stdint.h>

#define SPL_HD __device__ __forceinline__
#include "spl_genecount.h"
#include "spl_genecount_rule.h"
#include "spl_genecount_wave.h"
#include "spl_genemap_dev.h" // DevMap, DevOps, levels
#include "spl_mate_rule.h"   // the fragment's rule

static_assert(splgene::NO_FEATURE == SPL_GENE_NO_FEATURE && splgene::AMBIGUOUS == SPL_GENE_AMBIGUOUS && splgene::NOT_COUNTED == SPL_GENE_NOT_COUNTED &&
                  splgene::IDLE == SPL_GENE_IDLE && splgene::SPECIALS == SPL_GENE_SPECIALS,
              "the rule's results are the histogram's");
static_assert(SPL_GENE_TILE % 64 == 0, "whole waves: splgene::wave_count is called by all 64 lanes");

namespace {

__global__ __launch_bounds__(SPL_GENE_TILE) void spl_gene_count_kernel(const spl_devreads src, int64_t n_ops_total, int64_t first, int64_t n, int32_t shift, int stranded, int64_t n_a,
                                                                        const int32_t *a_start, const uint32_t *a_code, uint32_t a_stride, uint32_t a_top, int64_t n_b,
                                                                        const int32_t *b_start, const uint32_t *b_code, uint32_t b_stride, uint32_t b_top, uint32_t n_genes,
                                                                        unsigned long long *counts)
{
    __shared__ int32_t s_top[2 * SPL_GENE_TOP];
    __shared__ uint32_t s_sum[SPL_GENE_SPECIALS];
    const uint32_t t = threadIdx.x;
    const uint32_t lane = wv::lane();
    for (uint32_t j = t; j < a_top; j += SPL_GENE_TILE) s_top[j] = a_start[(int64_t)j * a_stride];
    for (uint32_t j = t; j < b_top; j += SPL_GENE_TILE) s_top[SPL_GENE_TOP + j] = b_start[(int64_t)j * b_stride];
    if (t < SPL_GENE_SPECIALS) s_sum[t] = 0u;
    __syncthreads();
    const DevMap map_a{s_top, a_top, a_stride, n_a, a_start, a_code}, map_b{s_top + SPL_GENE_TOP, b_top, b_stride, n_b, b_start, b_code};
    uint32_t mine = 0; // lane c of a wave: the wave's reads that add to special counter c (at most 64 a step: 32 bits hold any read set's)
    for (int64_t base = (int64_t)blockIdx.x * SPL_GENE_TILE; base < n; base += (int64_t)gridDim.x * SPL_GENE_TILE) { // (uniform over the workgroup)
        const int64_t r = base + t;
        uint32_t result = SPL_GENE_IDLE;
        if (r < n) {
            const int64_t i = first + r;
            const uint32_t flag = src.flag[i];
            const int64_t pos = (int64_t)src.pos[i];
            uint32_t c0 = src.cig_off[i], c1 = src.cig_off[i + 1];
            if (c1 < c0 || (int64_t)c1 > n_ops_total) c1 = c0; // (offsets of the arrays' own ops: said for the memory's sake)
            result = SPL_GENE_NOT_COUNTED;
            if (spl_gene_eligible(flag, pos, c1 - c0)) {
                const int64_t p = pos - 1 + (int64_t)shift;
                result = spl_gene_uses_b(flag, stranded) ? spl_gene_of_blocks(DevOps{src.cigar + c0}, c1 - c0, p, map_b) : spl_gene_of_blocks(DevOps{src.cigar + c0}, c1 - c0, p, map_a);
            }
        }
        splgene::wave_count(result, n_genes, reinterpret_cast<uint64_t *>(counts), mine);
    }
    if (lane < SPL_GENE_SPECIALS && mine) atomicAdd(&s_sum[lane], mine);
    __syncthreads();
    if (t < SPL_GENE_SPECIALS && s_sum[t]) atomicAdd(&counts[(int64_t)n_genes + t], (unsigned long long)s_sum[t]);
}

// Fragments (spl_gene_count_fragments): the same launch over the segment with its mate table (spl_mates.hip) beside the arrays.
// A lane whose read leads a fragment walks its own ops and then its mate's, wherever that read lies in the segment; the mate's lane
// stays silent (SPL_GENE_IDLE), so the histogram is the per-read kernel's.  The rule is spl_gene_fragment_result.
__global__ __launch_bounds__(SPL_GENE_TILE) void spl_gene_count_fragments_kernel(const spl_devreads src, int64_t n_ops_total, int64_t first, int64_t n, int32_t shift, int stranded, int64_t n_a,
                                                                                  const int32_t *a_start, const uint32_t *a_code, uint32_t a_stride, uint32_t a_top, int64_t n_b,
                                                                                  const int32_t *b_start, const uint32_t *b_code, uint32_t b_stride, uint32_t b_top, uint32_t n_genes,
                                                                                  const uint32_t *mate, unsigned long long *counts)
{
    __shared__ int32_t s_top[2 * SPL_GENE_TOP];
    __shared__ uint32_t s_sum[SPL_GENE_SPECIALS];
    const uint32_t t = threadIdx.x;
    const uint32_t lane = wv::lane();
    for (uint32_t j = t; j < a_top; j += SPL_GENE_TILE) s_top[j] = a_start[(int64_t)j * a_stride];
    for (uint32_t j = t; j < b_top; j += SPL_GENE_TILE) s_top[SPL_GENE_TOP + j] = b_start[(int64_t)j * b_stride];
    if (t < SPL_GENE_SPECIALS) s_sum[t] = 0u;
    __syncthreads();
    const DevMap map_a{s_top, a_top, a_stride, n_a, a_start, a_code}, map_b{s_top + SPL_GENE_TOP, b_top, b_stride, n_b, b_start, b_code};
    const spl_mate_reads reads{src.pos, src.flag, src.cig_off, src.cigar, n_ops_total};
    uint32_t mine = 0; // (as in the per-read kernel)
    for (int64_t base = (int64_t)blockIdx.x * SPL_GENE_TILE; base < n; base += (int64_t)gridDim.x * SPL_GENE_TILE) { // (uniform over the workgroup)
        const int64_t r = base + t;
        uint32_t result = SPL_GENE_IDLE;
        if (r < n) result = spl_gene_fragment_result<DevOps>(reads, first, n, r, mate, (int64_t)shift, stranded, map_a, map_b);
        splgene::wave_count(result, n_genes, reinterpret_cast<uint64_t *>(counts), mine);
    }
    if (lane < SPL_GENE_SPECIALS && mine) atomicAdd(&s_sum[lane], mine);
    __syncthreads();
    if (t < SPL_GENE_SPECIALS && s_sum[t]) atomicAdd(&counts[(int64_t)n_genes + t], (unsigned long long)s_sum[t]);
}

} // namespace

extern "C" uint32_t spl_dev_gene_grid(int64_t n)
{
    const int64_t g = (n + SPL_GENE_TILE - 1) / SPL_GENE_TILE;
    return (uint32_t)(g < 1 ? 1 : g > SPL_GENE_GRID_MAX ? SPL_GENE_GRID_MAX : g);
}

extern "C" int spl_dev_launch_gene_count(const spl_devreads *src, int64_t n_rec, int64_t n_ops, int64_t first, int64_t n, int32_t shift, int stranded, int64_t n_a, const int32_t *a_start,
                                         const uint32_t *a_code, int64_t n_b, const int32_t *b_start, const uint32_t *b_code, uint32_t n_genes, unsigned long long *counts, void *stream)
{
    if (n <= 0) return 0;
    if (!src || !counts || first < 0 || first + n > n_rec || stranded < 0 || stranded > 2 || n_genes > SPL_GENE_INDEX_MAX || n_a < 0 || (n_a && (!a_start || !a_code)) || n_b < 0 ||
        (n_b && (!b_start || !b_code)))
        return (int)hipErrorInvalidValue;
    uint32_t a_stride, a_top, b_stride, b_top;
    levels(n_a, SPL_GENE_TOP, &a_stride, &a_top);
    levels(n_b, SPL_GENE_TOP, &b_stride, &b_top);
    hipLaunchKernelGGL(spl_gene_count_kernel, dim3(spl_dev_gene_grid(n)), dim3(SPL_GENE_TILE), 0, (hipStream_t)stream, *src, n_ops, first, n, shift, stranded, n_a, a_start, a_code, a_stride,
                       a_top, n_b, b_start, b_code, b_stride, b_top, n_genes, counts);
    return (int)hipGetLastError();
}

extern "C" int spl_dev_launch_gene_count_fragments(const spl_devreads *src, int64_t n_rec, int64_t n_ops, int64_t first, int64_t n, int32_t shift, int stranded, int64_t n_a,
                                                   const int32_t *a_start, const uint32_t *a_code, int64_t n_b, const int32_t *b_start, const uint32_t *b_code, uint32_t n_genes,
                                                   const uint32_t *mate, unsigned long long *counts, void *stream)
{
    if (n <= 0) return 0;
    if (!src || !counts || !mate || first < 0 || first + n > n_rec || stranded < 0 || stranded > 2 || n_genes > SPL_GENE_INDEX_MAX || n_a < 0 || (n_a && (!a_start || !a_code)) || n_b < 0 ||
        (n_b && (!b_start || !b_code)))
        return (int)hipErrorInvalidValue;
    uint32_t a_stride, a_top, b_stride, b_top;
    levels(n_a, SPL_GENE_TOP, &a_stride, &a_top);
    levels(n_b, SPL_GENE_TOP, &b_stride, &b_top);
    hipLaunchKernelGGL(spl_gene_count_fragments_kernel, dim3(spl_dev_gene_grid(n)), dim3(SPL_GENE_TILE), 0, (hipStream_t)stream, *src, n_ops, first, n, shift, stranded, n_a, a_start, a_code,
                       a_stride, a_top, n_b, b_start, b_code, b_stride, b_top, n_genes, mate, counts);
    return (int)hipGetLastError();
}
