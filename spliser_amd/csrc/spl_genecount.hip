// spl_genecount.hip -- per-gene read counts over the BAM-native arrays of a fused read set (spl_gene_count: the `genecounts`
// command).  The per-read rule is spl_genecount_rule.h, which the host compiles too; the histogram is spl_genecount_wave.h, which
// the wave emulator runs.  gfx950.
//
// Replaces a second pass over the file this library has just decoded by `htseq-count` (--mode union --nonunique none) or
// `featureCounts`: the gene's expression beside a change in SSE, for the edgeR session of the diffSpliSER analysis.  The reference
// has no counterpart.
//
// The geometry is spl_strand.hip's: one launch per segment of the set, a grid-stride loop over its reads, SPL_GENE_TILE reads a
// workgroup and step, a read a lane, in whatever order the reads are: the frame of spl_genemap_dev.h (CountFrame), whose loop both
// kernels here run with a per-step body of their own.  A lane walks its eligible read's ops where they lie (the block walk) and
// folds every block over the gene map of its strand.  A map is searched in two steps: its top level -- every stride-th start, at
// most SPL_GENE_TOP of them -- is in LDS (both maps': 8 KB), the stretch of `stride` entries below the hit is searched where it is, in global
// memory; the stretches a block runs over behind the hit are read in turn.  A map of any size takes this path.
//
// The lane's result -- a gene, no feature, ambiguous, not counted -- goes into the counts by splgene::wave_count: one 64-bit
// atomic per RUN of equal gene results in a wave, and for the three special counters a ballot and a popcount per wave and step;
// the frame sums them.
#include <hip/hip_runtime.h>
#include <stdint.h>

#define SPL_HD __device__ __forceinline__
#include "spl_genecount.h"
#include "spl_genecount_rule.h"
#include "spl_genecount_wave.h"
#include "spl_genemap_dev.h" // DevMap, CountFrame, count_launch_fits
#include "spl_mate_rule.h"   // the fragment's rule

static_assert(splgene::NO_FEATURE == SPL_GENE_NO_FEATURE && splgene::AMBIGUOUS == SPL_GENE_AMBIGUOUS && splgene::NOT_COUNTED == SPL_GENE_NOT_COUNTED &&
                  splgene::IDLE == SPL_GENE_IDLE && splgene::SPECIALS == SPL_GENE_SPECIALS,
              "the rule's results are the histogram's");

namespace {

__global__ __launch_bounds__(SPL_GENE_TILE) void spl_gene_count_kernel(const spl_devreads src, int64_t n_ops_total, int64_t first, int64_t n, int32_t shift, int stranded,
                                                                        const spl_count_maps maps, uint32_t n_genes, unsigned long long *counts)
{
    CountFrame<SPL_GENE_TILE, SPL_GENE_TOP, SPL_GENE_SPECIALS> f(maps);
    for (int64_t base = f.first(); base < n; base += f.stride()) { // (uniform over the workgroup)
        const int64_t r = base + threadIdx.x;
        uint32_t result = SPL_GENE_IDLE;
        if (r < n) {
            const int64_t i = first + r;
            const uint32_t flag = src.flag[i];
            const int64_t pos = (int64_t)src.pos[i];
            uint32_t c0, n_ops;
            spl_ops_of(src.cig_off, i, n_ops_total, &c0, &n_ops);
            result = SPL_GENE_NOT_COUNTED;
            if (spl_gene_eligible(flag, pos, n_ops)) {
                const int64_t p = pos - 1 + (int64_t)shift;
                result = spl_gene_uses_b(flag, stranded) ? spl_gene_of_blocks(spl_ops_ptr{src.cigar + c0}, n_ops, p, f.map_b) : spl_gene_of_blocks(spl_ops_ptr{src.cigar + c0}, n_ops, p, f.map_a);
            }
        }
        splgene::wave_count(result, n_genes, reinterpret_cast<uint64_t *>(counts), f.mine);
    }
    f.finish(n_genes, counts);
}

// Fragments (spl_gene_count_fragments): the same launch over the segment with its mate table (spl_mates.hip) beside the arrays.
// A lane whose read leads a fragment walks its own ops and then its mate's, wherever that read lies in the segment; the mate's lane
// stays silent (SPL_GENE_IDLE), so the histogram is the per-read kernel's.  The rule is spl_gene_fragment_result.
__global__ __launch_bounds__(SPL_GENE_TILE) void spl_gene_count_fragments_kernel(const spl_devreads src, int64_t n_ops_total, int64_t first, int64_t n, int32_t shift, int stranded,
                                                                                  const spl_count_maps maps, uint32_t n_genes, const uint32_t *mate, unsigned long long *counts)
{
    const spl_read_view reads{src.pos, src.flag, src.cig_off, src.cigar, n_ops_total};
    CountFrame<SPL_GENE_TILE, SPL_GENE_TOP, SPL_GENE_SPECIALS> f(maps);
    for (int64_t base = f.first(); base < n; base += f.stride()) { // (uniform over the workgroup)
        const int64_t r = base + threadIdx.x;
        uint32_t result = SPL_GENE_IDLE;
        if (r < n) result = spl_gene_fragment_result<spl_ops_ptr>(reads, first, n, r, mate, (int64_t)shift, stranded, f.map_a, f.map_b);
        splgene::wave_count(result, n_genes, reinterpret_cast<uint64_t *>(counts), f.mine);
    }
    f.finish(n_genes, counts);
}

} // namespace

extern "C" uint32_t spl_dev_gene_grid(int64_t n)
{
    const int64_t g = (n + SPL_GENE_TILE - 1) / SPL_GENE_TILE;
    return (uint32_t)(g < 1 ? 1 : g > SPL_GENE_GRID_MAX ? SPL_GENE_GRID_MAX : g);
}

extern "C" int spl_dev_launch_gene_count(const spl_devreads *src, int64_t n_rec, int64_t n_ops, int64_t first, int64_t n, int32_t shift, int stranded, const spl_count_maps *maps,
                                         uint32_t n_genes, unsigned long long *counts, void *stream)
{
    if (n <= 0) return 0;
    spl_count_maps m;
    if (!count_launch_fits(src, n_rec, first, n, stranded, maps, n_genes, counts, SPL_GENE_TOP, &m)) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(spl_gene_count_kernel, dim3(spl_dev_gene_grid(n)), dim3(SPL_GENE_TILE), 0, (hipStream_t)stream, *src, n_ops, first, n, shift, stranded, m, n_genes, counts);
    return (int)hipGetLastError();
}

extern "C" int spl_dev_launch_gene_count_fragments(const spl_devreads *src, int64_t n_rec, int64_t n_ops, int64_t first, int64_t n, int32_t shift, int stranded, const spl_count_maps *maps,
                                                   uint32_t n_genes, const uint32_t *mate, unsigned long long *counts, void *stream)
{
    if (n <= 0) return 0;
    spl_count_maps m;
    if (!mate || !count_launch_fits(src, n_rec, first, n, stranded, maps, n_genes, counts, SPL_GENE_TOP, &m)) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(spl_gene_count_fragments_kernel, dim3(spl_dev_gene_grid(n)), dim3(SPL_GENE_TILE), 0, (hipStream_t)stream, *src, n_ops, first, n, shift, stranded, m, n_genes, mate,
                       counts);
    return (int)hipGetLastError();
}
