// spl_exoncount.hip -- per-exon-bin read counts over the BAM-native arrays of a fused read set (spl_exon_count: the `exoncounts`
// command).  The per-read rule is spl_exoncount_rule.h, which the host compiles too; the commit is spl_exoncount_wave.h, which the
// wave emulator runs.  gfx950.
//
// Replaces a second pass over the file this library has just decoded by `featureCounts -f -O` or `dexseq_count.py`: reads per exon
// counting bin for edgeR::diffSpliceDGE / DEXSeq, beside the change in splice-site strength.  The reference has no counterpart.
//
// The geometry is spl_genecount.hip's: one launch per segment of the set, a grid-stride loop over its reads, SPL_EXON_TILE reads a
// workgroup and step, a read a lane, in whatever order the reads are; both bin maps' top levels in LDS (8 KB), the rest searched
// in global memory (spl_genemap_dev.h).  The shape is not: a read adds to several bins, and to none of them before its verdict is
// known -- an ambiguous read adds to no bin.  A lane walks its read TWICE: the first walk (spl_exon_verdict) gives the verdict, the
// second (spl_exon_hits again, for counted reads only) gives the bins one by one to splexon::wave_commit, which takes a bin a lane
// a round and makes one 64-bit add per run of equal bins in the wave.  Nothing is stored per lane: a read has any number of bins.
// The four verdict counters are ballots and popcounts per wave and step, the waves' sums meeting in LDS and a workgroup ending
// with one atomic per counter.  Integer sums: exact, whatever the order.
//
// spl_exon_count_fragments (`exoncounts --countReadPairs`) is a kernel of its own below, in the same geometry over the segment's
// mate table: a fragment's leader walks both mates, and its bins are the merge of the two walks (spl_exonfragment_rule.h).
#include <hip/hip_runtime.h>
#include <stdint.h>

#define SPL_HD __device__ __forceinline__
#include "spl_exoncount.h"
#include "spl_exoncount_rule.h"
#include "spl_exoncount_wave.h"
#include "spl_exonfragment_rule.h" // a fragment's rule: spl_exon_count_fragments_kernel
#include "spl_genemap_dev.h"       // DevMap, DevOps, levels

static_assert(splexon::VERDICTS == SPL_EXON_VERDICTS && splexon::IDLE_VERDICT == SPL_EXON_IDLE && SPL_EXON_COUNTED == 0u && SPL_EXON_NO_FEATURE == 1u && SPL_EXON_AMBIGUOUS == 2u &&
                  SPL_EXON_NOT_COUNTED == 3u,
              "the rule's verdicts are the commit's counters");
static_assert(SPL_EXON_NO_BIN == splexon::NO_BIN, "the merge's ended walk is the commit's lane without a bin");
static_assert(SPL_EXON_TILE % 64 == 0, "whole waves: splexon::wave_commit is called by all 64 lanes");

namespace {

// A lane's bins for splexon::wave_commit: the second walk of a counted read; a lane without one has no op to walk.
struct LaneBins {
    spl_exon_hits<DevOps, DevMap> hits;
    __device__ __forceinline__ uint32_t next() { return spl_exon_next_bin(hits, splexon::NO_BIN); }
};

__global__ __launch_bounds__(SPL_EXON_TILE) void spl_exon_count_kernel(const spl_devreads src, int64_t n_ops_total, int64_t first, int64_t n, int32_t shift, int stranded, int64_t n_a,
                                                                        const int32_t *a_start, const uint32_t *a_code, uint32_t a_stride, uint32_t a_top, int64_t n_b,
                                                                        const int32_t *b_start, const uint32_t *b_code, uint32_t b_stride, uint32_t b_top, uint32_t n_bins,
                                                                        const uint32_t *bin_gene, unsigned long long *counts)
{
    __shared__ int32_t s_top[2 * SPL_EXON_TOP];
    __shared__ uint32_t s_sum[SPL_EXON_VERDICTS];
    const uint32_t t = threadIdx.x;
    const uint32_t lane = wv::lane();
    for (uint32_t j = t; j < a_top; j += SPL_EXON_TILE) s_top[j] = a_start[(int64_t)j * a_stride];
    for (uint32_t j = t; j < b_top; j += SPL_EXON_TILE) s_top[SPL_EXON_TOP + j] = b_start[(int64_t)j * b_stride];
    if (t < SPL_EXON_VERDICTS) s_sum[t] = 0u;
    __syncthreads();
    const DevMap map_a{s_top, a_top, a_stride, n_a, a_start, a_code}, map_b{s_top + SPL_EXON_TOP, b_top, b_stride, n_b, b_start, b_code};
    uint32_t mine = 0; // lane c of a wave: the wave's reads of verdict c (at most 64 a step: 32 bits hold any read set's)
    for (int64_t base = (int64_t)blockIdx.x * SPL_EXON_TILE; base < n; base += (int64_t)gridDim.x * SPL_EXON_TILE) { // (uniform over the workgroup)
        const int64_t r = base + t;
        uint32_t verdict = SPL_EXON_IDLE, c0 = 0u, n_ops = 0u;
        int64_t p = 0;
        DevMap map = map_a;
        if (r < n) {
            const int64_t i = first + r;
            const uint32_t flag = src.flag[i];
            const int64_t pos = (int64_t)src.pos[i];
            c0 = src.cig_off[i];
            uint32_t c1 = src.cig_off[i + 1];
            if (c1 < c0 || (int64_t)c1 > n_ops_total) c1 = c0; // (offsets of the arrays' own ops: said for the memory's sake)
            verdict = SPL_EXON_NOT_COUNTED;
            if (spl_gene_eligible(flag, pos, c1 - c0)) {
                n_ops = c1 - c0;
                p = pos - 1 + (int64_t)shift;
                if (spl_gene_uses_b(flag, stranded)) map = map_b;
                verdict = spl_exon_verdict(DevOps{src.cigar + c0}, n_ops, p, map, bin_gene);
            }
        }
        splexon::wave_verdicts(verdict, mine);
        LaneBins bins{spl_exon_hits<DevOps, DevMap>(DevOps{src.cigar + c0}, verdict == SPL_EXON_COUNTED ? n_ops : 0u, p, map)};
        splexon::wave_commit(bins, n_bins, reinterpret_cast<uint64_t *>(counts));
    }
    if (lane < SPL_EXON_VERDICTS && mine) atomicAdd(&s_sum[lane], mine);
    __syncthreads();
    if (t < SPL_EXON_VERDICTS && s_sum[t]) atomicAdd(&counts[(int64_t)n_bins + t], (unsigned long long)s_sum[t]);
}

// Fragments (spl_exon_count_fragments): the same launch over the segment with its mate table (spl_mates.hip) beside the arrays.  A
// lane whose read leads a fragment walks its own ops and its mate's, wherever that read lies in the segment, first for the verdict
// over both (spl_exon_fragment_verdict), then -- a counted fragment only -- as the merge of the two walks (spl_exon_merge), which
// gives splexon::wave_commit every distinct bin once, in ascending order, with nothing stored per lane.  The mate's lane stays
// silent: SPL_EXON_IDLE and no bin.  The rule is spl_exonfragment_rule.h.
// Two walks a lane are 135 vector registers when the compiler is left alone: three waves a SIMD, three workgroups a CU, and the
// fourth quarter of a launch of SPL_EXON_GRID_MAX workgroups (four a CU) waits for a second round.  The bound of four waves a SIMD
// keeps all of them resident (128 registers, DESIGN section 7: what it costs in scratch, and what it gains).
struct LaneFragmentBins {
    spl_exon_merge<DevOps, DevMap> merge;
    __device__ __forceinline__ uint32_t next() { return merge.next(); }
};

__global__ __launch_bounds__(SPL_EXON_TILE, 4) void spl_exon_count_fragments_kernel(const spl_devreads src, int64_t n_ops_total, int64_t first, int64_t n, int32_t shift, int stranded, int64_t n_a,
                                                                                  const int32_t *a_start, const uint32_t *a_code, uint32_t a_stride, uint32_t a_top, int64_t n_b,
                                                                                  const int32_t *b_start, const uint32_t *b_code, uint32_t b_stride, uint32_t b_top, uint32_t n_bins,
                                                                                  const uint32_t *bin_gene, const uint32_t *mate, unsigned long long *counts)
{
    __shared__ int32_t s_top[2 * SPL_EXON_TOP];
    __shared__ uint32_t s_sum[SPL_EXON_VERDICTS];
    const uint32_t t = threadIdx.x;
    const uint32_t lane = wv::lane();
    for (uint32_t j = t; j < a_top; j += SPL_EXON_TILE) s_top[j] = a_start[(int64_t)j * a_stride];
    for (uint32_t j = t; j < b_top; j += SPL_EXON_TILE) s_top[SPL_EXON_TOP + j] = b_start[(int64_t)j * b_stride];
    if (t < SPL_EXON_VERDICTS) s_sum[t] = 0u;
    __syncthreads();
    const DevMap map_a{s_top, a_top, a_stride, n_a, a_start, a_code}, map_b{s_top + SPL_EXON_TOP, b_top, b_stride, n_b, b_start, b_code};
    const spl_mate_reads reads{src.pos, src.flag, src.cig_off, src.cigar, n_ops_total};
    uint32_t mine = 0; // (as in the per-read kernel)
    for (int64_t base = (int64_t)blockIdx.x * SPL_EXON_TILE; base < n; base += (int64_t)gridDim.x * SPL_EXON_TILE) { // (uniform over the workgroup)
        const int64_t r = base + t;
        uint32_t verdict = SPL_EXON_IDLE;
        spl_exon_side lead{0u, 0u, 0, false}, other{0u, 0u, 0, false};
        if (r < n) {
            verdict = spl_exon_fragment_sides(reads, first, n, r, mate, (int64_t)shift, stranded, &lead, &other);
            if (verdict == SPL_EXON_COUNTED) verdict = spl_exon_fragment_verdict<DevOps>(src.cigar, lead, other, map_a, map_b, bin_gene);
        }
        splexon::wave_verdicts(verdict, mine);
        if (verdict != SPL_EXON_COUNTED) lead.n_ops = other.n_ops = 0u; // (no walk: the merge has no bin)
        LaneFragmentBins bins{spl_exon_merge<DevOps, DevMap>(src.cigar, lead, other, map_a, map_b)};
        splexon::wave_commit(bins, n_bins, reinterpret_cast<uint64_t *>(counts));
    }
    if (lane < SPL_EXON_VERDICTS && mine) atomicAdd(&s_sum[lane], mine);
    __syncthreads();
    if (t < SPL_EXON_VERDICTS && s_sum[t]) atomicAdd(&counts[(int64_t)n_bins + t], (unsigned long long)s_sum[t]);
}

} // namespace

extern "C" uint32_t spl_dev_exon_grid(int64_t n)
{
    const int64_t g = (n + SPL_EXON_TILE - 1) / SPL_EXON_TILE;
    return (uint32_t)(g < 1 ? 1 : g > SPL_EXON_GRID_MAX ? SPL_EXON_GRID_MAX : g);
}

extern "C" int spl_dev_launch_exon_count(const spl_devreads *src, int64_t n_rec, int64_t n_ops, int64_t first, int64_t n, int32_t shift, int stranded, int64_t n_a, const int32_t *a_start,
                                         const uint32_t *a_code, int64_t n_b, const int32_t *b_start, const uint32_t *b_code, uint32_t n_bins, const uint32_t *bin_gene,
                                         unsigned long long *counts, void *stream)
{
    if (n <= 0) return 0;
    if (!src || !counts || first < 0 || first + n > n_rec || stranded < 0 || stranded > 2 || n_bins > SPL_GENE_INDEX_MAX || (n_bins && !bin_gene) || n_a < 0 ||
        (n_a && (!a_start || !a_code)) || n_b < 0 || (n_b && (!b_start || !b_code)))
        return (int)hipErrorInvalidValue;
    uint32_t a_stride, a_top, b_stride, b_top;
    levels(n_a, SPL_EXON_TOP, &a_stride, &a_top);
    levels(n_b, SPL_EXON_TOP, &b_stride, &b_top);
    hipLaunchKernelGGL(spl_exon_count_kernel, dim3(spl_dev_exon_grid(n)), dim3(SPL_EXON_TILE), 0, (hipStream_t)stream, *src, n_ops, first, n, shift, stranded, n_a, a_start, a_code, a_stride,
                       a_top, n_b, b_start, b_code, b_stride, b_top, n_bins, bin_gene, counts);
    return (int)hipGetLastError();
}

extern "C" int spl_dev_launch_exon_count_fragments(const spl_devreads *src, int64_t n_rec, int64_t n_ops, int64_t first, int64_t n, int32_t shift, int stranded, int64_t n_a,
                                                   const int32_t *a_start, const uint32_t *a_code, int64_t n_b, const int32_t *b_start, const uint32_t *b_code, uint32_t n_bins,
                                                   const uint32_t *bin_gene, const uint32_t *mate, unsigned long long *counts, void *stream)
{
    if (n <= 0) return 0;
    if (!src || !counts || !mate || first < 0 || first + n > n_rec || stranded < 0 || stranded > 2 || n_bins > SPL_GENE_INDEX_MAX || (n_bins && !bin_gene) || n_a < 0 ||
        (n_a && (!a_start || !a_code)) || n_b < 0 || (n_b && (!b_start || !b_code)))
        return (int)hipErrorInvalidValue;
    uint32_t a_stride, a_top, b_stride, b_top;
    levels(n_a, SPL_EXON_TOP, &a_stride, &a_top);
    levels(n_b, SPL_EXON_TOP, &b_stride, &b_top);
    hipLaunchKernelGGL(spl_exon_count_fragments_kernel, dim3(spl_dev_exon_grid(n)), dim3(SPL_EXON_TILE), 0, (hipStream_t)stream, *src, n_ops, first, n, shift, stranded, n_a, a_start, a_code,
                       a_stride, a_top, n_b, b_start, b_code, b_stride, b_top, n_bins, bin_gene, mate, counts);
    return (int)hipGetLastError();
}
