// spl_exoncount.hip -- per-exon-bin read counts over the BAM-native arrays of a fused read set (spl_exon_count: the `exoncounts`
// command).  The per-read rule is spl_exoncount_rule.h, which the host compiles too; the commit is spl_exoncount_wave.h, which the
// wave emulator runs.  gfx950.
//
// Replaces a second pass over the file this library has just decoded by `featureCounts -f -O` or `dexseq_count.py`: reads per exon
// counting bin for edgeR::diffSpliceDGE / DEXSeq, beside the change in splice-site strength.  The reference has no counterpart.
//
// The geometry is spl_genecount.hip's, the frame of spl_genemap_dev.h (CountFrame) with SPL_EXON_TILE reads a workgroup and step
// and both bin maps' top levels in LDS (8 KB); both kernels here are its loop with a per-step body of their own.  The shape is not: a read adds to
// several bins, and to none of them before its verdict is known -- an ambiguous read adds to no bin.  A lane walks its read TWICE:
// the first walk (spl_exon_verdict) gives the verdict, the second (spl_exon_hits again, for counted reads only) gives the bins one
// by one to splexon::wave_commit, which takes a bin a lane a round and makes one 64-bit add per run of equal bins in the wave.
// Nothing is stored per lane: a read has any number of bins.  The four verdict counters are ballots and popcounts per wave and
// step (splexon::wave_verdicts); the frame sums them.
//
// spl_exon_count_fragments (`exoncounts --countReadPairs`) is the second kernel below, over the segment's mate table: a fragment's
// leader walks both mates, and its bins are the merge of the two walks (spl_exonfragment_rule.h).
#include <hip/hip_runtime.h>
#include <stdint.h>

#define SPL_HD __device__ __forceinline__
#include "spl_exoncount.h"
#include "spl_exoncount_rule.h"
#include "spl_exoncount_wave.h"
#include "spl_exonfragment_rule.h" // a fragment's rule: spl_exon_count_fragments_kernel
#include "spl_genemap_dev.h"       // DevMap, CountFrame, count_launch_fits

static_assert(splexon::VERDICTS == SPL_EXON_VERDICTS && splexon::IDLE_VERDICT == SPL_EXON_IDLE && SPL_EXON_COUNTED == 0u && SPL_EXON_NO_FEATURE == 1u && SPL_EXON_AMBIGUOUS == 2u &&
                  SPL_EXON_NOT_COUNTED == 3u,
              "the rule's verdicts are the commit's counters");
static_assert(SPL_EXON_NO_BIN == splexon::NO_BIN, "the merge's ended walk is the commit's lane without a bin");

namespace {

// A lane's bins for splexon::wave_commit: the second walk of a counted read; a lane without one has no op to walk.
struct LaneBins {
    spl_exon_hits<spl_ops_ptr, DevMap> hits;
    __device__ __forceinline__ uint32_t next() { return spl_exon_next_bin(hits, splexon::NO_BIN); }
};

__global__ __launch_bounds__(SPL_EXON_TILE) void spl_exon_count_kernel(const spl_devreads src, int64_t n_ops_total, int64_t first, int64_t n, int32_t shift, int stranded,
                                                                        const spl_count_maps maps, uint32_t n_bins, const uint32_t *bin_gene, unsigned long long *counts)
{
    CountFrame<SPL_EXON_TILE, SPL_EXON_TOP, SPL_EXON_VERDICTS> f(maps);
    for (int64_t base = f.first(); base < n; base += f.stride()) { // (uniform over the workgroup)
        const int64_t r = base + threadIdx.x;
        uint32_t verdict = SPL_EXON_IDLE, c0 = 0u, n_ops = 0u;
        int64_t p = 0;
        DevMap map = f.map_a;
        if (r < n) {
            const int64_t i = first + r;
            const uint32_t flag = src.flag[i];
            const int64_t pos = (int64_t)src.pos[i];
            uint32_t its_ops;
            spl_ops_of(src.cig_off, i, n_ops_total, &c0, &its_ops);
            verdict = SPL_EXON_NOT_COUNTED;
            if (spl_gene_eligible(flag, pos, its_ops)) {
                n_ops = its_ops; // (a read that is not eligible is not walked)
                p = pos - 1 + (int64_t)shift;
                if (spl_gene_uses_b(flag, stranded)) map = f.map_b;
                verdict = spl_exon_verdict(spl_ops_ptr{src.cigar + c0}, n_ops, p, map, bin_gene);
            }
        }
        splexon::wave_verdicts(verdict, f.mine);
        LaneBins bins{spl_exon_hits<spl_ops_ptr, DevMap>(spl_ops_ptr{src.cigar + c0}, verdict == SPL_EXON_COUNTED ? n_ops : 0u, p, map)};
        splexon::wave_commit(bins, n_bins, reinterpret_cast<uint64_t *>(counts));
    }
    f.finish(n_bins, counts);
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
    spl_exon_merge<spl_ops_ptr, DevMap> merge;
    __device__ __forceinline__ uint32_t next() { return merge.next(); }
};

__global__ __launch_bounds__(SPL_EXON_TILE, 4) void spl_exon_count_fragments_kernel(const spl_devreads src, int64_t n_ops_total, int64_t first, int64_t n, int32_t shift, int stranded,
                                                                                  const spl_count_maps maps, uint32_t n_bins, const uint32_t *bin_gene, const uint32_t *mate,
                                                                                  unsigned long long *counts)
{
    const spl_read_view reads{src.pos, src.flag, src.cig_off, src.cigar, n_ops_total};
    CountFrame<SPL_EXON_TILE, SPL_EXON_TOP, SPL_EXON_VERDICTS> f(maps);
    for (int64_t base = f.first(); base < n; base += f.stride()) { // (uniform over the workgroup)
        const int64_t r = base + threadIdx.x;
        uint32_t verdict = SPL_EXON_IDLE;
        spl_exon_side lead{0u, 0u, 0, false}, other{0u, 0u, 0, false};
        if (r < n) {
            verdict = spl_exon_fragment_sides(reads, first, n, r, mate, (int64_t)shift, stranded, &lead, &other);
            if (verdict == SPL_EXON_COUNTED) verdict = spl_exon_fragment_verdict<spl_ops_ptr>(src.cigar, lead, other, f.map_a, f.map_b, bin_gene);
        }
        splexon::wave_verdicts(verdict, f.mine);
        if (verdict != SPL_EXON_COUNTED) lead.n_ops = other.n_ops = 0u; // (no walk: the merge has no bin)
        LaneFragmentBins bins{spl_exon_merge<spl_ops_ptr, DevMap>(src.cigar, lead, other, f.map_a, f.map_b)};
        splexon::wave_commit(bins, n_bins, reinterpret_cast<uint64_t *>(counts));
    }
    f.finish(n_bins, counts);
}

} // namespace

extern "C" uint32_t spl_dev_exon_grid(int64_t n)
{
    const int64_t g = (n + SPL_EXON_TILE - 1) / SPL_EXON_TILE;
    return (uint32_t)(g < 1 ? 1 : g > SPL_EXON_GRID_MAX ? SPL_EXON_GRID_MAX : g);
}

extern "C" int spl_dev_launch_exon_count(const spl_devreads *src, int64_t n_rec, int64_t n_ops, int64_t first, int64_t n, int32_t shift, int stranded, const spl_count_maps *maps,
                                         uint32_t n_bins, const uint32_t *bin_gene, unsigned long long *counts, void *stream)
{
    if (n <= 0) return 0;
    spl_count_maps m;
    if ((n_bins && !bin_gene) || !count_launch_fits(src, n_rec, first, n, stranded, maps, n_bins, counts, SPL_EXON_TOP, &m)) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(spl_exon_count_kernel, dim3(spl_dev_exon_grid(n)), dim3(SPL_EXON_TILE), 0, (hipStream_t)stream, *src, n_ops, first, n, shift, stranded, m, n_bins, bin_gene, counts);
    return (int)hipGetLastError();
}

extern "C" int spl_dev_launch_exon_count_fragments(const spl_devreads *src, int64_t n_rec, int64_t n_ops, int64_t first, int64_t n, int32_t shift, int stranded, const spl_count_maps *maps,
                                                   uint32_t n_bins, const uint32_t *bin_gene, const uint32_t *mate, unsigned long long *counts, void *stream)
{
    if (n <= 0) return 0;
    spl_count_maps m;
    if (!mate || (n_bins && !bin_gene) || !count_launch_fits(src, n_rec, first, n, stranded, maps, n_bins, counts, SPL_EXON_TOP, &m)) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(spl_exon_count_fragments_kernel, dim3(spl_dev_exon_grid(n)), dim3(SPL_EXON_TILE), 0, (hipStream_t)stream, *src, n_ops, first, n, shift, stranded, m, n_bins, bin_gene,
                       mate, counts);
    return (int)hipGetLastError();
}
