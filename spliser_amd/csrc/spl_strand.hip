// spl_strand.hip -- read strand against evidence strand, tallied over the BAM-native arrays of a fused read set (spl_strand_tally:
// the `strandedness` command and `-s auto`).  The per-read rule is spl_strand_rule.h, which the host compiles too.  gfx950.
//
// Replaces the IGV paragraph of the reference's README -- open the BAM, colour the reads by first-in-pair, compare them with a
// junction -- by which its user is to learn whether the library is unstranded, fr or rf.  The reference has no counterpart.
//
// One launch per segment of the set, a grid-stride loop over its reads, SPL_STRAND_TILE reads a workgroup and step, a read a lane,
// in whatever order the reads are: nothing here knows of chunks or of sorted positions.  A read's FLAG and strand byte are all
// the tag evidence needs; POS, the two CIGAR offsets and the ops are read only when there is a cover map, and the ops only for an
// eligible read that lies in a stretch of the map at all.  The map is searched in two steps: its top level -- every stride-th
// start, at most SPL_STRAND_TOP of them -- is in LDS, the stretch of `stride` entries below the hit is searched where it is, in
// global memory (one entry when the whole map fits the top level).  A map of any size takes this path; nothing is a limit.
//
// Every counter is a 0/1 predicate per read: the predicate tally of spl_tally_dev.h.
#include <hip/hip_runtime.h>
#include <stdint.h>

#define SPL_HD __device__ __forceinline__
#include "spl_read_view.h"
#include "spl_strand.h"
#include "spl_strand_rule.h"
#include "spl_tally_dev.h"

namespace {

template <bool XS, bool MAP>
__global__ __launch_bounds__(SPL_STRAND_TILE) void spl_strand_tally_kernel(const spl_devreads src, const uint8_t *xs, int64_t n_ops_total, int64_t first, int64_t n, int32_t shift,
                                                                           int64_t n_cover, const int32_t *cover_start, const uint8_t *cover_code, uint32_t stride, uint32_t n_top,
                                                                           unsigned long long *out)
{
    __shared__ int32_t s_top[MAP ? SPL_STRAND_TOP : 1];
    const uint32_t t = threadIdx.x;
    if (MAP)
        for (uint32_t j = t; j < n_top; j += SPL_STRAND_TILE) s_top[j] = cover_start[(int64_t)j * stride];
    PredicateTally<SPL_STRAND_COUNTERS> tally; // (its barrier: s_top is filled)
    for (int64_t base = (int64_t)blockIdx.x * SPL_STRAND_TILE; base < n; base += (int64_t)gridDim.x * SPL_STRAND_TILE) { // (uniform over the workgroup)
        const int64_t r = base + t;
        uint32_t bits = 0;
        if (r < n) {
            const int64_t i = first + r;
            const uint32_t flag = src.flag[i];
            const uint8_t tag = XS ? xs[i] : (uint8_t)0;
            uint8_t ann = 0;
            if (MAP && spl_strand_eligible(flag)) {
                const int64_t pos = (int64_t)src.pos[i] + shift;
                const int64_t j = spl_cover_find(s_top, 0, n_top, pos);
                if (j >= 0) {
                    const int64_t lo = j * stride, hi = lo + stride < n_cover ? lo + stride : n_cover;
                    const int64_t k = spl_cover_find(cover_start, lo, hi, pos); // (start[lo] <= pos: k >= lo)
                    uint32_t c0, n_ops;
                    spl_ops_of(src.cig_off, i, n_ops_total, &c0, &n_ops);
                    ann = spl_cover_evidence(k, n_cover, cover_start, cover_code, pos, spl_strand_ref_len(src.cigar + c0, n_ops));
                }
            }
            bits = spl_strand_bits(flag, tag, ann);
        }
        tally.add(bits);
    }
    tally.finish(out);
}

} // namespace

extern "C" uint32_t spl_dev_strand_grid(int64_t n)
{
    const int64_t g = (n + SPL_STRAND_TILE - 1) / SPL_STRAND_TILE;
    return (uint32_t)(g < 1 ? 1 : g > SPL_STRAND_GRID_MAX ? SPL_STRAND_GRID_MAX : g);
}

extern "C" int spl_dev_launch_strand_tally(const spl_devreads *src, const uint8_t *xs, int64_t n_rec, int64_t n_ops, int64_t first, int64_t n, int32_t shift, int64_t n_cover,
                                           const int32_t *cover_start, const uint8_t *cover_code, unsigned long long *out14, void *stream)
{
    if (n <= 0) return 0;
    if (!src || !out14 || first < 0 || first + n > n_rec || n_cover < 0 || (n_cover && (!cover_start || !cover_code))) return (int)hipErrorInvalidValue;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(spl_dev_strand_grid(n)), block(SPL_STRAND_TILE);
    const uint32_t stride = n_cover ? (uint32_t)((n_cover + SPL_STRAND_TOP - 1) / SPL_STRAND_TOP) : 1u;
    const uint32_t n_top = n_cover ? (uint32_t)((n_cover + stride - 1) / stride) : 0u;
    if (n_cover && xs)
        hipLaunchKernelGGL((spl_strand_tally_kernel<true, true>), grid, block, 0, st, *src, xs, n_ops, first, n, shift, n_cover, cover_start, cover_code, stride, n_top, out14);
    else if (n_cover)
        hipLaunchKernelGGL((spl_strand_tally_kernel<false, true>), grid, block, 0, st, *src, xs, n_ops, first, n, shift, n_cover, cover_start, cover_code, stride, n_top, out14);
    else if (xs)
        hipLaunchKernelGGL((spl_strand_tally_kernel<true, false>), grid, block, 0, st, *src, xs, n_ops, first, n, shift, n_cover, cover_start, cover_code, stride, n_top, out14);
    else
        return (int)hipErrorInvalidValue; // (nothing to tally: the caller has said so already)
    return (int)hipGetLastError();
}
