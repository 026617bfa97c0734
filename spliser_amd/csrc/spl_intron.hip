// spl_intron.hip -- the trimmed depth of annotated introns (spl_intron_depth: the `intronretention` command) over the boundaries of
// the per-base depth that the coverage stages leave on the device.  The rule is spl_intron_rule.h; a team's body is
// spl_intron_wave.h, which the wave emulator runs.  gfx950.
//
// Replaces IRFinder / iREAD over the file this library has just decoded.  The reference has no counterpart.
//
// An intron costs its boundaries, not its bases: binary searches give each measurable piece its stretches of equal depth, and a
// weighted radix selection over (depth, bases) finds the two rank values of the trimmed range (spl_intron_wave.h).  One kernel,
// two geometries: an ordinary intron is taken by a workgroup of ONE wave, grid-stride over the list of such introns; an intron of
// SPL_INTRON_LONG_BASES measurable bases or more -- it may hold 10^5 boundaries -- by a workgroup of SPL_INTRON_TEAM lanes that
// share the histogram, so that it does not hold one wave while everything else has long ended.  The host sorts the introns
// into the two lists by their bases, which bound their boundaries.  An intron's four results are written by one lane: no
// atomics to device memory.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "spl_intron.h"
#include "spl_intron_wave.h"

static_assert(SPL_INTRON_TEAM % 64 == 0 && SPL_INTRON_TEAM <= 1024, "whole waves, one workgroup");

namespace {

template <uint32_t TEAM>
__global__ __launch_bounds__(TEAM) void spl_intron_kernel(const int32_t *bound_pos, const uint32_t *bound_depth, int64_t n_bound, const int64_t *piece_off, const int32_t *piece_start,
                                                          const int32_t *piece_end, const uint32_t *items, int64_t n_items, uint32_t trim_percent, int64_t *out)
{
    __shared__ splintron::Shared sh;
    const splintron::Depth depth{bound_pos, bound_depth, n_bound};
    for (int64_t k = blockIdx.x; k < n_items; k += gridDim.x) { // (uniform over the workgroup)
        const int64_t i = (int64_t)items[k];
        const int64_t p0 = piece_off[i], p1 = piece_off[i + 1];
        const splintron::Pieces pieces{piece_start + p0, piece_end + p0, p1 - p0};
        splintron::team_intron(threadIdx.x, TEAM, depth, pieces, trim_percent, &sh, out + 4 * i);
    }
}

} // namespace

extern "C" uint32_t spl_dev_intron_grid(int64_t n) { return (uint32_t)(n < 1 ? 1 : n > SPL_INTRON_GRID_MAX ? SPL_INTRON_GRID_MAX : n); }

extern "C" int spl_dev_launch_intron(int team, const int32_t *bound_pos, const uint32_t *bound_depth, int64_t n_bound, const int64_t *piece_off, const int32_t *piece_start,
                                     const int32_t *piece_end, const uint32_t *items, int64_t n_items, int trim_percent, int64_t *out, void *stream)
{
    if (n_items <= 0) return 0;
    if (!piece_off || !piece_start || !piece_end || !items || !out || n_bound < 0 || (n_bound && (!bound_pos || !bound_depth)) || trim_percent < 0 || trim_percent > 49 ||
        (team != 64 && team != SPL_INTRON_TEAM))
        return (int)hipErrorInvalidValue;
    if (team == 64)
        hipLaunchKernelGGL(spl_intron_kernel<64>, dim3(spl_dev_intron_grid(n_items)), dim3(64), 0, (hipStream_t)stream, bound_pos, bound_depth, n_bound, piece_off, piece_start, piece_end, items,
                           n_items, (uint32_t)trim_percent, out);
    else
        hipLaunchKernelGGL(spl_intron_kernel<SPL_INTRON_TEAM>, dim3(spl_dev_intron_grid(n_items)), dim3(SPL_INTRON_TEAM), 0, (hipStream_t)stream, bound_pos, bound_depth, n_bound, piece_off,
                           piece_start, piece_end, items, n_items, (uint32_t)trim_percent, out);
    return (int)hipGetLastError();
}
