// spl_subsample.hip -- the read set of a reproducible fraction of a fused read set's reads (spl_reads_subsample): an
// order-preserving stream compaction of the set's arrays into a second set of arrays, out of place.  The rule -- which read is
// kept -- is spl_subsample_rule.h, which the host compiles too; the kernels' bodies are spl_subsample_wave.h (the method is
// described there; the same source runs under the host's wave emulator).  gfx950; no library (rocPRIM, hipCUB, Thrust).
//
// One wave a workgroup and a tile (splsub::TILE reads) a wave, in both launches; between them the caller scans the tiles' two rows
// of totals with spl_sort.hip's device-wide scan.  No atomics: the result is bit-identical from run to run.
//
// Replaces `samtools view -s` in front of another run of the pipeline.  The reference has no counterpart.
#include <hip/hip_runtime.h>
#include <stdint.h>

#define SPL_HD __device__ __forceinline__
#include "spl_subsample.h"
#include "spl_subsample_wave.h"

namespace {

__global__ __launch_bounds__(64) void spl_subsample_count_kernel(const splsub::Src src, const splsub::Seg *segs, uint32_t n_seg, uint64_t n_tiles, uint64_t salt, uint64_t threshold,
                                                                 uint32_t *rows)
{
    const uint64_t t = blockIdx.x;
    int64_t lo, hi, base;
    splsub::tile_range(segs, n_seg, t, &lo, &hi, &base);
    splsub::tile_count(src, lo, hi, salt, threshold, rows + t, rows + n_tiles + t);
}

__global__ __launch_bounds__(64) void spl_subsample_ends_kernel(const uint32_t *rows, const splsub::Seg *segs, uint32_t n_seg, uint64_t n_tiles, uint32_t *ends)
{
    for (uint32_t k = blockIdx.x * 64u + threadIdx.x; k < n_seg; k += gridDim.x * 64u) {
        uint64_t end = k + 1u < n_seg ? segs[k + 1u].tile0 : n_tiles;
        if (end > n_tiles) end = n_tiles; // (tile0 ascends to n_tiles: said for the memory's sake)
        ends[k] = end ? rows[end - 1u] : 0u;
        ends[n_seg + k] = end ? rows[n_tiles + end - 1u] : 0u;
    }
}

__global__ __launch_bounds__(64) void spl_subsample_write_kernel(const splsub::Src src, const splsub::Dst dst, const splsub::Seg *segs, uint32_t n_seg, uint64_t n_tiles, uint64_t salt,
                                                                 uint64_t threshold, const uint32_t *rows)
{
    const uint64_t t = blockIdx.x;
    if (t == 0u && threadIdx.x == 0u) dst.cig_off[dst.n_rec] = (uint32_t)dst.n_ops;
    int64_t lo, hi, base;
    splsub::tile_range(segs, n_seg, t, &lo, &hi, &base);
    splsub::tile_write(src, dst, lo, hi, base, salt, threshold, t ? rows[t - 1u] : 0u, t ? rows[n_tiles + t - 1u] : 0u);
}

} // namespace

extern "C" uint32_t spl_dev_subsample_tile(void) { return splsub::TILE; }

extern "C" int spl_dev_launch_subsample_count(const splsub::Src *src, const splsub::Seg *d_segs, uint32_t n_seg, uint64_t n_tiles, uint64_t salt, uint64_t threshold, uint32_t *rows, void *stream)
{
    if (n_tiles == 0) return 0;
    if (!src || !src->key || !d_segs || !n_seg || !rows || n_tiles > 0x7fffffffull) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(spl_subsample_count_kernel, dim3((uint32_t)n_tiles), dim3(64), 0, (hipStream_t)stream, *src, d_segs, n_seg, n_tiles, salt, threshold, rows);
    return (int)hipGetLastError();
}

extern "C" int spl_dev_launch_subsample_ends(const uint32_t *rows, const splsub::Seg *d_segs, uint32_t n_seg, uint64_t n_tiles, uint32_t *ends, void *stream)
{
    if (n_seg == 0) return 0;
    if (!rows || !d_segs || !ends || n_tiles == 0) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(spl_subsample_ends_kernel, dim3(n_seg < 64u * 256u ? (n_seg + 63u) / 64u : 256u), dim3(64), 0, (hipStream_t)stream, rows, d_segs, n_seg, n_tiles, ends);
    return (int)hipGetLastError();
}

extern "C" int spl_dev_launch_subsample_write(const splsub::Src *src, const splsub::Dst *dst, const splsub::Seg *d_segs, uint32_t n_seg, uint64_t n_tiles, uint64_t salt, uint64_t threshold,
                                              const uint32_t *rows, void *stream)
{
    if (n_tiles == 0) return 0;
    if (!src || !src->key || !dst || !dst->key || !dst->cig_off || !d_segs || !n_seg || !rows || n_tiles > 0x7fffffffull || (src->xs == nullptr) != (dst->xs == nullptr))
        return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(spl_subsample_write_kernel, dim3((uint32_t)n_tiles), dim3(64), 0, (hipStream_t)stream, *src, *dst, d_segs, n_seg, n_tiles, salt, threshold, rows);
    return (int)hipGetLastError();
}
