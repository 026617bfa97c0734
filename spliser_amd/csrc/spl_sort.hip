// spl_sort.hip -- a stable LSD radix sort of (reference id, POS) keys with the record's index as payload, and the gather of the
// records' arrays into the sorted order: what `--anyOrder` (spl_bam_set_any_order) runs between the device decode's last
// extraction and the bounds kernel when the file is not in coordinate order.  gfx950; no library (rocPRIM, hipCUB, Thrust).
//
// The sort's kernels are one wave a workgroup, their bodies in spl_sort_wave.h (the method is described there; the same source runs
// under the host's wave emulator).  Grids are sized by the work: at most splsort::MAX_PARTS waves a launch, each walking a
// contiguous stretch of whole tiles; the gather's kernels are plain grid-stride loops.
//
// Replaces `samtools sort` in front of SpliSER_v0_1_8.py:422.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "spl_sort.h"
#include "spl_sort_wave.h"

namespace {
constexpr uint32_t GATHER_BLOCK = 256u, GATHER_GRID = 2048u;
uint32_t gather_grid(uint64_t n) { return (uint32_t)std::min<uint64_t>((n + GATHER_BLOCK - 1u) / GATHER_BLOCK, GATHER_GRID); }

struct Work { uint32_t *hist, *totals; };
Work work_of(void *work, uint32_t parts) { return Work{(uint32_t *)work, (uint32_t *)work + (size_t)splsort::RADIX * parts}; }
} // namespace

__global__ __launch_bounds__(64) void spl_sort_histogram_kernel(const uint64_t *keys, uint64_t n, uint32_t shift, uint64_t n_tiles, uint64_t tiles_per_part, uint32_t *hist)
{
    __shared__ uint32_t h[splsort::RADIX];
    const uint64_t t0 = (uint64_t)blockIdx.x * tiles_per_part, t1 = min(n_tiles, t0 + tiles_per_part);
    splsort::part_histogram(keys, n, shift, t0, t1, h, hist, gridDim.x, blockIdx.x);
}

__global__ __launch_bounds__(64) void spl_sort_digit_scan_kernel(uint32_t *hist, uint32_t parts, uint32_t *totals)
{
    splsort::digit_scan(hist + (size_t)blockIdx.x * parts, parts, totals + blockIdx.x);
}

__global__ __launch_bounds__(64) void spl_sort_scatter_kernel(const uint64_t *keys_in, const uint32_t *perm_in, uint64_t n, uint32_t shift, uint64_t n_tiles, uint64_t tiles_per_part,
                                                               const uint32_t *hist, const uint32_t *totals, uint64_t *keys_out, uint32_t *perm_out)
{
    __shared__ uint32_t offs[splsort::RADIX];
    const uint64_t t0 = (uint64_t)blockIdx.x * tiles_per_part, t1 = min(n_tiles, t0 + tiles_per_part);
    splsort::part_scatter(keys_in, perm_in, n, shift, t0, t1, offs, hist, totals, gridDim.x, blockIdx.x, keys_out, perm_out);
}

__global__ __launch_bounds__(64) void spl_sort_part_sum_kernel(const uint32_t *v, uint64_t n, uint64_t n_tiles, uint64_t tiles_per_part, uint32_t *partial)
{
    const uint64_t t0 = (uint64_t)blockIdx.x * tiles_per_part, t1 = min(n_tiles, t0 + tiles_per_part);
    splsort::part_sum(v, n, t0, t1, partial, blockIdx.x);
}

__global__ __launch_bounds__(64) void spl_sort_part_rescan_kernel(uint32_t *v, uint64_t n, uint64_t n_tiles, uint64_t tiles_per_part, const uint32_t *partial)
{
    const uint64_t t0 = (uint64_t)blockIdx.x * tiles_per_part, t1 = min(n_tiles, t0 + tiles_per_part);
    splsort::part_rescan(v, n, t0, t1, partial, blockIdx.x);
}

__global__ __launch_bounds__(256) void spl_sort_make_keys_kernel(const int32_t *tid, const int32_t *pos, uint64_t n, uint64_t *keys)
{
    for (uint64_t i = (uint64_t)blockIdx.x * GATHER_BLOCK + threadIdx.x; i < n; i += (uint64_t)gridDim.x * GATHER_BLOCK)
        keys[i] = (uint64_t)(uint32_t)tid[i] << 32 | (uint64_t)(uint32_t)pos[i];
}

template <bool XS>
__global__ __launch_bounds__(256) void spl_sort_gather_kernel(const uint32_t *perm, const uint64_t *keys, uint64_t n, const int32_t *pos, const uint16_t *flag, const uint8_t *xs,
                                                              const uint32_t *cig_off, int32_t *pos_out, uint16_t *flag_out, uint8_t *xs_out, int32_t *tid_out, uint32_t *cig_off_out)
{
    if (blockIdx.x == 0 && threadIdx.x == 0) cig_off_out[0] = 0u;
    for (uint64_t i = (uint64_t)blockIdx.x * GATHER_BLOCK + threadIdx.x; i < n; i += (uint64_t)gridDim.x * GATHER_BLOCK) {
        uint64_t j = perm[i];
        if (j >= n) j = 0; // (a permutation of 0 .. n - 1: said for the memory's sake)
        pos_out[i] = pos[j];
        flag_out[i] = flag[j];
        if (XS) xs_out[i] = xs[j];
        tid_out[i] = (int32_t)(uint32_t)(keys[i] >> 32);
        cig_off_out[i + 1] = cig_off[j + 1] - cig_off[j];
    }
}

__global__ __launch_bounds__(256) void spl_sort_cigar_kernel(const uint32_t *perm, uint64_t n, const uint32_t *cig_off, const uint32_t *cigar, const uint32_t *cig_off_out, uint32_t *cigar_out)
{
    for (uint64_t i = (uint64_t)blockIdx.x * GATHER_BLOCK + threadIdx.x; i < n; i += (uint64_t)gridDim.x * GATHER_BLOCK) {
        uint64_t j = perm[i];
        if (j >= n) j = 0;
        const uint32_t from = cig_off[j], count = cig_off[j + 1] - from, to = cig_off_out[i];
        if (cig_off_out[i + 1] - to != count) continue; // (the scan's offsets are these counts' sums: said for the memory's sake)
        for (uint32_t k = 0; k < count; ++k) cigar_out[to + k] = cigar[from + k];
    }
}

extern "C" uint32_t spl_dev_sort_parts(uint64_t n) { return splsort::plan_for(n, splsort::MAX_PARTS).parts; }
extern "C" size_t spl_dev_sort_work_bytes(uint64_t n) { return 4u * ((size_t)splsort::RADIX * std::max<uint32_t>(spl_dev_sort_parts(n), 1u) + splsort::RADIX + 64u); }
extern "C" uint32_t spl_dev_sort_passes(uint32_t pos_bits, uint32_t tid_bits, uint32_t *shifts) { return splsort::pass_shifts2(pos_bits, tid_bits, shifts); }

extern "C" int spl_dev_launch_sort_make_keys(const int32_t *tid, const int32_t *pos, uint64_t n, uint64_t *keys, void *st)
{
    if (n == 0) return 0;
    hipLaunchKernelGGL(spl_sort_make_keys_kernel, dim3(gather_grid(n)), dim3(GATHER_BLOCK), 0, (hipStream_t)st, tid, pos, n, keys);
    return (int)hipGetLastError();
}

extern "C" int spl_dev_launch_sort_pass(const uint64_t *keys_in, const uint32_t *perm_in, uint64_t n, uint32_t shift, uint64_t *keys_out, uint32_t *perm_out, void *work, void *st)
{
    if (n == 0) return 0;
    if (!work || n > 0xfffffff0ull || shift > 56u || (const void *)keys_in == (const void *)keys_out || (perm_in && perm_in == perm_out)) return (int)hipErrorInvalidValue;
    const splsort::Plan pl = splsort::plan_for(n, splsort::MAX_PARTS);
    const Work w = work_of(work, pl.parts);
    hipLaunchKernelGGL(spl_sort_histogram_kernel, dim3(pl.parts), dim3(64), 0, (hipStream_t)st, keys_in, n, shift, pl.n_tiles, pl.tiles_per_part, w.hist);
    hipLaunchKernelGGL(spl_sort_digit_scan_kernel, dim3(splsort::RADIX), dim3(64), 0, (hipStream_t)st, w.hist, pl.parts, w.totals);
    hipLaunchKernelGGL(spl_sort_scatter_kernel, dim3(pl.parts), dim3(64), 0, (hipStream_t)st, keys_in, perm_in, n, shift, pl.n_tiles, pl.tiles_per_part, (const uint32_t *)w.hist,
                       (const uint32_t *)w.totals, keys_out, perm_out);
    return (int)hipGetLastError();
}

extern "C" int spl_dev_launch_sort_gather(const uint32_t *perm, const uint64_t *keys, uint64_t n, const int32_t *pos, const uint16_t *flag, const uint8_t *xs, const uint32_t *cig_off,
                                          int32_t *pos_out, uint16_t *flag_out, uint8_t *xs_out, int32_t *tid_out, uint32_t *cig_off_out, void *st)
{
    if (n == 0) return 0;
    if ((xs == nullptr) != (xs_out == nullptr)) return (int)hipErrorInvalidValue;
    if (xs)
        hipLaunchKernelGGL(spl_sort_gather_kernel<true>, dim3(gather_grid(n)), dim3(GATHER_BLOCK), 0, (hipStream_t)st, perm, keys, n, pos, flag, xs, cig_off, pos_out, flag_out, xs_out, tid_out, cig_off_out);
    else
        hipLaunchKernelGGL(spl_sort_gather_kernel<false>, dim3(gather_grid(n)), dim3(GATHER_BLOCK), 0, (hipStream_t)st, perm, keys, n, pos, flag, xs, cig_off, pos_out, flag_out, xs_out, tid_out, cig_off_out);
    return (int)hipGetLastError();
}

extern "C" int spl_dev_launch_sort_scan(uint32_t *v, uint64_t n, void *work, void *st)
{
    if (n == 0) return 0;
    if (!work || n > 0xfffffff0ull) return (int)hipErrorInvalidValue;
    const splsort::Plan pl = splsort::plan_for(n, splsort::MAX_PARTS);
    uint32_t *partial = (uint32_t *)work; // (parts + 1 words of the histograms' room)
    hipLaunchKernelGGL(spl_sort_part_sum_kernel, dim3(pl.parts), dim3(64), 0, (hipStream_t)st, (const uint32_t *)v, n, pl.n_tiles, pl.tiles_per_part, partial);
    hipLaunchKernelGGL(spl_sort_digit_scan_kernel, dim3(1), dim3(64), 0, (hipStream_t)st, partial, pl.parts, partial + pl.parts);
    hipLaunchKernelGGL(spl_sort_part_rescan_kernel, dim3(pl.parts), dim3(64), 0, (hipStream_t)st, v, n, pl.n_tiles, pl.tiles_per_part, (const uint32_t *)partial);
    return (int)hipGetLastError();
}

extern "C" int spl_dev_launch_sort_cigar(const uint32_t *perm, uint64_t n, const uint32_t *cig_off, const uint32_t *cigar, const uint32_t *cig_off_out, uint32_t *cigar_out, void *st)
{
    if (n == 0) return 0;
    hipLaunchKernelGGL(spl_sort_cigar_kernel, dim3(gather_grid(n)), dim3(GATHER_BLOCK), 0, (hipStream_t)st, perm, n, cig_off, cigar, cig_off_out, cigar_out);
    return (int)hipGetLastError();
}
