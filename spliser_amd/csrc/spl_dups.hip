// spl_dups.hip -- the duplicate marks of one segment of a fused read set (spl_reads_duplicates) and the read set without the marked
// reads (spl_reads_dedup).  The rule -- who is examined, a fragment's signature, who is a group's representative -- is
// spl_dup_rule.h, which the host compiles too.  gfx950; no library (rocPRIM, hipCUB, Thrust).
//
// Replaces Picard MarkDuplicates / `samtools fixmate` + `samtools markdup` in front of `--excludeFlags 0x400`: a sorted copy of the
// file and a rewrite of it.  The reference has no counterpart.
//
// Four stages a segment.  LEAD: a read a lane asks the mate table what it is to the rule (spl_dup_lead_kernel; the counters of the
// examined reads are a ballot and a popcount per wave and step, meeting in LDS, one atomic per counter and workgroup); the marks
// become their prefix sums by spl_sort.hip's scan, and every leader writes its fragment's element -- three words and its own index
// -- to the place its sum names (spl_dup_signature_kernel: the leader walks its own ops and, by a dependent load through the mate
// table, its mate's, as the fragment coverage kernel does; a forward read's walk ends at its first op that is no clip).  SORT: the
// caller's, by (W0, W1, W2), least significant word first, stable.  MARK: an element a lane, one comparison with the element in
// front (spl_dup_mark_kernel).  GROUPS: a group's head finds its end by binary search and adds to a 256-bin histogram in LDS
// (spl_dup_groups_kernel), a workgroup ending with one 64-bit integer add per touched bin.  Integer atomics only: the same words
// from run to run.  The geometry is spl_mates.hip's: a grid-stride loop, SPL_DUP_TILE a workgroup and step.
//
// The compaction by mark is spl_subsample.hip's two launches with the keep decision of spl_dups_wave.h.
#include <hip/hip_runtime.h>
#include <stdint.h>

#define SPL_HD __device__ __forceinline__
#include "spl_dup_rule.h"
#include "spl_dups.h"
#include "spl_dups_wave.h"
#include "spl_mates.h"
#include "spl_wave.h"

static_assert(SPL_DUP_TILE % 64 == 0, "whole waves: the ballots are called by all 64 lanes");
static_assert(SPL_DUP_TILE >= SPL_DUP_BINS, "a lane a bin when the workgroup's histogram goes out");

namespace {

__device__ __forceinline__ spl_read_view view_of(const splsub::Src &s) { return spl_read_view{s.pos, s.flag, s.cig_off, s.cigar, s.n_ops}; }

__global__ __launch_bounds__(SPL_DUP_TILE) void spl_dup_lead_kernel(const splsub::Src src, int64_t first, int64_t n, const uint32_t *mate, uint32_t *lead, unsigned long long *counters)
{
    __shared__ uint32_t s_sum[4];
    const uint32_t t = threadIdx.x;
    if (t < 4u) s_sum[t] = 0u;
    __syncthreads();
    const spl_read_view reads = view_of(src);
    uint32_t examined = 0, pairs = 0, singles = 0, flagged = 0; // lane 0 of a wave: the wave's sums (at most 64 a step)
    for (int64_t base = (int64_t)blockIdx.x * SPL_DUP_TILE; base < n; base += (int64_t)gridDim.x * SPL_DUP_TILE) { // (uniform over the workgroup)
        const int64_t r = base + t;
        uint32_t what = SPL_FRAG_OUT;
        spl_frag_side me{0u, 0u, 0, 0u}, its{0u, 0u, 0, 0u};
        if (r < n) {
            what = spl_dup_sides(reads, first, n, r, mate, &me, &its);
            lead[r] = what == SPL_FRAG_LEADS ? 1u : 0u;
        }
        examined += wv::popc64(wv::ballot(what != SPL_FRAG_OUT));
        pairs += wv::popc64(wv::ballot(what == SPL_FRAG_LEADS && its.n_ops != 0u));
        singles += wv::popc64(wv::ballot(what == SPL_FRAG_LEADS && its.n_ops == 0u));
        flagged += wv::popc64(wv::ballot(what != SPL_FRAG_OUT && (me.flag & 0x400u)));
    }
    if (wv::lane() == 0u) {
        if (examined) atomicAdd(&s_sum[0], examined);
        if (pairs) atomicAdd(&s_sum[1], pairs);
        if (singles) atomicAdd(&s_sum[2], singles);
        if (flagged) atomicAdd(&s_sum[3], flagged);
    }
    __syncthreads();
    if (t < 3u && s_sum[t]) atomicAdd(&counters[1u + t], (unsigned long long)s_sum[t]);
    if (t == 3u && s_sum[3]) atomicAdd(&counters[6], (unsigned long long)s_sum[3]);
}

__global__ __launch_bounds__(SPL_DUP_TILE) void spl_dup_signature_kernel(const splsub::Src src, int64_t first, int64_t n, const uint32_t *mate, const uint32_t *scan, int64_t n_el,
                                                                          uint64_t *w0, uint64_t *w1, uint64_t *w2, uint32_t *leader)
{
    const spl_read_view reads = view_of(src);
    for (int64_t r = (int64_t)blockIdx.x * SPL_DUP_TILE + threadIdx.x; r < n; r += (int64_t)gridDim.x * SPL_DUP_TILE) {
        const uint32_t here = scan[r], before = r ? scan[r - 1] : 0u;
        if (here == before || (int64_t)before >= n_el) continue; // (before < scan[n - 1] = n_el, the elements the caller made room for)
        spl_frag_side me, its;
        if (spl_dup_sides(reads, first, n, r, mate, &me, &its) != SPL_FRAG_LEADS) continue; // (a leader: the scan said so)
        const spl_dup_sig sig = spl_dup_signature(reads, me, its, src.key[first + r]);
        w0[before] = sig.w0;
        w1[before] = sig.w1;
        w2[before] = sig.w2;
        leader[before] = (uint32_t)r;
    }
}

__global__ __launch_bounds__(SPL_DUP_TILE) void spl_dup_mark_kernel(const uint64_t *w0, const uint64_t *w1, const uint32_t *perm, const uint32_t *leader, int64_t n_el,
                                                                     const uint32_t *mate, int64_t n, uint8_t *dup)
{
    for (int64_t j = (int64_t)blockIdx.x * SPL_DUP_TILE + threadIdx.x; j < n_el; j += (int64_t)gridDim.x * SPL_DUP_TILE)
        (void)spl_dup_mark_element(w0, w1, perm, leader, n_el, j, mate, n, dup);
}

__global__ __launch_bounds__(SPL_DUP_TILE) void spl_dup_groups_kernel(const uint64_t *w0, const uint64_t *w1, int64_t n_el, unsigned long long *hist, unsigned long long *counters)
{
    __shared__ uint32_t s_bin[SPL_DUP_BINS];
    __shared__ unsigned long long s_sum[3]; // fragments of the groups in the last bin, duplicate pairs, duplicate singles
    const uint32_t t = threadIdx.x;
    if (t < (uint32_t)SPL_DUP_BINS) s_bin[t] = 0u;
    if (t < 3u) s_sum[t] = 0ull;
    __syncthreads();
    for (int64_t j = (int64_t)blockIdx.x * SPL_DUP_TILE + t; j < n_el; j += (int64_t)gridDim.x * SPL_DUP_TILE) {
        if (j && spl_dup_same(w0, w1, j - 1, j)) continue; // (no head)
        const uint64_t size = (uint64_t)(spl_dup_group_end(w0, w1, n_el, j) - j);
        atomicAdd(&s_bin[(size < (uint64_t)SPL_DUP_BINS ? size : (uint64_t)SPL_DUP_BINS) - 1u], 1u);
        if (size >= (uint64_t)SPL_DUP_BINS) atomicAdd(&s_sum[0], (unsigned long long)size);
        if (size > 1u) atomicAdd(&s_sum[(w0[j] & 2ull) ? 1 : 2], (unsigned long long)(size - 1u));
    }
    __syncthreads();
    if (t < (uint32_t)SPL_DUP_BINS && s_bin[t]) atomicAdd(&hist[t], (unsigned long long)s_bin[t]);
    if (t == 0u && s_sum[0]) atomicAdd(&hist[SPL_DUP_BINS], s_sum[0]);
    if (t == 1u && s_sum[1]) atomicAdd(&counters[4], s_sum[1]);
    if (t == 2u && s_sum[2]) atomicAdd(&counters[5], s_sum[2]);
}

__global__ __launch_bounds__(64) void spl_dedup_count_kernel(const splsub::Src src, const splsub::Seg *segs, uint32_t n_seg, uint64_t n_tiles, const uint8_t *dup, uint32_t *rows)
{
    const uint64_t t = blockIdx.x;
    int64_t lo, hi, base;
    splsub::tile_range(segs, n_seg, t, &lo, &hi, &base);
    spldup::tile_count(src, lo, hi, dup, rows + t, rows + n_tiles + t);
}

__global__ __launch_bounds__(64) void spl_dedup_write_kernel(const splsub::Src src, const splsub::Dst dst, const splsub::Seg *segs, uint32_t n_seg, uint64_t n_tiles, const uint8_t *dup,
                                                             const uint32_t *rows)
{
    const uint64_t t = blockIdx.x;
    if (t == 0u && threadIdx.x == 0u) dst.cig_off[dst.n_rec] = (uint32_t)dst.n_ops;
    int64_t lo, hi, base;
    splsub::tile_range(segs, n_seg, t, &lo, &hi, &base);
    spldup::tile_write(src, dst, lo, hi, base, dup, t ? rows[t - 1u] : 0u, t ? rows[n_tiles + t - 1u] : 0u);
}

bool segment_fits(const splsub::Src *src, int64_t first, int64_t n) { return src && src->key && first >= 0 && n <= 0xfffffff0LL && first + n <= src->n_rec; }

} // namespace

extern "C" int spl_dev_launch_dup_lead(const splsub::Src *src, int64_t first, int64_t n, const uint32_t *mate, uint32_t *lead, unsigned long long *counters, void *stream)
{
    if (n <= 0) return 0;
    if (!segment_fits(src, first, n) || !mate || !lead || !counters) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(spl_dup_lead_kernel, dim3(spl_dev_mate_grid(n)), dim3(SPL_DUP_TILE), 0, (hipStream_t)stream, *src, first, n, mate, lead, counters);
    return (int)hipGetLastError();
}

extern "C" int spl_dev_launch_dup_signature(const splsub::Src *src, int64_t first, int64_t n, const uint32_t *mate, const uint32_t *scan, int64_t n_el, uint64_t *w0, uint64_t *w1,
                                            uint64_t *w2, uint32_t *leader, void *stream)
{
    if (n <= 0 || n_el <= 0) return 0;
    if (!segment_fits(src, first, n) || !mate || !scan || !w0 || !w1 || !w2 || !leader || n_el > n) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(spl_dup_signature_kernel, dim3(spl_dev_mate_grid(n)), dim3(SPL_DUP_TILE), 0, (hipStream_t)stream, *src, first, n, mate, scan, n_el, w0, w1, w2, leader);
    return (int)hipGetLastError();
}

extern "C" int spl_dev_launch_dup_mark(const uint64_t *w0, const uint64_t *w1, const uint32_t *perm, const uint32_t *leader, int64_t n_el, const uint32_t *mate, int64_t n, uint8_t *dup,
                                       void *stream)
{
    if (n_el <= 0) return 0;
    if (!w0 || !w1 || !perm || !leader || !mate || !dup || n_el > n) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(spl_dup_mark_kernel, dim3(spl_dev_mate_grid(n_el)), dim3(SPL_DUP_TILE), 0, (hipStream_t)stream, w0, w1, perm, leader, n_el, mate, n, dup);
    return (int)hipGetLastError();
}

extern "C" int spl_dev_launch_dup_groups(const uint64_t *w0, const uint64_t *w1, int64_t n_el, unsigned long long *hist, unsigned long long *counters, void *stream)
{
    if (n_el <= 0) return 0;
    if (!w0 || !w1 || !hist || !counters) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(spl_dup_groups_kernel, dim3(spl_dev_mate_grid(n_el)), dim3(SPL_DUP_TILE), 0, (hipStream_t)stream, w0, w1, n_el, hist, counters);
    return (int)hipGetLastError();
}

extern "C" int spl_dev_launch_dedup_count(const splsub::Src *src, const splsub::Seg *d_segs, uint32_t n_seg, uint64_t n_tiles, const uint8_t *dup, uint32_t *rows, void *stream)
{
    if (n_tiles == 0) return 0;
    if (!src || !src->key || !d_segs || !n_seg || !dup || !rows || n_tiles > 0x7fffffffull) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(spl_dedup_count_kernel, dim3((uint32_t)n_tiles), dim3(64), 0, (hipStream_t)stream, *src, d_segs, n_seg, n_tiles, dup, rows);
    return (int)hipGetLastError();
}

extern "C" int spl_dev_launch_dedup_write(const splsub::Src *src, const splsub::Dst *dst, const splsub::Seg *d_segs, uint32_t n_seg, uint64_t n_tiles, const uint8_t *dup,
                                          const uint32_t *rows, void *stream)
{
    if (n_tiles == 0) return 0;
    if (!src || !src->key || !dst || !dst->key || !dst->cig_off || !d_segs || !n_seg || !dup || !rows || n_tiles > 0x7fffffffull || (src->xs == nullptr) != (dst->xs == nullptr))
        return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(spl_dedup_write_kernel, dim3((uint32_t)n_tiles), dim3(64), 0, (hipStream_t)stream, *src, *dst, d_segs, n_seg, n_tiles, dup, rows);
    return (int)hipGetLastError();
}
