// spl_coverage.hip -- per-base read depth of one reference over the BAM-native arrays of a fused read set (spl_coverage: the
// `coverage` command).  The per-read rule is spl_coverage_rule.h, which the host compiles too.  gfx950.
//
// Replaces `samtools sort` + `index` for IGV, or `bedtools genomecov -bg -split` / deepTools `bamCoverage`, over a file this
// library has just decoded: the look at the alignments the reference's README asks for.  The reference has no counterpart.
//
// mark     One launch per segment of the set, a grid-stride loop over its reads, SPL_COV_TILE reads a workgroup and step, a read
//          a lane, in whatever order the reads are.  A lane walks its read's ops where they lie and adds, per clipped block
//          [s, e), +1 at diff[s] and -1 at diff[e] -- uint32 words, sums mod 2^32 (exact while the depth is below 2^32), plain
//          device-scope atomics whose value nobody waits for.  Three predicates a read (seen, contributed, past the end) are
//          counted by the predicate tally of spl_tally_dev.h; the covered bases are summed per lane and across the wave at the end, an atomic
//          a wave.
// compact  Depth changes exactly where diff[i] != 0, i in [0, length).  Pass 1 counts those words per tile of SPL_COV_POS_TILE
//          positions, a 16-byte load a lane; the tile counts are scanned (spl_dev_launch_sort_scan: the caller); pass 2 reads
//          the tiles again and writes (position, delta) in ascending order, a word's place being its tile's offset, the words of
//          the waves in front, of the lanes in front (ballots) and of the lane's own load.  No second array of `length` words.
// Integer sums throughout: exact, and the same for the reads in any order.
//
// spl_coverage_fragments (`coverage --fragments`) has a mark kernel of its own below, in the same geometry over the segment's mate
// table: a fragment's leader marks the union of both mates' blocks, the merge of two block cursors (spl_covfragment_rule.h); the
// count, emit and scan stages are the same.
#include <hip/hip_runtime.h>
#include <stdint.h>

#define SPL_HD __device__ __forceinline__
#include "spl_coverage.h"
#include "spl_coverage_rule.h"
#include "spl_covfragment_rule.h" // a fragment's rule: spl_cov_mark_fragments_kernel
#include "spl_tally_dev.h"       // PredicateTally, wave_add64; wv::lane

namespace {

constexpr uint32_t WAVES = SPL_COV_TILE / 64;
static_assert(SPL_COV_POS_TILE == 4 * SPL_COV_TILE, "compact: four positions a lane, SPL_COV_TILE lanes");

struct DiffMark {
    uint32_t *diff;
    __device__ __forceinline__ void operator()(int64_t s, int64_t e) const
    {
        atomicAdd(&diff[s], 1u);         // (0 <= s < e <= length: the walk clips; diff has length + 1 words)
        atomicAdd(&diff[e], 0xffffffffu); // -1 mod 2^32
    }
};

__global__ __launch_bounds__(SPL_COV_TILE) void spl_cov_mark_kernel(const spl_devreads src, int64_t n_ops_total, int64_t first, int64_t n, int32_t shift, int64_t length, int stranded,
                                                                     int strand, uint32_t *diff, unsigned long long *out)
{
    const uint32_t t = threadIdx.x;
    unsigned long long bases = 0; // this lane's covered bases
    PredicateTally<SPL_COV_COUNTERS> tally;
    const DiffMark mark{diff};
    for (int64_t base = (int64_t)blockIdx.x * SPL_COV_TILE; base < n; base += (int64_t)gridDim.x * SPL_COV_TILE) { // (uniform over the workgroup)
        const int64_t r = base + t;
        uint32_t bits = 0;
        if (r < n) {
            const int64_t i = first + r;
            const uint32_t flag = src.flag[i];
            const int64_t pos = (int64_t)src.pos[i];
            uint32_t c0, n_ops;
            spl_ops_of(src.cig_off, i, n_ops_total, &c0, &n_ops);
            bits = SPL_COV_SEEN;
            if (spl_cov_eligible(flag, pos, n_ops) && spl_cov_on_track(flag, stranded, strand)) {
                int64_t covered = 0;
                bits |= spl_cov_walk(spl_ops_ptr{src.cigar + c0}, n_ops, pos - 1 + (int64_t)shift, length, mark, &covered);
                bases += (unsigned long long)covered;
            }
        }
        tally.add(bits);
    }
    tally.finish(out);
    wave_add64(&out[SPL_COV_COUNTERS], bases);
}

struct FragmentSlots { // out: the per-read kernel's four sums where they were, and the pairs behind them
    __device__ __forceinline__ uint32_t operator()(uint32_t c) const { return c < SPL_COV_COUNTERS ? c : SPL_COV_COUNTERS + 1; }
};

// Fragments (spl_coverage_fragments): the same launch over the segment with its mate table (spl_mates.hip) beside the arrays, the
// same diff array and atomics.  A lane first asks whether its read's mate takes part in the call -- a dependent load of the mate's
// FLAG, POS and CIGAR offsets from wherever that read lies in the segment.  A silent lane then idles; a leader walks its own ops
// and its mate's as two block cursors and marks their union (spl_cov_fragment_walk): at most the two reads' marks, fewer where the
// mates overlap or abut.  Nothing is stored per lane.  One ballot counter more: the pairs whose union was taken.
__global__ __launch_bounds__(SPL_COV_TILE) void spl_cov_mark_fragments_kernel(const spl_devreads src, int64_t n_ops_total, int64_t first, int64_t n, int32_t shift, int64_t length,
                                                                               int stranded, int strand, const uint32_t *mate, uint32_t *diff, unsigned long long *out)
{
    const uint32_t t = threadIdx.x;
    const spl_read_view reads{src.pos, src.flag, src.cig_off, src.cigar, n_ops_total};
    unsigned long long bases = 0; // this lane's covered bases
    PredicateTally<SPL_COVF_COUNTERS> tally;
    DiffMark mark{diff};
    for (int64_t base = (int64_t)blockIdx.x * SPL_COV_TILE; base < n; base += (int64_t)gridDim.x * SPL_COV_TILE) { // (uniform over the workgroup)
        const int64_t r = base + t;
        uint32_t bits = 0;
        if (r < n) {
            bits = SPL_COV_SEEN;
            spl_cov_side lead, other;
            if (spl_cov_fragment_sides(reads, first, n, r, mate, (int64_t)shift, stranded, strand, &lead, &other) == SPL_COVF_LEADS) {
                int64_t covered = 0;
                bits |= spl_cov_fragment_walk<spl_ops_ptr>(src.cigar, lead, other, length, mark, &covered);
                bases += (unsigned long long)covered;
            }
        }
        tally.add(bits);
    }
    tally.finish(out, FragmentSlots{});
    wave_add64(&out[SPL_COV_COUNTERS], bases);
}

// The four words of this lane's load of tile `tile`, those at or beyond `length` as zero: bit k of the result = word k is not zero.
__device__ __forceinline__ uint32_t load_tile_words(const uint32_t *diff, int64_t length, int64_t tile, uint32_t t, uint4 &w)
{
    const int64_t p = tile * SPL_COV_POS_TILE + 4 * (int64_t)t;
    w = make_uint4(0u, 0u, 0u, 0u);
    if (p < length) w = *reinterpret_cast<const uint4 *>(diff + p); // (whole tiles are allocated: spl_dev_cov_diff_words)
    return (w.x != 0u && p < length ? 1u : 0u) | (w.y != 0u && p + 1 < length ? 2u : 0u) | (w.z != 0u && p + 2 < length ? 4u : 0u) | (w.w != 0u && p + 3 < length ? 8u : 0u);
}

__global__ __launch_bounds__(SPL_COV_TILE) void spl_cov_count_kernel(const uint32_t *diff, int64_t length, int64_t n_tiles, uint32_t *tile_count)
{
    __shared__ uint32_t s_wave[WAVES];
    const uint32_t t = threadIdx.x, lane = wv::lane(), wave = t >> 6;
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) { // (uniform over the workgroup)
        uint4 w;
        const uint32_t nz = load_tile_words(diff, length, tile, t, w);
        uint32_t sum = 0;
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) sum += (uint32_t)__popcll(__ballot((nz >> k) & 1u));
        if (lane == 0) s_wave[wave] = sum;
        __syncthreads();
        if (t == 0) {
            uint32_t all = 0;
            for (uint32_t k = 0; k < WAVES; ++k) all += s_wave[k];
            tile_count[tile] = all;
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(SPL_COV_TILE) void spl_cov_emit_kernel(const uint32_t *diff, int64_t length, int64_t n_tiles, const uint32_t *tile_sum, int32_t *pos, uint32_t *delta,
                                                                     int64_t n_out)
{
    __shared__ uint32_t s_wave[WAVES];
    const uint32_t t = threadIdx.x, lane = wv::lane(), wave = t >> 6;
    const unsigned long long in_front = lane ? (~0ull >> (64u - lane)) : 0ull; // the lanes below this one
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) { // (uniform over the workgroup)
        uint4 w;
        const uint32_t nz = load_tile_words(diff, length, tile, t, w);
        uint32_t before = 0, sum = 0; // words of the lanes in front of this one, and of the whole wave
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) {
            const unsigned long long b = __ballot((nz >> k) & 1u);
            before += (uint32_t)__popcll(b & in_front);
            sum += (uint32_t)__popcll(b);
        }
        if (lane == 0) s_wave[wave] = sum;
        __syncthreads();
        int64_t at = tile ? (int64_t)tile_sum[tile - 1] : 0;
        for (uint32_t k = 0; k < wave; ++k) at += s_wave[k];
        at += before;
        const int64_t p = tile * SPL_COV_POS_TILE + 4 * (int64_t)t;
        const uint32_t v[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k)
            if ((nz >> k) & 1u) {
                if (at < n_out) { pos[at] = (int32_t)(p + k); delta[at] = v[k]; } // (at < n_out always: said for the memory's sake)
                ++at;
            }
        __syncthreads();
    }
}

int64_t pos_tiles(int64_t length) { return (length + SPL_COV_POS_TILE - 1) / SPL_COV_POS_TILE; }

} // namespace

extern "C" uint32_t spl_dev_cov_grid(int64_t n)
{
    const int64_t g = (n + SPL_COV_TILE - 1) / SPL_COV_TILE;
    return (uint32_t)(g < 1 ? 1 : g > SPL_COV_GRID_MAX ? SPL_COV_GRID_MAX : g);
}

extern "C" uint32_t spl_dev_cov_pos_grid(int64_t n_tiles) { return (uint32_t)(n_tiles < 1 ? 1 : n_tiles > SPL_COV_POS_GRID_MAX ? SPL_COV_POS_GRID_MAX : n_tiles); }

extern "C" int64_t spl_dev_cov_diff_words(int64_t length) { return (pos_tiles(length + 1)) * SPL_COV_POS_TILE; }

extern "C" int spl_dev_launch_cov_mark(const spl_devreads *src, int64_t n_rec, int64_t n_ops, int64_t first, int64_t n, int32_t shift, int64_t length, int stranded, int strand,
                                       uint32_t *diff, unsigned long long *out4, void *stream)
{
    if (n <= 0) return 0;
    if (!src || !diff || !out4 || first < 0 || first + n > n_rec || length < 1 || length > SPL_COV_LENGTH_MAX || stranded < 0 || stranded > 2) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(spl_cov_mark_kernel, dim3(spl_dev_cov_grid(n)), dim3(SPL_COV_TILE), 0, (hipStream_t)stream, *src, n_ops, first, n, shift, length, stranded, strand, diff, out4);
    return (int)hipGetLastError();
}

extern "C" int spl_dev_launch_cov_mark_fragments(const spl_devreads *src, int64_t n_rec, int64_t n_ops, int64_t first, int64_t n, int32_t shift, int64_t length, int stranded, int strand,
                                                 const uint32_t *mate, uint32_t *diff, unsigned long long *out5, void *stream)
{
    if (n <= 0) return 0;
    if (!src || !mate || !diff || !out5 || first < 0 || first + n > n_rec || length < 1 || length > SPL_COV_LENGTH_MAX || stranded < 0 || stranded > 2) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(spl_cov_mark_fragments_kernel, dim3(spl_dev_cov_grid(n)), dim3(SPL_COV_TILE), 0, (hipStream_t)stream, *src, n_ops, first, n, shift, length, stranded, strand, mate, diff,
                       out5);
    return (int)hipGetLastError();
}

extern "C" int spl_dev_launch_cov_count(const uint32_t *diff, int64_t length, uint32_t *tile_count, void *stream)
{
    if (!diff || !tile_count || length < 1 || length > SPL_COV_LENGTH_MAX) return (int)hipErrorInvalidValue;
    const int64_t n_tiles = pos_tiles(length);
    hipLaunchKernelGGL(spl_cov_count_kernel, dim3(spl_dev_cov_pos_grid(n_tiles)), dim3(SPL_COV_TILE), 0, (hipStream_t)stream, diff, length, n_tiles, tile_count);
    return (int)hipGetLastError();
}

extern "C" int spl_dev_launch_cov_emit(const uint32_t *diff, int64_t length, const uint32_t *tile_sum, int32_t *pos, uint32_t *delta, int64_t n_out, void *stream)
{
    if (n_out <= 0) return 0;
    if (!diff || !tile_sum || !pos || !delta || length < 1 || length > SPL_COV_LENGTH_MAX) return (int)hipErrorInvalidValue;
    const int64_t n_tiles = pos_tiles(length);
    hipLaunchKernelGGL(spl_cov_emit_kernel, dim3(spl_dev_cov_pos_grid(n_tiles)), dim3(SPL_COV_TILE), 0, (hipStream_t)stream, diff, length, n_tiles, tile_sum, pos, delta, n_out);
    return (int)hipGetLastError();
}
