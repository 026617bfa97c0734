// spl_motif.hip -- the reads' strand bytes from the genome's splice motifs, written over the BAM-native arrays of a fused read set
// (spl_reads_motif_strand: --strandFromMotif), and the motif codes of a junction table's rows (spl_junction_motifs:
// --canonicalOnly).  The rule is spl_motif_rule.h, which the host compiles too; the genome's form is spl_genome.h's.  gfx950.
//
// Replaces `--outSAMstrandField intronMotif` of the aligner, for files whose aligner was not asked: the reference reads the strand
// a BED line says and has no counterpart.
//
// One launch per segment of the set, a grid-stride loop over its reads, a read a lane, 256 lanes a workgroup, in whatever order the
// reads are.  A read costs its two CIGAR offsets and its ops; only one with an N op loads FLAG and POS and walks, and a junction of
// the walk costs at most four nibble loads of the packed sequence (two where a pair lies in one byte).  Every read's byte is
// written: 0 for the reads the rule passes over.  The tally: a lane keeps its own twelve sums along the loop, the wave adds them up
// by shuffles, the waves' sums meet in LDS, and a workgroup ends with one 64-bit atomicAdd per counter.  Integer sums: exact.
#include <hip/hip_runtime.h>
#include <stdint.h>

#define SPL_HD __device__ __forceinline__
#include "spl_motif.h"
#include "spl_motif_rule.h"
#include "spl_read_view.h"

namespace {

__global__ __launch_bounds__(SPL_MOTIF_TILE) void spl_motif_strand_kernel(const spl_devreads src, uint8_t *xs, int64_t n_ops_total, int64_t first, int64_t n, int32_t shift,
                                                                          const uint8_t *packed, int64_t length, unsigned long long *out)
{
    __shared__ uint32_t s_sum[SPL_MOTIF_TALLY];
    const uint32_t t = threadIdx.x;
    if (t < SPL_MOTIF_TALLY) s_sum[t] = 0u;
    __syncthreads();
    uint32_t mine[SPL_MOTIF_TALLY];
#pragma unroll
    for (int c = 0; c < SPL_MOTIF_TALLY; ++c) mine[c] = 0u;
    const splmotif::NibblePairs pairs{packed};
    for (int64_t r = (int64_t)blockIdx.x * SPL_MOTIF_TILE + t; r < n; r += (int64_t)gridDim.x * SPL_MOTIF_TILE) {
        const int64_t i = first + r;
        uint32_t c0, n_ops;
        spl_ops_of(src.cig_off, i, n_ops_total, &c0, &n_ops);
        bool has_n = false;
        for (uint32_t k = 0; k < n_ops; ++k) has_n = has_n || (src.cigar[c0 + k] & 15u) == (uint32_t)SPL_OP_N;
        uint8_t strand = 0;
        if (has_n) {
            splmotif::ReadMotifs m;
            splmotif::read_motifs((uint32_t)src.flag[i], (int64_t)src.pos[i] + shift, spl_ops_ptr{src.cigar + c0}, n_ops, pairs, length, m);
            strand = m.strand;
#pragma unroll
            for (int c = 0; c < 7; ++c) mine[c] += m.walks[c];
#pragma unroll
            for (int c = 7; c < 11; ++c) mine[c] += m.cls == (uint32_t)c ? 1u : 0u;
            mine[11] += m.outside ? 1u : 0u;
        }
        xs[i] = strand;
    }
#pragma unroll
    for (int c = 0; c < SPL_MOTIF_TALLY; ++c) {
        uint32_t v = mine[c];
        for (int off = 32; off > 0; off >>= 1) v += (uint32_t)__shfl_xor((int)v, off);
        if ((t & 63u) == 0u && v) atomicAdd(&s_sum[c], v);
    }
    __syncthreads();
    if (t < SPL_MOTIF_TALLY && s_sum[t]) atomicAdd(&out[t], (unsigned long long)s_sum[t]);
}

__global__ __launch_bounds__(256) void spl_junction_motifs_kernel(const int32_t *left, const int32_t *right, int64_t n, const uint8_t *packed, int64_t length, uint8_t *code)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    bool outside = false;
    code[i] = (uint8_t)splmotif::junction_code(splmotif::NibblePairs{packed}, length, (int64_t)left[i], (int64_t)right[i], outside);
}

} // namespace

extern "C" int spl_dev_launch_motif_strand(const spl_devreads *src, uint8_t *xs, int64_t n_rec, int64_t n_ops, int64_t first, int64_t n, int32_t shift, const uint8_t *packed,
                                           int64_t length, unsigned long long *out12, void *stream)
{
    if (n <= 0) return 0;
    if (!src || !xs || !out12 || first < 0 || first + n > n_rec || length < 0 || (length && !packed)) return (int)hipErrorInvalidValue;
    const int64_t g = (n + SPL_MOTIF_TILE - 1) / SPL_MOTIF_TILE;
    hipLaunchKernelGGL(spl_motif_strand_kernel, dim3((uint32_t)(g > SPL_MOTIF_GRID_MAX ? SPL_MOTIF_GRID_MAX : g)), dim3(SPL_MOTIF_TILE), 0, (hipStream_t)stream, *src, xs, n_ops, first, n,
                       shift, packed, length, out12);
    return (int)hipGetLastError();
}

extern "C" int spl_dev_launch_junction_motifs(const int32_t *left, const int32_t *right, int64_t n, const uint8_t *packed, int64_t length, uint8_t *code, void *stream)
{
    if (n <= 0) return 0;
    if (!left || !right || !code || length < 0 || (length && !packed)) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(spl_junction_motifs_kernel, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, left, right, n, packed, length, code);
    return (int)hipGetLastError();
}
