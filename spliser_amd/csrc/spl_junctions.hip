// spl_junctions.hip -- the junction table of a FUSED read set (`process` without -b and the `junctions` command
// after a decode on the device): straight from the BAM-native arrays pos / flag / cig_off / cigar, driven by the chunk descriptors
// spl_chunk_slots_kernel writes when the set is finished -- no records in memory, no layout launch.  The table, its key, its hash
// and its compaction are spl_junction_kernel's (spl_kernels.hip: the same table from packed records); the per-read walk is
// spl_junction_walk.h, which the host compiles too.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <stdint.h>

#define SPL_HD __device__ __forceinline__
#include "spl_classify.h"
#include "spl_device.h"
#include "spl_junction_fused.h"
#include "spl_junction_walk.h"
#include "spl_junctionfragment_rule.h" // a fragment's rule: spl_junction_fused_kernel<XS, true>

namespace {

typedef uint32_t spl_u32x4 __attribute__((ext_vector_type(4)));

// Equal keys of a wave's lanes merged, then one insert per distinct key: its count the number of lanes, its anchors their
// maxima.  Every lane of the wave calls this together (`have`: the lane holds a key); `lane` = its number in the wave.
__device__ __forceinline__ void junction_merge_insert(bool have, unsigned long long key, uint32_t a_left, uint32_t a_right, int lane,
                                                      unsigned long long *keys, uint32_t *vals, uint32_t mask, int32_t *err)
{
    unsigned long long todo = __ballot(have);
    while (todo) {
        const int leader = __ffsll((long long)todo) - 1;
        const uint32_t klo = (uint32_t)__shfl((int)(uint32_t)key, leader), khi = (uint32_t)__shfl((int)(uint32_t)(key >> 32), leader);
        const bool same = have && (uint32_t)key == klo && (uint32_t)(key >> 32) == khi;
        const unsigned long long grp = __ballot(same);
        uint32_t ml = same ? a_left : 0u, mr = same ? a_right : 0u;
        for (int off = 32; off > 0; off >>= 1) { // wave max over the group (others contribute 0)
            const uint32_t xl = (uint32_t)__shfl_xor((int)ml, off), xr = (uint32_t)__shfl_xor((int)mr, off);
            ml = xl > ml ? xl : ml;
            mr = xr > mr ? xr : mr;
        }
        if (lane == leader) {
            const unsigned long long kk = ((unsigned long long)khi << 32) | klo;
            uint32_t h = (uint32_t)(kk * 0x9E3779B97F4A7C15ull >> 32);
            for (uint32_t probe = 0;; ++probe) {
                const uint32_t slot = (h + probe) & mask;
                const unsigned long long old = atomicCAS(&keys[slot], ~0ull, kk);
                if (old == ~0ull || old == kk) {
                    atomicAdd(&vals[3u * slot], (uint32_t)__popcll(grp));
                    atomicMax(&vals[3u * slot + 1u], ml);
                    atomicMax(&vals[3u * slot + 2u], mr);
                    break;
                }
                if (probe > mask) { atomicOr(err, SPL_DEV_ERR_TABLE); break; } // cannot happen: the table is at most half full
            }
        }
        todo &= ~grp;
    }
}

// ---- the same table from a FUSED read set: straight from pos / flag / cig_off / cigar, driven by the chunk descriptors of
// spl_chunk_slots_kernel (first read, number of reads, shift) -- no records, no layout launch.
//
// One workgroup per chunk, a TILE of 256 reads at a time (a read a lane):
//   1. the lane's two cig_off words give its op count before anything else is touched: with min_anchor > 0 a read of fewer than
//      three ops supports no junction (spljw::min_ops; exact), with min_anchor = 0 one op is enough and the op codes decide;
//   2. the tile's ops -- ONE contiguous stretch of the CIGAR array -- come into LDS in 16-byte loads (the first JSTAGE words of
//      them; what lies beyond, long-read CIGARs, is read where it is);
//   3. a lane whose read has an N op among its ops (looked for in LDS; a read whose ops are not all staged counts as having one)
//      and is mapped and placed enters the tile's LIST: ballot + mbcnt inside the wave, the waves' totals through LDS;
//   4. the list is walked 64 entries a wave-round, so that the lanes of a walking wave all hold a read with an N op -- most reads
//      have none (six in ten are one aligned op), and a wave does not sit through its slowest lane for them; equal keys of a
//      round merge before the insert, as in spl_junction_kernel.
// SPL_DEV_ERR_RANGE: raised by a mapped, placed read of at least spljw::min_ops(min_anchor) ops that HOLDS an N op and whose walk
// leaves the coordinate space -- a rule of the read alone, wherever it lies in its tile.  (spl_junction_kernel refuses every
// mapped read that leaves it, N op or not; those the rule here passes over are refused by the counting pass.)
struct StagedOrGlobalOps { // a listed read's ops: in the stage (LDS) when all of them are there, else in the arrays
    __attribute__((address_space(3))) const uint32_t *lds;
    const uint32_t *glob;
    bool staged;
    __device__ __forceinline__ uint32_t operator()(uint32_t k) const { return staged ? lds[k] : glob[k]; }
};

// XS (spl_junctions, stranded = 3): the strand of a junction is the byte the decode left for its read (spl_bam_set_aux_strand: '+',
// '-' or 0 -> '?'), so the table has up to three rows a junction (spljw::key3_of).  `xs` is an argument of this kernel's own --
// spl_devreads is the range kernels' argument too -- and is read for a LISTED read only, into bits 16.. of the list entry's flag
// word, which the 16-bit FLAG leaves free.  XS = false is the kernel of stranded = 0 / 1 / 2 as it was.
//
// FRAG (spl_junctions_fragments; the rule is spl_junctionfragment_rule.h): a junction whose read has an EARLIER mate that supports
// the same key is a duplicate carry and is not inserted.  mates: the set's mate table, a word a read of the arrays, a segment's
// words holding indexes within the segment; seg_first / seg_n: the set's segments in ascending order of their first read, the
// chunk's own found by a search that is uniform over the workgroup.  Only a LISTED read -- one with an N op -- loads its word of
// the table (its place in the tile rides in bits 24.. of the list entry's flag word); only one whose mate is earlier, walked and of
// its strand loads the mate's POS, FLAG and CIGAR offsets, and walks the mate's ops from the arrays, wherever that read lies, once
// per junction it supports itself.  FRAG = false is the kernel as it was.
template <bool XS, bool FRAG>
__global__ __launch_bounds__(SPL_JTILE) void spl_junction_fused_kernel(const spl_devreads src, int64_t n_rec, int64_t n_ops_total, const spl_layout_chunk *chunks,
                                                                      int stranded, uint32_t min_anchor, uint32_t min_intron, uint32_t max_intron,
                                                                      unsigned long long *keys, uint32_t *vals, uint32_t mask, int32_t *err, const uint8_t *xs,
                                                                      const uint32_t *mates, const int64_t *seg_first, const int64_t *seg_n, uint32_t n_segs)
{
    __shared__ uint32_t s_stage[SPL_JSTAGE];
    __shared__ uint4 s_list[SPL_JTILE];   // {POS + shift, flag, first op, number of ops} of the listed reads
    __shared__ uint32_t s_wave[SPL_JTILE / 64];
    __shared__ uint32_t s_span[2];        // the tile's ops: cigar[s_span[0], s_span[1])
    typedef __attribute__((address_space(3))) uint32_t lds_u32;
    const spl_layout_chunk ch = chunks[blockIdx.x];
    const spljw::Filter filter{min_anchor, min_intron, max_intron};
    const uint32_t need = spljw::min_ops(min_anchor);
    const uint32_t t = threadIdx.x, wave = t >> 6;
    const int lane = (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
    int64_t seg_lo = 0, seg_len = 0; // FRAG: the chunk's segment, reads [seg_lo, seg_lo + seg_len) of the arrays
    if (FRAG && n_segs) {
        uint32_t a = 0, b = n_segs;
        while (a + 1u < b) { const uint32_t mid = a + (b - a) / 2u; if (seg_first[mid] <= ch.lo) a = mid; else b = mid; }
        seg_lo = seg_first[a];
        seg_len = seg_n[a];
    }
    for (uint32_t base = 0; base < ch.n; base += SPL_JTILE) {
        const uint32_t left = ch.n - base, n_tile = left < (uint32_t)SPL_JTILE ? left : (uint32_t)SPL_JTILE;
        const int64_t i = ch.lo + base + t;
        const bool valid = t < n_tile && i < n_rec;
        uint32_t c0 = 0, c1 = 0;
        if (valid) { c0 = src.cig_off[i]; c1 = src.cig_off[i + 1]; }
        if (t == 0) s_span[0] = c0;
        if (t == n_tile - 1u) s_span[1] = c1;
        __syncthreads();
        const uint32_t o_lo = s_span[0], o_hi = s_span[1];
        const uint32_t n_ops = c1 - c0;
        // does any read of the tile have the ops to carry a junction?  (a tile of one-op reads is over here when min_anchor > 0)
        const bool maybe = valid && n_ops >= need;
        const bool any_maybe = __syncthreads_or(maybe) != 0;
        if (!any_maybe) continue; // (uniform over the workgroup; s_span is written again only after the next barrier pair)
        // the tile's ops into the stage: 16 bytes a lane and load, from the 16-byte boundary at or below the first op
        const uint64_t ws = o_lo & ~3u;
        const uint64_t o_end = (uint64_t)o_hi < ws + SPL_JSTAGE ? (uint64_t)o_hi : ws + SPL_JSTAGE;
#pragma unroll
        for (uint32_t q = 0; q < SPL_JSTAGE / (4 * SPL_JTILE); ++q) {
            const uint64_t at = ws + 4ull * (t + q * SPL_JTILE);
            spl_u32x4 v = {0u, 0u, 0u, 0u};
            if (at < o_end) {
                if (at + 4 <= (uint64_t)n_ops_total) v = *(const spl_u32x4 *)(src.cigar + at);
                else {
                    v.x = src.cigar[at];
                    if (at + 1 < (uint64_t)n_ops_total) v.y = src.cigar[at + 1];
                    if (at + 2 < (uint64_t)n_ops_total) v.z = src.cigar[at + 2];
                }
            }
            *(__attribute__((address_space(3))) spl_u32x4 *)((lds_u32 *)s_stage + 4u * (t + q * SPL_JTILE)) = v;
        }
        __syncthreads();
        const uint32_t rel = c0 - (uint32_t)ws;
        const bool staged = (uint64_t)c1 <= ws + SPL_JSTAGE; // all of the read's ops are in LDS
        bool listed = false;
        if (maybe) {
            listed = !staged || n_ops > (uint32_t)SPL_JSCAN;
            if (!listed)
                for (uint32_t k = 0; k < n_ops; ++k) listed = listed || (((const lds_u32 *)s_stage)[rel + k] & 15u) == (uint32_t)SPL_OP_N;
        }
        int32_t pos = 0;
        uint32_t fl = 0;
        if (listed) {
            pos = src.pos[i];
            fl = src.flag[i];
            listed = !(fl & 4u) && pos >= 0; // unmapped and unplaced records carry no junctions
            if (XS && listed) fl |= (uint32_t)xs[i] << 16;
            if (FRAG && listed) fl |= t << 24;
        }
        // the list: lanes with a read to walk, in tile order
        const unsigned long long bal = __ballot(listed);
        const uint32_t before_me = __builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0u));
        if (lane == 0) s_wave[wave] = (uint32_t)__popcll(bal);
        __syncthreads();
        uint32_t wave_base = 0, total = 0;
#pragma unroll
        for (uint32_t q = 0; q < SPL_JTILE / 64; ++q) { const uint32_t c = s_wave[q]; wave_base += q < wave ? c : 0u; total += c; }
        if (listed) s_list[wave_base + before_me] = make_uint4((uint32_t)(pos + ch.shift), fl, c0, n_ops);
        __syncthreads();
        for (uint32_t e0 = wave * 64u; e0 < total; e0 += SPL_JTILE) { // (uniform per wave)
            const uint32_t e = e0 + (uint32_t)lane;
            uint4 rd = make_uint4(0u, 0u, 0u, 0u);
            if (e < total) rd = s_list[e];
            const uint32_t r_ops = e < total ? rd.w : 0u;
            unsigned long long sbit;
            if (XS) { const uint32_t x = FRAG ? (rd.y >> 16) & 0xffu : rd.y >> 16; sbit = x == (uint32_t)'+' ? 0ull : x == (uint32_t)'-' ? 1ull : 2ull; }
            else sbit = (stranded && spl_read_strand(FRAG ? rd.y & 0xffffu : rd.y, stranded) == (uint8_t)'-') ? 1ull : 0ull;
            bool m_has = false; // FRAG: the read has an earlier mate that is walked and of its strand: ops cigar[m0, m0 + m_ops), from m_p
            uint32_t m0 = 0, m_ops = 0;
            int32_t m_p = 0;
            if (FRAG && e < total) {
                const int64_t r = ch.lo + (int64_t)base + (int64_t)(rd.y >> 24) - seg_lo; // the read's index within its segment
                const int64_t m = (r >= 0 && r < seg_len) ? spljf::earlier_mate(mates + seg_lo, seg_len, r) : -1;
                if (m >= 0) {
                    const int64_t mi = seg_lo + m; // (< seg_lo + seg_len <= n_rec: the launcher's check)
                    const uint32_t m_fl = src.flag[mi];
                    const int32_t m_pos = src.pos[mi];
                    uint32_t a = src.cig_off[mi], b = src.cig_off[mi + 1];
                    if (b < a || (int64_t)b > n_ops_total) b = a; // (offsets of the arrays' own ops: said for the memory's sake)
                    m0 = a; m_ops = b - a; m_p = m_pos + ch.shift;
                    m_has = spljf::walked(m_fl, (int64_t)m_pos) && spljf::strand_code(m_fl, XS ? (uint32_t)xs[mi] : 0u, stranded) == (uint32_t)sbit;
                }
            }
            StagedOrGlobalOps ops;
            ops.staged = (uint64_t)rd.z + rd.w <= ws + SPL_JSTAGE;
            ops.lds = (const lds_u32 *)s_stage + (ops.staged ? rd.z - (uint32_t)ws : 0u);
            ops.glob = src.cigar + rd.z;
            spljw::Walk w;
            w.begin((int32_t)rd.x);
            while (__any(w.k < r_ops)) {
                spljw::Junction j;
                j.passes = false; j.l = j.r = 0; j.anchor_left = j.anchor_right = 0;
                bool have = false;
                while (!have && spljw::next(w, ops, r_ops, filter, j)) have = j.passes;
                if (w.range_error) {
                    // refused only where the read HAS an N op: what is listed without looking (ops beyond the stage, more than
                    // SPL_JSCAN of them) must not be refused for where it happens to lie -- the rule is the reads', not the tiles'
                    bool has_n = false;
                    for (uint32_t k2 = 0; k2 < r_ops; ++k2) has_n = has_n || (ops(k2) & 15u) == (uint32_t)SPL_OP_N;
                    if (has_n) atomicOr(err, SPL_DEV_ERR_RANGE);
                    w.range_error = false;
                }
                if (XS && have && !spljw::key3_fits(j.l, j.r)) { atomicOr(err, SPL_DEV_ERR_RANGE); have = false; }
                if (FRAG && have && m_has && spljf::carries(spl_ops_ptr{src.cigar + m0}, m_ops, m_p, filter, j.l, j.r)) have = false; // a duplicate carry
                junction_merge_insert(have, have ? (XS ? spljw::key3_of(j.l, j.r, sbit) : spljw::key_of(j.l, j.r, sbit)) : ~0ull, j.anchor_left, j.anchor_right, lane, keys, vals, mask,
                                      err);
            }
        }
        __syncthreads(); // (the stage and the list are the next tile's)
    }
}

// What sizes the fused kernel's table: the N ops of the set's chunks whose length passes the intron filter (the anchors are
// not looked at: an upper bound of the inserts, from one coalesced pass over the chunks' stretch of the CIGAR array).
__global__ __launch_bounds__(256) void spl_junction_count_kernel(const uint32_t *cigar, const spl_layout_chunk *chunks, uint32_t min_intron, uint32_t max_intron,
                                                                 unsigned long long *n_out)
{
    const spl_layout_chunk ch = chunks[blockIdx.x];
    uint32_t mine = 0;
    for (uint64_t at = (uint64_t)ch.o_lo + threadIdx.x; at < (uint64_t)ch.o_hi; at += 256u) {
        const uint32_t op = cigar[at], d = op >> 4;
        mine += ((op & 15u) == (uint32_t)SPL_OP_N && d >= min_intron && (max_intron == 0u || d <= max_intron)) ? 1u : 0u;
    }
    for (int off = 32; off > 0; off >>= 1) mine += (uint32_t)__shfl_xor((int)mine, off);
    if ((threadIdx.x & 63u) == 0u && mine) atomicAdd(n_out, (unsigned long long)mine);
}

// Non-empty slots -> dense arrays (order arbitrary; the host sorts).
__global__ __launch_bounds__(256) void spl_junction_fused_compact_kernel(const unsigned long long *keys, const uint32_t *vals, uint32_t n_slots,
                                                                   unsigned long long *out_keys, uint32_t *out_vals, uint32_t *n_out)
{
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    if (j >= n_slots) return;
    const unsigned long long k = keys[j];
    if (k == ~0ull) return;
    const uint32_t at = atomicAdd(n_out, 1u);
    out_keys[at] = k;
    out_vals[3u * at] = vals[3u * j];
    out_vals[3u * at + 1u] = vals[3u * j + 1u];
    out_vals[3u * at + 2u] = vals[3u * j + 2u];
}

} // namespace

// ---- launchers (called from spl_capi.cpp through spl_junction_fused.h) ------------------------------------

// The N ops that pass the intron filter into *n_count: what the caller sizes the table by.
extern "C" int spl_dev_launch_junctions_count(const spl_devreads *src, const spl_layout_chunk *chunks, uint32_t n_chunks, uint32_t min_intron,
                                              uint32_t max_intron, unsigned long long *n_count, void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    const hipError_t e = hipMemsetAsync(n_count, 0, 8, st);
    if (e != hipSuccess) return (int)e;
    if (n_chunks > 0)
        hipLaunchKernelGGL(spl_junction_count_kernel, dim3(n_chunks), dim3(256), 0, st, src->cigar, chunks, min_intron, max_intron, n_count);
    return (int)hipGetLastError();
}

// The table of n_slots slots cleared, filled and compacted, like spl_dev_launch_junctions does it for packed records.
extern "C" int spl_dev_launch_junctions_fused(const spl_devreads *src, int64_t n_rec, int64_t n_ops, const spl_layout_chunk *chunks, uint32_t n_chunks,
                                              int stranded, uint32_t min_anchor, uint32_t min_intron, uint32_t max_intron,
                                              unsigned long long *keys, uint32_t *vals, uint32_t n_slots, unsigned long long *out_keys,
                                              uint32_t *out_vals, uint32_t *n_out, int32_t *err, const uint8_t *xs, void *stream)
{
    if ((stranded == 3) != (xs != nullptr)) return (int)hipErrorInvalidValue; // (mode 3 and the reads' strand bytes come together)
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(keys, 0xff, (size_t)n_slots * 8, st);
    if (e == hipSuccess) e = hipMemsetAsync(vals, 0, (size_t)n_slots * 12, st);
    if (e == hipSuccess) e = hipMemsetAsync(n_out, 0, 4, st);
    if (e == hipSuccess) e = hipMemsetAsync(err, 0, 4, st);
    if (e != hipSuccess) return (int)e;
    if (n_chunks > 0 && xs)
        hipLaunchKernelGGL((spl_junction_fused_kernel<true, false>), dim3(n_chunks), dim3(SPL_JTILE), 0, st, *src, n_rec, n_ops, chunks, stranded, min_anchor, min_intron,
                           max_intron, keys, vals, n_slots - 1u, err, xs, (const uint32_t *)nullptr, (const int64_t *)nullptr, (const int64_t *)nullptr, 0u);
    else if (n_chunks > 0)
        hipLaunchKernelGGL((spl_junction_fused_kernel<false, false>), dim3(n_chunks), dim3(SPL_JTILE), 0, st, *src, n_rec, n_ops, chunks, stranded, min_anchor, min_intron,
                           max_intron, keys, vals, n_slots - 1u, err, (const uint8_t *)nullptr, (const uint32_t *)nullptr, (const int64_t *)nullptr, (const int64_t *)nullptr, 0u);
    hipLaunchKernelGGL(spl_junction_fused_compact_kernel, dim3((n_slots + 255u) / 256u), dim3(256), 0, st, keys, vals, n_slots, out_keys, out_vals, n_out);
    return (int)hipGetLastError();
}

// The same per fragment: mates (n_rec words), and the set's n_segs >= 1 segments, ascending in seg_first (device memory), every one
// inside [0, n_rec): the caller's check.
extern "C" int spl_dev_launch_junctions_fused_fragments(const spl_devreads *src, int64_t n_rec, int64_t n_ops, const spl_layout_chunk *chunks, uint32_t n_chunks, int stranded,
                                                        uint32_t min_anchor, uint32_t min_intron, uint32_t max_intron, unsigned long long *keys, uint32_t *vals, uint32_t n_slots,
                                                        unsigned long long *out_keys, uint32_t *out_vals, uint32_t *n_out, int32_t *err, const uint8_t *xs, const uint32_t *mates,
                                                        const int64_t *seg_first, const int64_t *seg_n, uint32_t n_segs, void *stream)
{
    if ((stranded == 3) != (xs != nullptr) || !mates || !seg_first || !seg_n || n_segs < 1u) return (int)hipErrorInvalidValue;
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(keys, 0xff, (size_t)n_slots * 8, st);
    if (e == hipSuccess) e = hipMemsetAsync(vals, 0, (size_t)n_slots * 12, st);
    if (e == hipSuccess) e = hipMemsetAsync(n_out, 0, 4, st);
    if (e == hipSuccess) e = hipMemsetAsync(err, 0, 4, st);
    if (e != hipSuccess) return (int)e;
    if (n_chunks > 0 && xs)
        hipLaunchKernelGGL((spl_junction_fused_kernel<true, true>), dim3(n_chunks), dim3(SPL_JTILE), 0, st, *src, n_rec, n_ops, chunks, stranded, min_anchor, min_intron, max_intron, keys,
                           vals, n_slots - 1u, err, xs, mates, seg_first, seg_n, n_segs);
    else if (n_chunks > 0)
        hipLaunchKernelGGL((spl_junction_fused_kernel<false, true>), dim3(n_chunks), dim3(SPL_JTILE), 0, st, *src, n_rec, n_ops, chunks, stranded, min_anchor, min_intron, max_intron, keys,
                           vals, n_slots - 1u, err, (const uint8_t *)nullptr, mates, seg_first, seg_n, n_segs);
    hipLaunchKernelGGL(spl_junction_fused_compact_kernel, dim3((n_slots + 255u) / 256u), dim3(256), 0, st, keys, vals, n_slots, out_keys, out_vals, n_out);
    return (int)hipGetLastError();
}
