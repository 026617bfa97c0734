// spl_devpack.hip -- the packer of spl_pack.h on the device: BAM-native reads that are in device memory (the device decoder's
// arrays, spl_bam_decode_device; a caller's arrays brought up as they are, spl_soa_upload) -> the chunked, class-partitioned
// record layout the counting kernels read.  The host packer's classification (splrec::classify_ops) in fewer instructions (splrec::classify_lean: held to it on the host), same records.
//
// ONE launch per read set, one workgroup per chunk, every read fetched and classified ONCE (round 4: three launches per
// reference, every read fetched and classified twice, 5.4 ms per 200 M reads against 0.8 ms of counting):
//   * a thread takes FOUR consecutive reads: POS and the CIGAR offsets are one aligned 16-byte load each, the flags 8 bytes --
//     the chunks are cells of a grid over the arrays' indexes, so that this holds wherever a reference begins;
//   * the chunk's CIGAR ops are one contiguous stretch of the array: the workgroup stages it in LDS with coalesced 16-byte
//     loads and the classifier reads ops out of LDS (a stretch longer than the stage -- long-read CIGARs -- is read from
//     memory beyond it);
//   * the four records stay in registers while the workgroup counts: a read's rank in its run comes from a prefix sum over the
//     lanes' per-run counts, the waves' totals through LDS -- the runs keep file order;
//   * the chunk writes into a record slot of its own (worst-case size), so no workgroup waits for another's count; WIDE reads'
//     ops are not copied at all: their index points into the array they came from, which the read set keeps alive;
//   * the chunk's descriptor (spl_chunk_meta) is written by the kernel: nothing comes down to the host.
// The range kernel's chunk order (XCD share by XCD share, longest first) is made by spl_chunk_slots_kernel BEFORE the layout, from
// cost estimates that need the chunks' numbers of reads and ops only: layout -> range with nothing between.  A fused read set
// gets its chunks' descriptors from the same launch, written once, where the range kernel reads them.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <stdint.h>

#include "spl_pack.h"
#include "spl_devpack.h"
#include "spl_layout_tile.h"

using namespace spllay;

// Where chunk number i of segment s lies in the arrays: reads [lo, hi) of the cell that begins at c0 (chunk = reads per chunk, a
// power of two: sh = its log2).
__device__ __forceinline__ void chunk_reads(const spl_layout_seg &s, uint32_t i, uint32_t sh, int64_t &c0, int64_t &lo, int64_t &hi)
{
    c0 = ((s.first >> sh) + (int64_t)i) << sh;
    const int64_t c1 = c0 + ((int64_t)1 << sh), end = s.first + s.n_reads;
    lo = s.first > c0 ? s.first : c0;
    hi = end < c1 ? end : c1;
}

// What a chunk will cost the range kernel, roughly -- from its numbers of reads and ops alone (a simple read is one op and weighs
// 2, a once-spliced one three and 5, a twice-spliced one five and 9: (3 ops + reads) / 2), so that the chunk order can be made
// BEFORE the records are and nothing stands between the layout kernel and the range kernel.
__device__ __forceinline__ uint32_t chunk_cost(uint32_t ops, uint32_t reads) { return (3u * ops + reads) / 2u; }

// A thread per chunk of the launch: which segment it is of (a bisection over the segments' first chunks), where its reads and
// its ops lie, and its cost estimate.  For the groups of a read set that is not fused (spl_chunk_slots_kernel<true> does the same
// for a fused one): such a set's chunks may come from several groups and from the host, so their order is made from cost[].
__global__ __launch_bounds__(256) void spl_layout_map_kernel(const spl_devreads src, const spl_layout_seg *segs, uint32_t n_segs, uint32_t n_chunks, uint32_t chunk,
                                                             spl_layout_chunk *chunks, uint32_t *cost)
{
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k >= n_chunks) return;
    uint32_t a = 0, b = n_segs; // the last segment whose first chunk is <= k
    while (b - a > 1u) {
        const uint32_t mid = (a + b) >> 1;
        if (segs[mid].dev0 <= k) a = mid; else b = mid;
    }
    const spl_layout_seg s = segs[a];
    int64_t c0, hi;
    spl_layout_chunk c;
    chunk_reads(s, k - s.dev0, (uint32_t)__builtin_ctz(chunk), c0, c.lo, hi);
    c.n = (uint32_t)(hi - c.lo);
    c.o_lo = src.cig_off[c.lo]; c.o_hi = src.cig_off[hi]; c.seg_op0 = src.cig_off[s.first];
    c.shift = s.shift;
    c.flat = s.chunk0 + (k - s.dev0);
    chunks[k] = c;
    cost[c.flat] = chunk_cost(c.o_hi - c.o_lo, c.n);
}

template <int C>
__global__ __launch_bounds__(C / 4) __attribute__((amdgpu_waves_per_eu(8, 8))) void spl_layout_kernel(const spl_layout_params p)
{
    constexpr uint32_t T = C / 4, NW = T / 64, STAGE = 4 * C;
    __shared__ uint32_t s_ops[STAGE];
    __shared__ uint32_t s_cnt[NW][2];
    __shared__ int32_t s_first; // POS of the chunk's first read in file order: base of the range kernel's LDS window
    const uint32_t k = blockIdx.x;
    const spl_layout_chunk ch = p.chunks[k]; // (wave-uniform: one scalar load)
    uint32_t n[4];
    layout_tile<C>(p.src, p.n_rec, p.n_ops, ch, (lay_lds_w32 *)s_ops, (lay_lds_w32 *)&s_cnt[0][0], (lay_lds_i32 *)&s_first, RecordsInMemory{p.rec_base, SPL_LAYOUT_SLOT(C)}, n);
    if (threadIdx.x == 0) {
        uint8_t *const rec = p.rec_base + (size_t)k * SPL_LAYOUT_SLOT(C);
        spl_chunk_meta m;
        m.rec = (uint64_t)(uintptr_t)rec;
        m.wide = (uint64_t)(uintptr_t)(p.src.cigar + ch.seg_op0);
        m.shift = ch.shift;
        m.first_pos = s_first;
        m.n[0] = (uint16_t)n[0]; m.n[1] = (uint16_t)n[1]; m.n[2] = (uint16_t)n[2]; m.n[3] = (uint16_t)n[3];
        p.meta[ch.flat] = m;
    }
}

// The range kernel's workgroup b works on slot (b & 7) * per + (b >> 3): XCD x -- the hardware deals workgroups round-robin over
// the eight -- walks slots [x * per, (x + 1) * per).  WHICH chunks an XCD gets decides when it is done, and the launch ends with
// the slowest: the chunks are dealt to the XCDs in blocks of 8 consecutive chunks, round-robin (every stretch of the genome is
// spread over all eight; neighbouring chunks, which share lines of the position index, still go to one L2 together), and inside
// an XCD's share they go longest first by the cost estimate: by its key cost / 16 (at most 4095), equal keys in the order of the
// chunks' numbers.  Slots past a share's chunks hold 0xffffffff.
//
// A thread per slot, 256 of them a workgroup, every workgroup of ONE share (workgroup b: share b & 7, its members 256 (b >> 3) on;
// member e of share x is chunk (x + 8 (e / 8)) 8 + e % 8, so the members that are chunks at all are the share's first ones).  No
// sort, and nothing one workgroup waits for of another: a member's slot is the number of members that go before it, and every
// workgroup counts that for its own 256 from the costs of ALL members of its share -- a histogram over the 4096 keys in LDS, its
// prefix sums, and for equal keys the members before the workgroup's (the histogram's state when only they have been added) and
// before the thread within the workgroup (256 keys in LDS).  The costs of a share are strided loads that do not depend on one
// another, from L2 once the share's first workgroup has had them.
// FUSED (a read set whose chunks all come from ONE group of device arrays): the costs come from the segments and the arrays'
// CIGAR offsets, and a thread also makes its chunk's two descriptors -- the 32-byte one of the junction and literal paths
// (chunks[k]) and the fused counting kernel's 64 bytes, written ONCE, to the slot where that kernel's workgroup loads them.  Not
// FUSED: the costs are cost[] as spl_layout_map_kernel and the host packer left them, and the order is all that is written.
#define SPL_SLOTS_SEGS_LDS 256u // segments that are looked up in LDS (more: in memory)
template <bool FUSED>
__global__ __launch_bounds__(256) void spl_chunk_slots_kernel(const spl_devreads src, const spl_layout_seg *segs, uint32_t n_segs, const uint32_t *cost, uint32_t n, uint32_t per,
                                                              uint32_t chunk, spl_layout_chunk *chunks, uint32_t *order, spl_fused_slot *slots)
{
    constexpr uint32_t NB = 4096, T = 256, U = 4, NONE = 0xffffffffu;
    __shared__ alignas(16) uint32_t s_hist[NB];
    __shared__ alignas(16) uint32_t s_key[T];
    __shared__ uint32_t s_wave[T / 64];
    __shared__ spl_layout_seg s_segs[FUSED ? SPL_SLOTS_SEGS_LDS : 1u];
    const uint32_t x = blockIdx.x & 7u, t = threadIdx.x, e0 = (blockIdx.x >> 3) * T, e = e0 + t;
    const uint32_t sh = (uint32_t)__builtin_ctz(chunk);
    const bool staged = n_segs <= SPL_SLOTS_SEGS_LDS;
    for (uint32_t b = t; b < NB; b += T) s_hist[b] = 0;
    if (FUSED && staged)
        for (uint32_t i = t; i < n_segs; i += T) s_segs[i] = segs[i];
    __syncthreads();
    auto chunk_of = [&](uint32_t f) { return (x + 8u * (f >> 3)) * 8u + (f & 7u); };
    auto key_of = [&](uint32_t c) { const uint32_t q = c >> 4; return NB - 1u - (q < NB ? q : NB - 1u); };
    // the segment of flat chunk j: the last one whose first chunk is <= j (a segment without reads has no chunks: never the last)
    auto seg_of = [&](uint32_t j) {
        uint32_t a = 0, b = n_segs;
        while (b - a > 1u) {
            const uint32_t mid = (a + b) >> 1;
            if ((staged ? s_segs[mid].chunk0 : segs[mid].chunk0) <= j) a = mid; else b = mid;
        }
        return staged ? s_segs[a] : segs[a];
    };
    // the keys of members [f0, f1) of the share into the histogram: U a thread at a time, their loads in flight together
    auto tally = [&](uint32_t f0, uint32_t f1) {
        for (uint32_t f = f0 + t; f < f1; f += U * T) {
            uint32_t c[U];
            bool is[U];
            if constexpr (FUSED) {
                uint32_t o_lo[U], o_hi[U], reads[U];
#pragma unroll
                for (uint32_t u = 0; u < U; ++u) {
                    const uint32_t j = chunk_of(f + u * T);
                    is[u] = f + u * T < f1 && j < n;
                    o_lo[u] = o_hi[u] = reads[u] = 0;
                    if (is[u]) {
                        const spl_layout_seg s = seg_of(j);
                        int64_t c0, lo, hi;
                        chunk_reads(s, j - s.chunk0, sh, c0, lo, hi);
                        o_lo[u] = src.cig_off[lo]; o_hi[u] = src.cig_off[hi]; reads[u] = (uint32_t)(hi - lo);
                    }
                }
#pragma unroll
                for (uint32_t u = 0; u < U; ++u) c[u] = chunk_cost(o_hi[u] - o_lo[u], reads[u]);
            } else {
#pragma unroll
                for (uint32_t u = 0; u < U; ++u) {
                    const uint32_t j = chunk_of(f + u * T);
                    is[u] = f + u * T < f1 && j < n;
                    c[u] = is[u] ? cost[j] : 0u;
                }
            }
#pragma unroll
            for (uint32_t u = 0; u < U; ++u)
                if (is[u]) atomicAdd(&s_hist[key_of(c[u])], 1u);
        }
    };
    // the thread's own member
    const uint32_t j = chunk_of(e);
    const bool is_chunk = e < per && j < n;
    uint32_t key = NONE;
    spl_layout_chunk c = {};
    spl_fused_slot fs = {};
    uint32_t k = 0; // its chunk's index among the chunks of the group
    if (is_chunk) {
        if constexpr (FUSED) {
            const spl_layout_seg s = seg_of(j);
            int64_t c0, hi;
            chunk_reads(s, j - s.chunk0, sh, c0, c.lo, hi);
            k = s.dev0 + (j - s.chunk0);
            c.n = (uint32_t)(hi - c.lo);
            c.o_lo = src.cig_off[c.lo]; c.o_hi = src.cig_off[hi]; c.seg_op0 = src.cig_off[s.first];
            c.shift = s.shift;
            c.flat = j;
            // the fused counting kernel's view of the chunk: the offsets at its tiles' boundaries (cell c0's tile q begins at c0 + q TILE,
            // clamped to the chunk's reads) and its first POS -- a load of pos and at most three more of cig_off here, a thread per
            // chunk, instead of two dependent trips in front of every workgroup's first tile there
            fs.lo = c.lo; fs.chunk = c.flat; fs.n = c.n; fs.shift = c.shift; fs.seg_op0 = c.seg_op0;
            fs.pos0 = c.n ? src.pos[c.lo] : 0;
            fs.unused0 = 0; fs.unused1[0] = fs.unused1[1] = fs.unused1[2] = 0;
            const uint32_t tiles = chunk >> SPL_TILE_FUSED_SHIFT; // (0 for a chunk size the fused pass does not take: boundaries o_lo, o_hi ...)
#pragma unroll
            for (uint32_t q = 0; q <= SPL_FUSED_TILES_MAX; ++q) {
                int64_t i = c0 + (int64_t)q * SPL_TILE_FUSED;
                i = i < c.lo ? c.lo : (i > hi ? hi : i);
                fs.ob[q] = q == 0u ? c.o_lo : (q >= tiles ? c.o_hi : src.cig_off[i]);
            }
            key = key_of(chunk_cost(c.o_hi - c.o_lo, c.n));
        } else
            key = key_of(cost[j]);
    }
    s_key[t] = key;
    tally(0u, e0); // the members before this workgroup's ...
    __syncthreads();
    uint32_t before = is_chunk ? s_hist[key] : 0u; // ... of them, those of the thread's key go before it
    __syncthreads();
    if (is_chunk) atomicAdd(&s_hist[key], 1u);
    tally(e0 + T < per ? e0 + T : per, per);
    // of the workgroup's own members, the earlier ones of the same key do as well (a wave looks at the keys up to its last lane's)
    for (uint32_t u = 0; u < (t | 63u) + 1u; u += 4u) {
        const uint4 q = *(const uint4 *)&s_key[u];
        before += (q.x == key && u < t) + (q.y == key && u + 1u < t) + (q.z == key && u + 2u < t) + (q.w == key && u + 3u < t);
    }
    __syncthreads();
    // exclusive prefix sums over the keys: sixteen per thread, the threads' sums over the wave, the waves' through LDS
    uint4 h[4];
    uint32_t sum = 0;
#pragma unroll
    for (uint32_t i = 0; i < 4u; ++i) {
        h[i] = *(const uint4 *)&s_hist[16u * t + 4u * i];
        sum += h[i].x + h[i].y + h[i].z + h[i].w;
    }
    uint32_t incl = sum;
#pragma unroll
    for (uint32_t s = 1; s < 64u; s <<= 1) {
        const uint32_t up = (uint32_t)__shfl_up((int)incl, s, 64);
        if ((t & 63u) >= s) incl += up;
    }
    if ((t & 63u) == 63u) s_wave[t >> 6] = incl;
    __syncthreads();
    uint32_t run = incl - sum;
    for (uint32_t w = 0; w < (t >> 6); ++w) run += s_wave[w];
#pragma unroll
    for (uint32_t i = 0; i < 4u; ++i) {
        uint4 o;
        o.x = run; o.y = run + h[i].x; o.z = o.y + h[i].y; o.w = o.z + h[i].z;
        run = o.w + h[i].w;
        *(uint4 *)&s_hist[16u * t + 4u * i] = o;
    }
    __syncthreads();
    if (e >= per) return;
    const size_t slot = (size_t)x * per + (is_chunk ? s_hist[key] + before : e); // (the members that are no chunks are the share's last: their own places)
    if (is_chunk) {
        order[slot] = j;
        if constexpr (FUSED) {
            chunks[k] = c;
            slots[slot] = fs;
        }
    } else {
        order[slot] = NONE;
        if constexpr (FUSED) {
            uint4 *to = (uint4 *)(slots + slot);
            to[0] = make_uint4(0u, 0u, SPL_SLOT_EMPTY, 0u); // (lo, lo, chunk, n)
            to[1] = to[2] = to[3] = make_uint4(0u, 0u, 0u, 0u);
        }
    }
}

extern "C" int spl_dev_launch_layout_map(const spl_devreads *src, const spl_layout_seg *segs, uint32_t n_segs, uint32_t n_chunks, uint32_t chunk, spl_layout_chunk *chunks,
                                         uint32_t *cost, void *stream)
{
    if (!n_segs || !n_chunks) return 0;
    if (chunk & (chunk - 1u)) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(spl_layout_map_kernel, dim3((n_chunks + 255u) / 256u), dim3(256), 0, (hipStream_t)stream, *src, segs, n_segs, n_chunks, chunk, chunks, cost);
    return (int)hipGetLastError();
}

extern "C" int spl_dev_launch_layout(const spl_layout_params *p, uint32_t n_dev_chunks, uint32_t chunk, void *stream, void *ev_start, void *ev_stop)
{
    if (!n_dev_chunks) return 0;
    hipStream_t st = (hipStream_t)stream;
    hipEvent_t e0 = (hipEvent_t)ev_start, e1 = (hipEvent_t)ev_stop;
    if (chunk == (uint32_t)SPL_CHUNK) hipExtLaunchKernelGGL(spl_layout_kernel<SPL_CHUNK>, dim3(n_dev_chunks), dim3(SPL_CHUNK / 4), 0, st, e0, e1, 0, *p);
    else if (chunk == (uint32_t)SPL_CHUNK_BIG) hipExtLaunchKernelGGL(spl_layout_kernel<SPL_CHUNK_BIG>, dim3(n_dev_chunks), dim3(SPL_CHUNK_BIG / 4), 0, st, e0, e1, 0, *p);
    else return (int)hipErrorInvalidValue;
    return (int)hipGetLastError();
}

// (a workgroup per 256 slots of a share, the eight shares' workgroups interleaved: workgroup b is of share b & 7)
static dim3 chunk_slots_grid(uint32_t n_chunks) { return dim3(8u * ((spl_order_per(n_chunks) + 255u) / 256u)); }

extern "C" int spl_dev_launch_chunk_slots(const spl_devreads *src, const spl_layout_seg *segs, uint32_t n_segs, uint32_t n_chunks, uint32_t chunk, spl_layout_chunk *chunks,
                                          uint32_t *order, spl_fused_slot *slots, void *stream)
{
    if (!n_segs || !n_chunks) return 0;
    if ((chunk & (chunk - 1u)) || n_chunks > SPL_ORDER_CHUNKS_MAX) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(spl_chunk_slots_kernel<true>, chunk_slots_grid(n_chunks), dim3(256), 0, (hipStream_t)stream, *src, segs, n_segs, (const uint32_t *)nullptr, n_chunks,
                       spl_order_per(n_chunks), chunk, chunks, order, slots);
    return (int)hipGetLastError();
}

extern "C" int spl_dev_launch_chunk_order(const uint32_t *cost, uint32_t n_chunks, uint32_t *order, void *stream)
{
    if (!n_chunks) return 0;
    if (n_chunks > SPL_ORDER_CHUNKS_MAX) return (int)hipErrorInvalidValue;
    // (the estimate, (3 ops + reads) / 2, has no bound of its own for long-read chunks: the kernel's key_of clamps it to its 4096 keys)
    hipLaunchKernelGGL(spl_chunk_slots_kernel<false>, chunk_slots_grid(n_chunks), dim3(256), 0, (hipStream_t)stream, spl_devreads{}, (const spl_layout_seg *)nullptr, 0u, cost,
                       n_chunks, spl_order_per(n_chunks), 1u, (spl_layout_chunk *)nullptr, order, (spl_fused_slot *)nullptr);
    return (int)hipGetLastError();
}
