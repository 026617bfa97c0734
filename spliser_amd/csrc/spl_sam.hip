// spl_sam.hip -- SAM text parsed on the device (spl_sam.h has the interface and the method, spl_sam_line.h the rule).
//
// Bytes moved, per window of B bytes holding L lines: the two line-start launches read B each (the second from L2 / the Infinity
// Cache where the window fits) and write 4 L; the scan and the extraction read the lines' bytes again through the lanes' own
// byte loops -- neighbouring lanes read neighbouring lines, a wave's loads fall into a few dozen cache lines at a time -- and
// write 12 L and the arrays.  Four passes over text that came over a link seven times slower than the memory it lies in: nothing
// here is fused for its own sake.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "spl_sam.h"
#include "spl_sam_line.h"
#include "spl_flagstat.h"
#include "spl_wave.h"

namespace {

// bit j = byte j of the word is '\n' (exact: no borrow from a neighbouring byte)
__device__ __forceinline__ uint32_t newline_bits(uint32_t x)
{
    const uint32_t t = x ^ 0x0a0a0a0au;
    const uint32_t z = ~(((t & 0x7f7f7f7fu) + 0x7f7f7f7fu) | t | 0x7f7f7f7fu); // 0x80 in every byte of t that is zero
    return (z >> 7 & 1u) | (z >> 14 & 2u) | (z >> 21 & 4u) | (z >> 28 & 8u);
}

// The line starts among the sixteen bytes at `at` (a multiple of 16, at < hi16 = hi rounded up to 16): bit j = a line begins at byte
// at + j.  One begins at lo, and behind every '\n' at lo <= p with p + 1 < hi.  before: the byte in front of the sixteen is a '\n'
// -- from the lane below; carry for lane 0.  -> the starts, and whether the sixteenth byte is a '\n' (for the lane above).
__device__ __forceinline__ uint32_t line_start_bits(const uint8_t *text, uint64_t at, uint64_t lo, uint64_t hi, uint64_t hi16, uint32_t carry, uint32_t &last_out)
{
    uint32_t nl = 0;
    if (at < hi16) {
        const uint4 w = *(const uint4 *)(text + at);
        nl = newline_bits(w.x) | newline_bits(w.y) << 4 | newline_bits(w.z) << 8 | newline_bits(w.w) << 12;
    }
    const uint32_t last = nl >> 15 & 1u;
    uint32_t before = wv::shfl_up(last, 1);
    if (wv::lane() == 0) before = carry;
    uint32_t starts = (nl << 1 | before) & 0xffffu;
    // only bytes of [lo, hi) begin a line; lo itself does whatever stands in front of it
    uint32_t valid = 0xffffu;
    if (at < lo) valid = lo - at >= 16u ? 0u : valid & ~((1u << (uint32_t)(lo - at)) - 1u);
    if (at + 16u > hi) valid = at >= hi ? 0u : valid & ((1u << (uint32_t)(hi - at)) - 1u);
    starts &= valid;
    if (lo >= at && lo < at + 16u && lo < hi) starts |= 1u << (uint32_t)(lo - at);
    last_out = last;
    return starts;
}

constexpr uint32_t ROUNDS = SPL_SAM_CHUNK / (64u * 16u);

template <bool FILL>
__device__ __forceinline__ void line_starts(const uint8_t *text, uint64_t lo, uint64_t hi, uint32_t *chunk_count, const uint32_t *chunk_end, uint32_t *line_start)
{
    const uint64_t base = lo & ~(uint64_t)15, hi16 = (hi + 15u) & ~(uint64_t)15;
    const uint32_t k = blockIdx.x, l = wv::lane();
    const uint64_t chunk = base + (uint64_t)k * SPL_SAM_CHUNK;
    // the byte in front of the chunk (the chunk before holds it; in front of lo nothing counts)
    uint32_t carry = chunk > lo ? (text[chunk - 1] == '\n' ? 1u : 0u) : 0u;
    uint32_t total = 0;
    uint32_t out = FILL ? (k ? chunk_end[k - 1] : 0u) : 0u;
    for (uint32_t r = 0; r < ROUNDS; ++r) {
        const uint64_t at = chunk + (uint64_t)r * 1024u + (uint64_t)l * 16u;
        uint32_t last = 0;
        const uint32_t starts = line_start_bits(text, at, lo, hi, hi16, carry, last);
        carry = wv::shfl(last, 63);
        const uint32_t n = (uint32_t)__popc(starts);
        if (FILL) {
            const uint32_t incl = wv::scan_add(n);
            uint32_t o = out + incl - n;
            for (uint32_t m = starts; m; m &= m - 1u) line_start[o++] = (uint32_t)(at - base) + (uint32_t)__ffs((int)m) - 1u;
            out += wv::shfl(incl, 63);
        } else
            total += n;
    }
    if (!FILL) {
        const uint32_t incl = wv::scan_add(total);
        if (l == 63) chunk_count[k] = incl;
    }
}

__global__ __launch_bounds__(64) void spl_sam_line_count_kernel(const uint8_t *text, uint64_t lo, uint64_t hi, uint32_t *chunk_count)
{
    line_starts<false>(text, lo, hi, chunk_count, nullptr, nullptr);
}

__global__ __launch_bounds__(64) void spl_sam_line_fill_kernel(const uint8_t *text, uint64_t lo, uint64_t hi, const uint32_t *chunk_end, uint32_t *line_start)
{
    line_starts<true>(text, lo, hi, nullptr, chunk_end, line_start);
}

__device__ __forceinline__ void line_span(const uint8_t *text, uint64_t base, const uint32_t *line_start, uint32_t n_lines, uint64_t last_end, uint32_t i, const uint8_t *&p,
                                          const uint8_t *&end)
{
    p = text + base + line_start[i];
    end = i + 1u < n_lines ? text + base + line_start[i + 1u] - 1 : text + last_end;
}

__global__ __launch_bounds__(SPL_SAM_SCAN_LANES) void spl_sam_scan_kernel(const uint8_t *text, uint64_t base, const uint32_t *line_start, uint32_t n_lines, uint64_t last_end,
                                                                           spl_sam_names names, spl_bam_filter filter, uint32_t want_xs, uint32_t *kept, uint32_t *n_ops,
                                                                           int32_t *line_tid, uint32_t *fstat, spl_sam_counts *counts)
{
    const uint32_t i = blockIdx.x * SPL_SAM_SCAN_LANES + threadIdx.x;
    const bool live = i < n_lines;
    spl_sam_line ln;
    ln.reason = SPL_SAM_OK;
    ln.verdict = SPL_BAM_KEPT;
    ln.placed = 0;
    ln.flag = ln.mapq = ln.n_ops = 0;
    ln.tid = ln.next_tid = -1;
    if (live) {
        const uint8_t *p, *end;
        line_span(text, base, line_start, n_lines, last_end, i, p, end);
        spl_sam_parse_line(p, end, names, -1, filter, want_xs != 0u, &ln);
        const bool ok = ln.reason == SPL_SAM_OK, take = ok && ln.placed && ln.verdict == SPL_BAM_KEPT;
        kept[i] = take ? 1u : 0u;
        n_ops[i] = take ? ln.n_ops : 0u;
        line_tid[i] = ok ? ln.tid : -1;
        if (!ok) atomicMin(&counts->first_bad, (unsigned long long)i << 8 | ln.reason);
    }
    const bool ok = live && ln.reason == SPL_SAM_OK;
    // the wave's sums (every lane of the wave gets here: the launch is whole workgroups)
    const uint32_t by_flags = wv::popc64(wv::ballot(ok && ln.placed && ln.verdict == SPL_BAM_DROP_FLAGS));
    const uint32_t by_mapq = wv::popc64(wv::ballot(ok && ln.placed && ln.verdict == SPL_BAM_DROP_MAPQ));
    const uint32_t l = wv::lane();
    if (l == 0 && by_flags) atomicAdd(&counts->n_drop_flags, by_flags);
    if (l == 0 && by_mapq) atomicAdd(&counts->n_drop_mapq, by_mapq);
    if (fstat) { // (wave-uniform) the wave's row: word c = the lines of category c, QC-passed in the low half, QC-failed in the high
        const bool counted = ok && ln.verdict == SPL_BAM_KEPT;
        const uint32_t m = counted ? spl_flagstat_categories(ln.flag, ln.tid, ln.next_tid, ln.mapq) : 0u;
        const bool qc_fail = (ln.flag >> 9 & 1u) != 0u;
        uint32_t word = 0;
        for (uint32_t c = 0; c < SPL_FS_CATEGORIES; ++c) {
            const bool in = (m >> c & 1u) != 0u;
            const uint32_t pass = wv::popc64(wv::ballot(in && !qc_fail)), fail = wv::popc64(wv::ballot(in && qc_fail));
            if (l == c) word = pass | fail << 16;
        }
        const uint32_t row = i / 64u; // (lane 0's line exists whenever the wave has any: rows are written for those waves only)
        if (l < SPL_FS_CATEGORIES && (i - l) < n_lines) fstat[(size_t)row * SPL_FS_CATEGORIES + l] = word;
    }
}

// (Written once with a template parameter, as the BAM extractions are: KEY = false is the kernel a file gets that nobody asked the
//  name keys of -- spl_bam_set_mate_keys --, not a load, a branch or an argument more; KEY = true leaves the key of column 1 per read.)
template <bool KEY>
__device__ __forceinline__ void sam_extract_lines(const uint8_t *text, uint64_t base, const uint32_t *line_start, uint32_t n_lines, uint64_t last_end, const spl_sam_names &names,
                                                  const spl_bam_filter &filter, const uint32_t *kept_end, const uint32_t *ops_end, const int32_t *line_tid, uint64_t rec0, uint64_t op0,
                                                  uint64_t cap_rec, uint64_t cap_ops, int32_t *pos, uint16_t *flag, int32_t *tid, uint32_t *cig_off, uint32_t *cigar, uint8_t *xs,
                                                  unsigned long long *ref_max_end, spl_sam_counts *counts, uint64_t *name_key)
{
    const uint32_t i = blockIdx.x * SPL_SAM_SCAN_LANES + threadIdx.x;
    int32_t my_tid = -1;
    long long my_end = -1;
    if (i < n_lines) {
        const uint32_t k1 = kept_end[i], k0 = i ? kept_end[i - 1u] : 0u;
        if (k1 != k0) {
            const uint32_t o1 = ops_end[i], o0 = i ? ops_end[i - 1u] : 0u;
            const uint64_t r = rec0 + k1 - 1u, o = op0 + o0;
            if (r >= cap_rec || op0 + o1 > cap_ops) atomicOr(&counts->overflow, 1u);
            else {
                const uint8_t *p, *end;
                line_span(text, base, line_start, n_lines, last_end, i, p, end);
                spl_sam_line ln;
                spl_sam_parse_line(p, end, names, line_tid[i], filter, xs != nullptr, &ln);
                uint32_t n = 0;
                int64_t ref_len = 0;
                bool has_n = false;
                // (the scan took this line: the rule takes it again, and its CIGAR has the o1 - o0 ops the scan counted)
                if (ln.reason != SPL_SAM_OK || ln.n_ops != o1 - o0 || !spl_sam_cigar(p + ln.cigar_at, p + ln.cigar_at + ln.cigar_len, cigar + o, &n, &ref_len, &has_n))
                    atomicOr(&counts->overflow, 2u);
                pos[r] = ln.pos;
                flag[r] = (uint16_t)ln.flag;
                tid[r] = ln.tid;
                if (xs) xs[r] = ln.xs;
                if (KEY) name_key[r] = spl_name_key_sam(p, end);
                cig_off[r + 1u] = (uint32_t)(op0 + o1);
                my_tid = ln.tid;
                my_end = (long long)ln.end;
            }
        }
    }
    // ref_max_end: one atomic per wave and reference (a sorted file's wave holds one reference)
    for (uint32_t turn = 0; turn < 64u; ++turn) {
        const uint64_t open = wv::ballot(my_tid >= 0);
        if (!open) break;
        const uint32_t lead = wv::ffs64(open);
        const int32_t t = (int32_t)wv::shfl((uint32_t)my_tid, lead);
        const bool mine = my_tid == t;
        long long m = mine ? my_end : -1;
        for (uint32_t s = 32u; s; s >>= 1) {
            const long long other = (long long)((unsigned long long)wv::shfl((uint32_t)m, wv::lane() ^ s) | (unsigned long long)wv::shfl((uint32_t)((unsigned long long)m >> 32), wv::lane() ^ s) << 32);
            m = other > m ? other : m;
        }
        if (wv::lane() == lead) atomicMax(&ref_max_end[t], (unsigned long long)m);
        if (mine) my_tid = -1;
    }
}

__global__ __launch_bounds__(SPL_SAM_SCAN_LANES) void spl_sam_extract_kernel(const uint8_t *text, uint64_t base, const uint32_t *line_start, uint32_t n_lines, uint64_t last_end,
                                                                              spl_sam_names names, spl_bam_filter filter, const uint32_t *kept_end, const uint32_t *ops_end,
                                                                              const int32_t *line_tid, uint64_t rec0, uint64_t op0, uint64_t cap_rec, uint64_t cap_ops, int32_t *pos,
                                                                              uint16_t *flag, int32_t *tid, uint32_t *cig_off, uint32_t *cigar, uint8_t *xs,
                                                                              unsigned long long *ref_max_end, spl_sam_counts *counts)
{
    sam_extract_lines<false>(text, base, line_start, n_lines, last_end, names, filter, kept_end, ops_end, line_tid, rec0, op0, cap_rec, cap_ops, pos, flag, tid, cig_off, cigar, xs,
                             ref_max_end, counts, nullptr);
}

__global__ __launch_bounds__(SPL_SAM_SCAN_LANES) void spl_sam_extract_keys_kernel(const uint8_t *text, uint64_t base, const uint32_t *line_start, uint32_t n_lines, uint64_t last_end,
                                                                                   spl_sam_names names, spl_bam_filter filter, const uint32_t *kept_end, const uint32_t *ops_end,
                                                                                   const int32_t *line_tid, uint64_t rec0, uint64_t op0, uint64_t cap_rec, uint64_t cap_ops, int32_t *pos,
                                                                                   uint16_t *flag, int32_t *tid, uint32_t *cig_off, uint32_t *cigar, uint8_t *xs,
                                                                                   unsigned long long *ref_max_end, spl_sam_counts *counts, uint64_t *name_key)
{
    sam_extract_lines<true>(text, base, line_start, n_lines, last_end, names, filter, kept_end, ops_end, line_tid, rec0, op0, cap_rec, cap_ops, pos, flag, tid, cig_off, cigar, xs,
                            ref_max_end, counts, name_key);
}

__global__ __launch_bounds__(256) void spl_sam_order_kernel(const int32_t *tid, const int32_t *pos, uint64_t first, uint64_t n, spl_sam_counts *counts)
{
    const uint64_t r = first + (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (r >= first + n || r == 0) return;
    const int32_t t0 = tid[r - 1], t1 = tid[r];
    if (t1 < t0 || (t1 == t0 && pos[r] < pos[r - 1])) atomicOr(&counts->unordered, 1u);
}

// ---- the join behind an inflate (spl_sam.h): where the text that has arrived ends in a whole line, and lines too long for the rule
// The last '\n' of [lo, hi): a lane per sixteen bytes (the same aligned load and the same test as the line starts'), the wave's
// largest, one atomicMax a wave that has any.  *last = that byte's offset + 1, left as it was (the caller's 0) where there is none.
__global__ __launch_bounds__(256) void spl_sam_last_newline_kernel(const uint8_t *text, uint64_t lo, uint64_t hi, unsigned long long *last)
{
    const uint64_t base = lo & ~(uint64_t)15, hi16 = (hi + 15u) & ~(uint64_t)15;
    unsigned long long mine = 0;
    for (uint64_t at = base + ((uint64_t)blockIdx.x * 256u + threadIdx.x) * 16u; at < hi16; at += (uint64_t)gridDim.x * 256u * 16u) {
        const uint4 w = *(const uint4 *)(text + at);
        uint32_t nl = newline_bits(w.x) | newline_bits(w.y) << 4 | newline_bits(w.z) << 8 | newline_bits(w.w) << 12;
        if (at < lo) nl &= ~((1u << (uint32_t)(lo - at)) - 1u);              // (lo - at < 16: at >= base)
        if (at + 16u > hi) nl &= (1u << (uint32_t)(hi - at)) - 1u;           // (hi - at in 1 .. 15: at < hi16)
        if (nl) mine = at + (31u - (uint32_t)__clz((int)nl)) + 1u;           // (offsets go up along the loop: the last word with one wins)
    }
    for (uint32_t s = 32u; s; s >>= 1) {
        const unsigned long long other = (unsigned long long)wv::shfl((uint32_t)mine, wv::lane() ^ s) | (unsigned long long)wv::shfl((uint32_t)(mine >> 32), wv::lane() ^ s) << 32;
        mine = other > mine ? other : mine;
    }
    if (wv::lane() == 0 && mine) atomicMax(last, mine);
}

// *first_long = the smallest i whose line is longer than max_line, its newline counted (atomicMin; the caller sets ~0 first).
// Line i is [line_start[i], line_start[i + 1]), the last one ends at end_off (all from the window's base): a last line without a
// newline counts its bytes, as the host parser counts them.
__global__ __launch_bounds__(256) void spl_sam_long_line_kernel(const uint32_t *line_start, uint32_t n_lines, uint32_t end_off, uint32_t max_line, uint32_t *first_long)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n_lines) return;
    const uint32_t len = (i + 1u < n_lines ? line_start[i + 1u] : end_off) - line_start[i];
    if (len > max_line) atomicMin(first_long, i);
}

} // namespace

extern "C" int spl_dev_launch_sam_last_newline(const uint8_t *text, uint64_t lo, uint64_t hi, unsigned long long *last, void *st)
{
    if (hi <= lo) return 0;
    const uint64_t words = (((hi + 15u) & ~(uint64_t)15) - (lo & ~(uint64_t)15)) / 16u;
    const uint32_t groups = (uint32_t)std::min<uint64_t>((words + 255u) / 256u, 256u * 8u); // (eight workgroups a CU's worth of grid; the loop takes the rest)
    hipLaunchKernelGGL(spl_sam_last_newline_kernel, dim3(groups), dim3(256), 0, (hipStream_t)st, text, lo, hi, last);
    return (int)hipGetLastError();
}

extern "C" int spl_dev_launch_sam_long_line(const uint32_t *line_start, uint32_t n_lines, uint32_t end_off, uint32_t max_line, uint32_t *first_long, void *st)
{
    if (!n_lines) return 0;
    hipLaunchKernelGGL(spl_sam_long_line_kernel, dim3((n_lines + 255u) / 256u), dim3(256), 0, (hipStream_t)st, line_start, n_lines, end_off, max_line, first_long);
    return (int)hipGetLastError();
}

extern "C" uint32_t spl_sam_chunks(uint64_t lo, uint64_t hi)
{
    if (hi <= lo) return 0;
    const uint64_t base = lo & ~(uint64_t)15;
    return (uint32_t)((hi - base + SPL_SAM_CHUNK - 1u) / SPL_SAM_CHUNK);
}

extern "C" int spl_dev_launch_sam_line_count(const uint8_t *text, uint64_t lo, uint64_t hi, uint32_t *chunk_count, void *st)
{
    const uint32_t n = spl_sam_chunks(lo, hi);
    if (!n) return 0;
    hipLaunchKernelGGL(spl_sam_line_count_kernel, dim3(n), dim3(64), 0, (hipStream_t)st, text, lo, hi, chunk_count);
    return (int)hipGetLastError();
}

extern "C" int spl_dev_launch_sam_line_fill(const uint8_t *text, uint64_t lo, uint64_t hi, const uint32_t *chunk_end, uint32_t *line_start, void *st)
{
    const uint32_t n = spl_sam_chunks(lo, hi);
    if (!n) return 0;
    hipLaunchKernelGGL(spl_sam_line_fill_kernel, dim3(n), dim3(64), 0, (hipStream_t)st, text, lo, hi, chunk_end, line_start);
    return (int)hipGetLastError();
}

extern "C" int spl_dev_launch_sam_scan(const uint8_t *text, uint64_t base, const uint32_t *line_start, uint32_t n_lines, uint64_t last_end, const spl_sam_names *names,
                                       uint32_t min_mapq, uint32_t require_flags, uint32_t exclude_flags, int want_xs, uint32_t *kept, uint32_t *n_ops, int32_t *line_tid,
                                       uint32_t *fstat, spl_sam_counts *counts, void *st)
{
    if (!n_lines) return 0;
    hipLaunchKernelGGL(spl_sam_scan_kernel, dim3((n_lines + SPL_SAM_SCAN_LANES - 1u) / SPL_SAM_SCAN_LANES), dim3(SPL_SAM_SCAN_LANES), 0, (hipStream_t)st, text, base, line_start, n_lines,
                       last_end, *names, spl_bam_filter{min_mapq, require_flags, exclude_flags}, want_xs ? 1u : 0u, kept, n_ops, line_tid, fstat, counts);
    return (int)hipGetLastError();
}

extern "C" int spl_dev_launch_sam_extract(const uint8_t *text, uint64_t base, const uint32_t *line_start, uint32_t n_lines, uint64_t last_end, const spl_sam_names *names,
                                          uint32_t min_mapq, uint32_t require_flags, uint32_t exclude_flags, const uint32_t *kept_end, const uint32_t *ops_end, const int32_t *line_tid,
                                          uint64_t rec0, uint64_t op0, uint64_t cap_rec, uint64_t cap_ops, int32_t *pos, uint16_t *flag, int32_t *tid, uint32_t *cig_off, uint32_t *cigar,
                                          uint8_t *xs, unsigned long long *ref_max_end, spl_sam_counts *counts, void *st)
{
    if (!n_lines) return 0;
    hipLaunchKernelGGL(spl_sam_extract_kernel, dim3((n_lines + SPL_SAM_SCAN_LANES - 1u) / SPL_SAM_SCAN_LANES), dim3(SPL_SAM_SCAN_LANES), 0, (hipStream_t)st, text, base, line_start,
                       n_lines, last_end, *names, spl_bam_filter{min_mapq, require_flags, exclude_flags}, kept_end, ops_end, line_tid, rec0, op0, cap_rec, cap_ops, pos, flag, tid,
                       cig_off, cigar, xs, ref_max_end, counts);
    return (int)hipGetLastError();
}

extern "C" int spl_dev_launch_sam_extract_keys(const uint8_t *text, uint64_t base, const uint32_t *line_start, uint32_t n_lines, uint64_t last_end, const spl_sam_names *names,
                                               uint32_t min_mapq, uint32_t require_flags, uint32_t exclude_flags, const uint32_t *kept_end, const uint32_t *ops_end,
                                               const int32_t *line_tid, uint64_t rec0, uint64_t op0, uint64_t cap_rec, uint64_t cap_ops, int32_t *pos, uint16_t *flag, int32_t *tid,
                                               uint32_t *cig_off, uint32_t *cigar, uint8_t *xs, uint64_t *name_key, unsigned long long *ref_max_end, spl_sam_counts *counts, void *st)
{
    if (!name_key)
        return spl_dev_launch_sam_extract(text, base, line_start, n_lines, last_end, names, min_mapq, require_flags, exclude_flags, kept_end, ops_end, line_tid, rec0, op0, cap_rec,
                                          cap_ops, pos, flag, tid, cig_off, cigar, xs, ref_max_end, counts, st);
    if (!n_lines) return 0;
    hipLaunchKernelGGL(spl_sam_extract_keys_kernel, dim3((n_lines + SPL_SAM_SCAN_LANES - 1u) / SPL_SAM_SCAN_LANES), dim3(SPL_SAM_SCAN_LANES), 0, (hipStream_t)st, text, base, line_start,
                       n_lines, last_end, *names, spl_bam_filter{min_mapq, require_flags, exclude_flags}, kept_end, ops_end, line_tid, rec0, op0, cap_rec, cap_ops, pos, flag, tid,
                       cig_off, cigar, xs, ref_max_end, counts, name_key);
    return (int)hipGetLastError();
}

extern "C" int spl_dev_launch_sam_order(const int32_t *tid, const int32_t *pos, uint64_t first, uint64_t n, spl_sam_counts *counts, void *st)
{
    if (!n) return 0;
    hipLaunchKernelGGL(spl_sam_order_kernel, dim3((unsigned)((n + 255u) / 256u)), dim3(256), 0, (hipStream_t)st, tid, pos, first, n, counts);
    return (int)hipGetLastError();
}
