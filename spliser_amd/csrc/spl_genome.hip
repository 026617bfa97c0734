// spl_genome.hip -- a FASTA's text packed into base codes on the device (spl_genome.h has the interface, the stored form and the
// method, spl_motif_rule.h the rule).  gfx950.
//
// Bytes moved, per window of B bytes holding L lines and N bases: the two line-start launches of spl_sam.hip read B each and write
// 4 L; classify and headers read two or three bytes a line and 4 L of the line table, write 8 L; the pack reads the N bytes of the
// sequence lines once, in aligned 4-byte words, and writes N / 2.  The text came over a link seven times slower than the memory it
// lies in.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "spl_genome.h"
#include "spl_motif_rule.h"

namespace {

__device__ __forceinline__ void line_of(const uint8_t *text, uint64_t base, const uint32_t *line_start, uint32_t n_lines, uint64_t last_end, uint64_t hi, uint32_t i, const uint8_t *&p,
                                        uint64_t &content)
{
    p = text + base + line_start[i];
    const bool inner = i + 1u < n_lines;
    const uint8_t *end = inner ? text + base + line_start[i + 1u] - 1 : text + last_end;
    content = splmotif::line_content(p, end, inner || last_end < hi);
}

__global__ __launch_bounds__(256) void spl_genome_classify_kernel(const uint8_t *text, uint64_t base, const uint32_t *line_start, uint32_t n_lines, uint64_t last_end, uint64_t hi,
                                                                  uint32_t *nb, uint32_t *hdr, spl_genome_counts *counts)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n_lines) return;
    const uint8_t *p;
    uint64_t content;
    line_of(text, base, line_start, n_lines, last_end, hi, i, p, content);
    const int kind = splmotif::line_kind(p, content);
    nb[i] = kind == SPL_FASTA_LINE_BASES ? (uint32_t)content : 0u;
    hdr[i] = kind == SPL_FASTA_LINE_HEADER ? 1u : 0u;
    if (kind == SPL_FASTA_LINE_HEADER && splmotif::name_length(p, content) == 0u) atomicMin(&counts->first_bad, (unsigned long long)i << 8 | SPL_FASTA_EMPTY_NAME);
}

__global__ __launch_bounds__(256) void spl_genome_headers_kernel(const uint8_t *text, uint64_t base, const uint32_t *line_start, uint32_t n_lines, uint64_t last_end, uint64_t hi,
                                                                 const uint32_t *nb_end, const uint32_t *hdr_end, int open_before, spl_genome_header *headers,
                                                                 spl_genome_counts *counts)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n_lines) return;
    const uint32_t h1 = hdr_end[i], h0 = i ? hdr_end[i - 1u] : 0u;
    if (h1 != h0) {
        const uint8_t *p;
        uint64_t content;
        line_of(text, base, line_start, n_lines, last_end, hi, i, p, content);
        spl_genome_header h;
        h.name_at = base + line_start[i] + 1u;
        h.name_len = (uint32_t)splmotif::name_length(p, content);
        h.bases_before = nb_end[i];
        h.line = i;
        h.pad = 0u;
        headers[h1 - 1u] = h;
    } else if (h1 == 0u && !open_before && nb_end[i] != (i ? nb_end[i - 1u] : 0u))
        atomicMin(&counts->first_bad, (unsigned long long)i << 8 | SPL_FASTA_BEFORE_HEADER);
}

// One lane, one 16-byte word of the store: 32 bases of one sequence.
__global__ __launch_bounds__(256) void spl_genome_pack_kernel(const uint8_t *text, uint64_t base, const uint32_t *line_start, uint32_t n_lines, const uint32_t *nb_end,
                                                              const spl_genome_segment *segs, uint32_t n_segs, uint32_t n_groups, uint8_t *store, uint64_t store_bytes)
{
    const uint32_t gid = blockIdx.x * 256u + threadIdx.x;
    if (gid >= n_groups) return;
    // the segment: the last one whose first group is at or below gid (segments without a group share their neighbour's number: the
    // last of equal ones is the one that has groups, n_groups > gid says there is one)
    uint32_t a = 0, b = n_segs;
    while (a + 1u < b) { const uint32_t mid = a + (b - a) / 2u; if (segs[mid].group_first <= gid) a = mid; else b = mid; }
    const spl_genome_segment sg = segs[a];
    const uint64_t grp = sg.seq_first / 32u + (gid - sg.group_first);
    const uint64_t q_end = sg.seq_first + sg.n;
    const uint64_t q_lo = grp * 32u > sg.seq_first ? grp * 32u : sg.seq_first, q_hi = grp * 32u + 32u < q_end ? grp * 32u + 32u : q_end;
    const uint64_t at = sg.dst + 16u * grp;
    if (q_lo >= q_hi || at + 16u > store_bytes) return; // (neither happens while the host's tables are right: said for the memory's sake)
    uint64_t lo = 0, hi = 0;
    if (q_lo > grp * 32u) { // the word's first bases came with the window before: its launch stored them, the nibbles behind them 0
        const uint2 *w = (const uint2 *)(store + at);
        const uint2 w0 = w[0], w1 = w[1];
        lo = (uint64_t)w0.x | (uint64_t)w0.y << 32;
        hi = (uint64_t)w1.x | (uint64_t)w1.y << 32;
    }
    uint32_t k = (uint32_t)(q_lo - grp * 32u), left = (uint32_t)(q_hi - q_lo);
    uint32_t wb = sg.wb + (uint32_t)(q_lo - sg.seq_first);
    // the line that holds the window's base wb: the first whose inclusive sum is beyond it
    uint32_t i = 0, j = n_lines;
    while (i < j) { const uint32_t mid = i + (j - i) / 2u; if (nb_end[mid] > wb) j = mid; else i = mid + 1u; }
    uint32_t before = i ? nb_end[i - 1u] : 0u;
    while (left && i < n_lines) {
        const uint32_t upto = nb_end[i];
        if (upto > wb) {
            const uint32_t take = upto - wb < left ? upto - wb : left;
            uint64_t addr = base + line_start[i] + (wb - before);
            const uint64_t stop = addr + take;
            while (addr < stop) { // aligned words: the buffer is readable from the window's base to 16 bytes behind its end
                const uint64_t wa = addr & ~(uint64_t)3;
                const uint32_t word = *(const uint32_t *)(text + wa);
                const uint32_t s = (uint32_t)(addr - wa), room = 4u - s, n = stop - addr < room ? (uint32_t)(stop - addr) : room;
                for (uint32_t m = 0; m < n; ++m) {
                    const uint64_t code = splmotif::base_code(word >> (8u * (s + m)) & 255u);
                    if (k < 16u) lo |= code << (4u * k); else hi |= code << (4u * (k - 16u));
                    ++k;
                }
                addr += n;
            }
            wb += take;
            left -= take;
        }
        before = upto;
        ++i;
    }
    uint4 v;
    v.x = (uint32_t)lo; v.y = (uint32_t)(lo >> 32); v.z = (uint32_t)hi; v.w = (uint32_t)(hi >> 32);
    *(uint4 *)(store + at) = v;
}

} // namespace

extern "C" int spl_dev_launch_genome_classify(const uint8_t *text, uint64_t base, const uint32_t *line_start, uint32_t n_lines, uint64_t last_end, uint64_t hi, uint32_t *nb, uint32_t *hdr,
                                              spl_genome_counts *counts, void *st)
{
    if (!n_lines) return 0;
    hipLaunchKernelGGL(spl_genome_classify_kernel, dim3((n_lines + 255u) / 256u), dim3(256), 0, (hipStream_t)st, text, base, line_start, n_lines, last_end, hi, nb, hdr, counts);
    return (int)hipGetLastError();
}

extern "C" int spl_dev_launch_genome_headers(const uint8_t *text, uint64_t base, const uint32_t *line_start, uint32_t n_lines, uint64_t last_end, uint64_t hi, const uint32_t *nb_end,
                                             const uint32_t *hdr_end, int open_before, spl_genome_header *headers, spl_genome_counts *counts, void *st)
{
    if (!n_lines) return 0;
    hipLaunchKernelGGL(spl_genome_headers_kernel, dim3((n_lines + 255u) / 256u), dim3(256), 0, (hipStream_t)st, text, base, line_start, n_lines, last_end, hi, nb_end, hdr_end,
                       open_before, headers, counts);
    return (int)hipGetLastError();
}

extern "C" int spl_dev_launch_genome_pack(const uint8_t *text, uint64_t base, const uint32_t *line_start, uint32_t n_lines, const uint32_t *nb_end, const spl_genome_segment *segs,
                                          uint32_t n_segs, uint32_t n_groups, uint8_t *store, uint64_t store_bytes, void *st)
{
    if (!n_groups || !n_segs || !n_lines) return 0;
    hipLaunchKernelGGL(spl_genome_pack_kernel, dim3((n_groups + 255u) / 256u), dim3(256), 0, (hipStream_t)st, text, base, line_start, n_lines, nb_end, segs, n_segs, n_groups, store,
                       store_bytes);
    return (int)hipGetLastError();
}
