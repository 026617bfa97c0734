// spl_junction_walk.h -- the junctions one read carries: the walk over its CIGAR ops, one source for the device
// (spl_junctions.hip: spl_junction_fused_kernel over the BAM-native arrays) and the host (spl_junction_walk_host:
// tests/test_bedless_host.py holds it to oracle.junction_table).  spl_junction_kernel (spl_kernels.hip, packed records) states the
// same walk inline: that file is stamped by the committed HBM-traffic measurement (bench.py: kernel_src_sha16) and changes only
// together with a new measurement.
//
// Every N op of a read is a junction (l, r) in SpliSER's site convention (l = last base before the intron, r = last intronic
// base; SpliSER_v0_1_8.py:482-483).  Its anchors are the reference bases of the read between the junction and the previous /
// next N op or the read's end (the block sizes of a BED12 junction line).  A read SUPPORTS a junction only if both anchors are
// >= min_anchor and the intron length is in [min_intron, max_intron] (max_intron 0 = no upper limit): regtools' -a / -m / -M.
//
// Whether a read is walked at all (flag 0x4 clear, POS not negative) is the caller's business, and so is the strand.
#ifndef SPL_JUNCTION_WALK_H
#define SPL_JUNCTION_WALK_H
#include <stdint.h>

#include "spl_classify.h"
#include "spl_pack.h"

#ifndef SPL_JW_HD
#if defined(__HIPCC__) || defined(__CUDACC__)
#define SPL_JW_HD __host__ __device__ __forceinline__
#else
#define SPL_JW_HD inline
#endif
#endif

namespace spljw {

struct Filter { uint32_t min_anchor, min_intron, max_intron; };

// One N op of a read.
struct Junction {
    int32_t l, r;
    uint32_t anchor_left, anchor_right;
    bool passes; // the read supports it under the filter
};

// Where a walk stands: the next op, the cursor (1-based position of the next reference base), the reference bases since the
// previous N op (or the read's start).
struct Walk {
    uint32_t k, before;
    int32_t cur;
    bool range_error; // an op reached beyond SPL_COORD_MAX: the walk has ended there
    SPL_JW_HD void begin(int32_t pos) { k = 0; before = 0; cur = pos; range_error = false; }
};

// The fewest ops a read must have to support any junction under `min_anchor`: an anchor of one base or more needs a
// consuming op on that side of the N op.  With min_anchor = 0 a lone N op is a junction (both anchors empty).
SPL_JW_HD uint32_t min_ops(uint32_t min_anchor) { return min_anchor > 0u ? 3u : 1u; }

// The read's next N op into `out`; false when the ops are used up (or the walk left the coordinate space: w.range_error).
// `ops(k)` = the read's k-th op in BAM form (length << 4 | code).
template <class Ops>
SPL_JW_HD bool next(Walk &w, const Ops &ops, uint32_t n_ops, const Filter &f, Junction &out)
{
    while (w.k < n_ops) {
        const uint32_t op = ops(w.k);
        const uint32_t code = op & 15u, d = op >> 4;
        ++w.k;
        if (!((SPL_PROG_MASK >> code) & 1u)) continue;
        if ((int64_t)w.cur + d > (int64_t)SPL_COORD_MAX) { w.range_error = true; w.k = n_ops; return false; }
        w.cur += (int32_t)d;
        if (code != SPL_OP_N) { w.before += d; continue; }
        // anchor on the right: reference bases up to the next N op or the end of the read
        uint32_t after = 0;
        for (uint32_t k2 = w.k; k2 < n_ops; ++k2) {
            const uint32_t op2 = ops(k2);
            const uint32_t c2 = op2 & 15u;
            if (c2 == SPL_OP_N) break;
            if ((SPL_PROG_MASK >> c2) & 1u) after += op2 >> 4;
        }
        out.l = w.cur - (int32_t)d - 1;
        out.r = w.cur - 1;
        out.anchor_left = w.before;
        out.anchor_right = after;
        out.passes = out.anchor_left >= f.min_anchor && out.anchor_right >= f.min_anchor && d >= f.min_intron && (f.max_intron == 0u || d <= f.max_intron);
        w.before = 0;
        return true;
    }
    return false;
}

// The key of the device table: (l, r, strand bit); l in the high word as the unsigned number it is.
SPL_JW_HD unsigned long long key_of(int32_t l, int32_t r, unsigned long long strand_bit)
{
    return ((unsigned long long)(uint32_t)l << 32) | ((unsigned long long)(uint32_t)r << 1) | strand_bit;
}

// The key of a table whose strand comes from the reads' own bytes (spl_junctions, stranded = 3): THREE strand values -- 0 '+',
// 1 '-', 2 '?' -- need two bits, which key_of does not have beside 32 bits of l and 31 of r.  They are found by storing l + 1 and
// r + 1, 31 bits each: a walked read has POS >= 0 and every cursor it reaches is <= SPL_COORD_MAX = 2^31 - 67 (beyond it the
// walk ends with range_error, which the kernel turns into SPL_DEV_ERR_RANGE), so -1 <= l, r <= 2^31 - 68 and both sums fit.  A
// coordinate below -1 -- only a segment moved by a negative shift could make one -- is refused by the kernel with the same
// SPL_DEV_ERR_RANGE before it gets here.  Keys compare like (l, r, strand byte): '+' < '-' < '?'; none is ~0, the empty slot.
// The tables of stranded = 0 / 1 / 2 keep key_of.
SPL_JW_HD unsigned long long key3_of(int32_t l, int32_t r, unsigned long long strand_code)
{
    return ((unsigned long long)(uint32_t)(l + 1) << 33) | ((unsigned long long)(uint32_t)(r + 1) << 2) | strand_code;
}
SPL_JW_HD bool key3_fits(int32_t l, int32_t r) { return l >= -1 && r >= -1; }
SPL_JW_HD void key3_read(unsigned long long key, int32_t &l, int32_t &r, uint8_t &strand)
{
    l = (int32_t)(uint32_t)(key >> 33) - 1;
    r = (int32_t)(uint32_t)((key >> 2) & 0x7fffffffull) - 1;
    const uint32_t s = (uint32_t)(key & 3ull);
    strand = s == 0u ? (uint8_t)'+' : s == 1u ? (uint8_t)'-' : (uint8_t)'?';
}

} // namespace spljw
#endif
