// spl_coverage_rule.h -- what ONE read adds to the per-base depth of its reference, as straight-line C++: the rule of spl_coverage.
//
// The kernel (spl_coverage.hip) includes this header with SPL_HD = __device__ __forceinline__.  It contains no HIP intrinsics, so
// that the host compiles it too (spl_coverage_rule_host); the product never calls it on the host.
//
// Replaces a manual step: the reference's README sends the user to IGV whenever something looks wrong, and IGV wants a sorted,
// indexed BAM (or a coverage track: `bedtools genomecov -bg -split`, deepTools `bamCoverage`).  The reference has no counterpart.
//
// A read is ELIGIBLE when (flag & 0x4) == 0, POS >= 1 and it has at least one op: secondary, supplementary, duplicate and
// QC-failed reads count, as in bedtools genomecov (the decode's read filter narrows them).  With `stranded` 1 (fr) or 2 (rf) it
// belongs to the track spl_read_strand(flag, stranded) names, '+' or '-'; with 0 there is one track.  The WALK starts at the
// 0-based p = POS - 1 + shift, in int64: M, = and X cover [p, p + len) and advance; D and N advance without covering (a deletion
// is a gap, as an intron is: genomecov's -split); I, S, H, P and the op codes above 8 do nothing, nor does an op of length zero.
// Covering ops that abut (10M2I5M, 10M0N5M) are ONE block.  Blocks are CLIPPED to [0, length): a read that loses a base that way
// is "past the end", and one left without a covered base does not contribute.
#ifndef SPL_COVERAGE_RULE_H
#define SPL_COVERAGE_RULE_H

#include <stdint.h>

#include "spl_classify.h"

#define SPL_COV_COUNTERS 3 // predicates of a read: [0] seen, [1] contributed, [2] past the end (the covered bases are a sum)
#define SPL_COV_SEEN 1u
#define SPL_COV_CONTRIBUTED 2u
#define SPL_COV_PAST_END 4u
#define SPL_COV_LENGTH_MAX 2147483646ll // 2^31 - 2: every block end fits an int32, and so does length + 1
#define SPL_BLOCK_NONE 0x7FFFFFFFFFFFFFFFll // no block is open: above every position a walk reaches

SPL_HD bool spl_cov_eligible(uint32_t flag, int64_t pos, uint32_t n_ops) { return (flag & 0x4u) == 0u && pos >= 1 && n_ops >= 1u; }

// strand: 0 with stranded = 0, '+' or '-' with stranded = 1 / 2
SPL_HD bool spl_cov_args_fit(int stranded, int strand)
{
    if (stranded == 0) return strand == 0;
    return (stranded == 1 || stranded == 2) && (strand == '+' || strand == '-');
}

SPL_HD bool spl_cov_on_track(uint32_t flag, int stranded, int strand) { return stranded == 0 || (int)spl_read_strand(flag, stranded) == strand; }

// THE BLOCK WALK, stated once, an op a step: a read's blocks [s, e), ascending, disjoint and not clipped, from p in int64.  Every
// op that advances either covers or is a gap, so p is always the open block's end: a covering op lengthens the open block or
// opens one at p, a gap or the read's end closes it.  Whoever walks feeds the read's ops in turn (BAM form) and then its end.
struct spl_block_walk {
    int64_t p, bs; // the open block is [bs, p); bs == SPL_BLOCK_NONE: none is open
    SPL_HD explicit spl_block_walk(int64_t p0) : p(p0), bs(SPL_BLOCK_NONE) {}
    // at_end: the read's end, `op` is nothing.  -> true: a block ended here, [*s, *e).
    SPL_HD bool feed(bool at_end, uint32_t op, int64_t *s, int64_t *e)
    {
        int64_t len = 0; // (the read's end: a gap of no length)
        if (!at_end) {
            len = (int64_t)(op >> 4);
            if (len == 0 || !((SPL_PROG_MASK >> (op & 15u)) & 1u)) return false;
            if ((SPL_MAPPED_MASK >> (op & 15u)) & 1u) { // covers: abuts the open block, or opens one
                if (bs == SPL_BLOCK_NONE) bs = p;
                p += len;
                return false;
            }
        }
        const bool ended = bs != SPL_BLOCK_NONE; // the open block ends here
        if (ended) { *s = bs; *e = p; bs = SPL_BLOCK_NONE; }
        p += len;
        return ended;
    }
};

// The walk, clipped and resumable: next() gives the read's clipped blocks one by one, 0 <= s < e <= length, ascending and disjoint;
// bits gathers SPL_COV_PAST_END as the walk meets it (complete once next() has said false).  ops(k) = the read's k-th op.
template <class Ops>
struct spl_cov_cursor {
    Ops ops;
    uint32_t n_ops, k, bits; // k: the next op (n_ops + 1: the walk is over)
    int64_t length;
    spl_block_walk walk;
    SPL_HD spl_cov_cursor(const Ops &o, uint32_t n, int64_t p0, int64_t len) : ops(o), n_ops(n), k(0u), bits(0u), length(len), walk(p0) {}
    SPL_HD bool next(int64_t *s, int64_t *e)
    {
        while (k <= n_ops) {
            const uint32_t at = k++;
            int64_t bs, be;
            if (!walk.feed(at == n_ops, at < n_ops ? ops(at) : 0u, &bs, &be)) continue;
            *s = bs < 0 ? 0 : bs;
            *e = be > length ? length : be;
            if (*s != bs || *e != be) bits |= SPL_COV_PAST_END; // the clipping took a base
            if (*e > *s) return true;
        }
        return false;
    }
};

// The clipped blocks of one read that is eligible and on the track: emit(s, e) for each, ascending.  -> SPL_COV_* bits without
// SPL_COV_SEEN; *covered_out = the bases the blocks hold.
template <class Ops, class Emit>
SPL_HD uint32_t spl_cov_walk(const Ops &ops, uint32_t n_ops, int64_t p, int64_t length, Emit &emit, int64_t *covered_out)
{
    spl_cov_cursor<Ops> blocks(ops, n_ops, p, length);
    int64_t covered = 0, s, e;
    while (blocks.next(&s, &e)) { emit(s, e); covered += e - s; }
    *covered_out = covered;
    return blocks.bits | (covered ? SPL_COV_CONTRIBUTED : 0u);
}

#endif // SPL_COVERAGE_RULE_H
