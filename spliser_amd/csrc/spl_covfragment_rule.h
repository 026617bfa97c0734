// spl_covfragment_rule.h -- what ONE FRAGMENT of a paired-end library adds to the per-base depth of its reference, as straight-line
// C++: the rule of spl_coverage_fragments (the `coverage --fragments` switch).
//
// The kernel (spl_coverage.hip) includes this header with SPL_HD = __device__ __forceinline__.  It contains no HIP intrinsics, so
// that tests/ compile it with g++ too (spl_coverage_fragment_rule_host, tests/hostsim/covfragment_rule_asan.cpp); the product never
// calls it on the host.
//
// Replaces deepTools `bamCoverage` (paired-end default) / `bedtools genomecov -pc -split` over the file this library has just
// decoded: on a 2 x 150 library with 300-base inserts most mates overlap, and covering per read shows a depth of two over the
// overlap where one molecule was sequenced.  The reference has no counterpart.
//
// Mates, the mate table and A FRAGMENT'S SIDES -- which read is out, which is silent, which leads -- are spl_mate_rule.h's
// (spl_fragment_sides; here a mate must take part too); eligibility, the track, the walk, the blocks and their clipping are
// spl_coverage_rule.h's, unchanged.  THE RULE, per call -- one segment with its mate table, `length`, `stranded`, `strand`:
//   a read TAKES PART when spl_cov_eligible and spl_cov_on_track hold for it (secondary, supplementary, duplicate and QC-failed
//   reads still cover; only pairable reads can have a mate).  A mate on the other track of a stranded run is no partner: each
//   mate then covers alone on its own track;
//   a silent read marks nothing and is only "seen";
//   a leader marks the UNION of its own clipped blocks and, if it has one, its partner's: blocks that overlap OR abut become one
//   interval, the intervals are given ascending and disjoint.  It CONTRIBUTED when the union has a base, is PAST THE END when
//   either read lost a base to the clipping, and its covered bases are the union's length.
// A read's leader depends on the reads' order; the union does not, nor do the counters: a pair contributes once, whichever leads.
//
// NOTHING STORED PER LANE.  One read's clipped blocks ascend and are disjoint (spl_cov_cursor, spl_coverage_rule.h), so a
// fragment's union is the two-way merge of two block cursors: hold both heads, take the one that starts first, and let it
// lengthen the open interval or close it.
#ifndef SPL_COVFRAGMENT_RULE_H
#define SPL_COVFRAGMENT_RULE_H

#include <stdint.h>

#include "spl_coverage_rule.h"
#include "spl_mate_rule.h"

#define SPL_COVF_COUNTERS 4   // spl_coverage_rule.h's three predicates of a read, and [3]: it led a pair whose union was taken
#define SPL_COVF_PAIR 8u
// What read r of a segment is to a call (spl_cov_fragment_sides): spl_mate_rule.h's answers under the coverage's names.
#define SPL_COVF_NOT_PARTICIPATING SPL_FRAG_OUT
#define SPL_COVF_SILENT SPL_FRAG_SILENT
#define SPL_COVF_LEADS SPL_FRAG_LEADS // to be walked: a fragment's leader, or a read without a partner

// The coverage's predicate: a read takes part when it is eligible and on the call's track.
struct spl_cov_takes {
    int stranded, strand;
    SPL_HD bool operator()(uint32_t flag, int64_t pos, uint32_t n_ops) const { return spl_cov_eligible(flag, pos, n_ops) && spl_cov_on_track(flag, stranded, strand); }
};

// One read of a fragment as a cursor takes it: spl_mate_rule.h's side.
typedef spl_frag_side spl_cov_side;

// What read r of the n reads of a segment is to the call: SPL_COVF_NOT_PARTICIPATING, SPL_COVF_SILENT or SPL_COVF_LEADS
// (spl_fragment_sides; a mate that does not take part is no partner).
SPL_HD uint32_t spl_cov_fragment_sides(const spl_read_view &s, int64_t first, int64_t n, int64_t r, const uint32_t *mate, int64_t shift, int stranded, int strand, spl_cov_side *lead,
                                       spl_cov_side *other)
{
    return spl_fragment_sides<true>(s, first, n, r, mate, shift, spl_cov_takes{stranded, strand}, lead, other);
}

// The union of the clipped blocks of a read that leads (spl_cov_fragment_sides said SPL_COVF_LEADS): emit(s, e) for each interval,
// 0 <= s < e <= length, ascending and disjoint -- not even abutting.  cigar: the segment's ops.  -> SPL_COV_CONTRIBUTED,
// SPL_COV_PAST_END and SPL_COVF_PAIR as they hold; *covered_out = the union's bases.
template <class Ops, class Emit>
SPL_HD uint32_t spl_cov_fragment_walk(const uint32_t *cigar, const spl_cov_side &lead, const spl_cov_side &other, int64_t length, Emit &emit, int64_t *covered_out)
{
    spl_cov_cursor<Ops> x(Ops{cigar + lead.c0}, lead.n_ops, lead.p, length), y(Ops{cigar + other.c0}, other.n_ops, other.p, length);
    int64_t xs = 0, xe = 0, ys = 0, ye = 0, cs = 0, ce = 0, covered = 0; // the heads, and the open interval [cs, ce); cs == ce: none
    bool hx = x.next(&xs, &xe), hy = y.next(&ys, &ye);
    while (hx || hy) {
        int64_t s, e;
        if (hx && (!hy || xs <= ys)) { s = xs; e = xe; hx = x.next(&xs, &xe); }
        else { s = ys; e = ye; hy = y.next(&ys, &ye); }
        if (ce > cs && s <= ce) { if (e > ce) ce = e; continue; } // overlaps or abuts the open interval
        if (ce > cs) { emit(cs, ce); covered += ce - cs; }
        cs = s; ce = e;
    }
    if (ce > cs) { emit(cs, ce); covered += ce - cs; }
    *covered_out = covered;
    return ((x.bits | y.bits) & SPL_COV_PAST_END) | (covered ? SPL_COV_CONTRIBUTED : 0u) | (other.n_ops ? SPL_COVF_PAIR : 0u);
}

#endif // SPL_COVFRAGMENT_RULE_H
