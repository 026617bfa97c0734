// spl_junctionfragment_rule.h -- which of the junctions a read supports a FRAGMENT has counted already, as straight-line C++: the
// rule of spl_junctions_fragments (the splice counts of `intronretention --fragments`).
//
// The kernel (spl_junctions.hip) includes this header with SPL_HD = __device__ __forceinline__.  It contains no HIP intrinsics, so
// that tests/ compile it with g++ too (spl_junction_fragment_rule_host, tests/hostsim/covfragment_rule_asan.cpp); the product never
// calls it on the host.
//
// Replaces nothing of the reference's: IRFinder, whose measure `intronretention` restates, works on fragments -- both mates of a
// pair that cross the same intron are one molecule's evidence for one splicing event.  The BED score of `junctions` / `process`
// stays per read: it feeds SpliSER's alpha, which stands beside the per-read beta1 / beta2.
//
// Walks, anchors, knobs, the strand modes 0 / 1 / 2 / 3 and the table keys are spl_junction_walk.h's and spl_junctions', unchanged:
// a read is walked when its flag 0x4 is clear and its POS is not negative.  THE RULE, per read r of a segment with its mate table:
// a junction that r SUPPORTS, with table key K = (l, r, strand code), is a DUPLICATE CARRY when
//   r has a mate m < r by the segment's mate table (m != SPL_MATE_NONE, m < n, m != r), and
//   read m's own walk supports a junction with the same key K -- (l, r) under the same knobs, the strand code taken by m's own
//   flag (or strand byte) under the same mode.
// A duplicate carry adds nothing, no count and no anchors; everything else is inserted exactly as spl_junctions inserts it.  Hence
// the table's key set is the per-read table's, count_frag(K) = count_read(K) - duplicates(K), and the anchors are <= the per-read
// table's.  Reads that are not pairable have no mate and behave as in the per-read table.
//
// A read's junctions ascend in l along its walk, so the look into the mate's walk ends at the first junction beyond l.
#ifndef SPL_JUNCTIONFRAGMENT_RULE_H
#define SPL_JUNCTIONFRAGMENT_RULE_H

#include <stdint.h>

#include "spl_junction_walk.h"
#include "spl_mate_rule.h"

namespace spljf {

// The strand code of a read's junctions under `stranded`: 0 '+' (and every read of mode 0), 1 '-', 2 '?' (mode 3: a strand byte
// that is neither).
SPL_HD uint32_t strand_code(uint32_t flag, uint32_t xs_byte, int stranded)
{
    if (stranded == 3) return xs_byte == (uint32_t)'+' ? 0u : xs_byte == (uint32_t)'-' ? 1u : 2u;
    return (stranded && spl_read_strand(flag, stranded) == (uint8_t)'-') ? 1u : 0u;
}

// Is a read walked at all?  (spl_junctions' condition.)
SPL_HD bool walked(uint32_t flag, int64_t pos) { return !(flag & 4u) && pos >= 0; }

// The earlier mate of read r of the n reads of a segment: -> its index within the segment, or -1.
SPL_HD int64_t earlier_mate(const uint32_t *mate, int64_t n, int64_t r)
{
    const uint32_t m = mate[r];
    return (m != SPL_MATE_NONE && (int64_t)m < n && (int64_t)m < r) ? (int64_t)m : -1; // (m < r: not the read itself)
}

// Does the walk of a read from p = POS + shift support the junction (l, r) under the knobs?
template <class Ops>
SPL_HD bool carries(const Ops &ops, uint32_t n_ops, int32_t p, const spljw::Filter &f, int32_t l, int32_t r)
{
    spljw::Walk w;
    w.begin(p);
    spljw::Junction j;
    while (spljw::next(w, ops, n_ops, f, j)) {
        if (j.l > l) return false;
        if (j.passes && j.l == l && j.r == r) return true;
    }
    return false;
}

// The whole rule for read r of a segment from arrays the caller can index as they are (the host's form): visit(l, r, strand code,
// anchor_left, anchor_right, duplicate) for every junction the read supports, in walk order.  xs: the reads' strand bytes (mode 3)
// or null.  -> false: the read's walk left the coordinate space (what it gave until then was visited).
template <class Visit>
SPL_HD bool read_junctions(const spl_read_view &s, const uint8_t *xs, int64_t n, int64_t r, const uint32_t *mate, int32_t shift, int stranded, const spljw::Filter &f, Visit &visit)
{
    const uint32_t flag = s.flag[r];
    const int64_t pos = (int64_t)s.pos[r];
    uint32_t c0, n_ops;
    s.ops_of(r, &c0, &n_ops);
    if (!walked(flag, pos) || n_ops < spljw::min_ops(f.min_anchor)) return true;
    const uint32_t code = strand_code(flag, xs ? xs[r] : 0u, stranded);
    int64_t m = earlier_mate(mate, n, r);
    uint32_t m0 = 0, m_ops = 0;
    int32_t m_p = 0;
    if (m >= 0) {
        s.ops_of(m, &m0, &m_ops);
        m_p = (int32_t)((int64_t)s.pos[m] + (int64_t)shift);
        if (!walked(s.flag[m], (int64_t)s.pos[m]) || strand_code(s.flag[m], xs ? xs[m] : 0u, stranded) != code) m = -1;
    }
    const spl_ops_ptr ops{s.cigar + c0};
    spljw::Walk w;
    w.begin((int32_t)((int64_t)s.pos[r] + (int64_t)shift));
    spljw::Junction j;
    while (spljw::next(w, ops, n_ops, f, j)) {
        if (!j.passes || (stranded == 3 && !spljw::key3_fits(j.l, j.r))) continue;
        const bool dup = m >= 0 && carries(spl_ops_ptr{s.cigar + m0}, m_ops, m_p, f, j.l, j.r);
        visit(j.l, j.r, code, j.anchor_left, j.anchor_right, dup);
    }
    return !w.range_error;
}

} // namespace spljf
#endif // SPL_JUNCTIONFRAGMENT_RULE_H
