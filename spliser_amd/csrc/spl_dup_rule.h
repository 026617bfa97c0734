// spl_dup_rule.h -- which fragments of a segment are PCR DUPLICATES of another, as straight-line C++: the rule of
// spl_reads_duplicates / spl_reads_dedup (spl_dups.hip) and of `duplicates` / `--dedup`.
//
// The kernels include this header with SPL_HD = __device__ __forceinline__.  It contains no HIP intrinsics, so that tests/ compile
// it with g++ too (spl_duplicates_host, tests/hostsim/dup_rule_asan.cpp); the product never calls it on the host.
//
// Replaces Picard MarkDuplicates / `samtools fixmate` + `samtools markdup` in front of `--excludeFlags 0x400`: both want a
// coordinate-sorted copy of the file and rewrite it.  The reference has no counterpart.
//
// THE RULE, per segment (one chromosome's reads) of a finished, fused set with name keys.
// EXAMINED: a read is examined when spl_gene_eligible holds (mapped, primary, QC-passed, not supplementary, POS >= 1, an op at
// least).  An incoming 0x400 bit is ignored.  Every other record is never marked.
// FRAGMENTS: spl_fragment_sides<false> with spl_gene_takes over the segment's mate table (spl_mate_rule.h).  A read that LEADS with
// a mate is a PAIR fragment, one that leads without is a SINGLE fragment, a SILENT read belongs to its leader's fragment:
// examined = 2 * pairs + singles.
// THE UNCLIPPED 5' END of a read: cl = the sum of the S/H ops before the first op that is neither (every op a clip: cl is their
// sum and ct = 0), ct = the sum of the S/H ops after the last op that is neither, L = the sum of the M, D, N, =, X lengths,
// o = FLAG bit 0x10;  u = POS - cl when o = 0, else POS + L - 1 + ct, in 64 bits, clamped to [-2^31, 2^31 - 1].
// THE SIGNATURE, three 64-bit words.  For a pair, end A is the smaller of the two reads' ends by (u, o), on a tie the read with
// FLAG 0x40; B is the other.
//   W0 = (uA + 2^31) << 3 | oA << 2 | paired << 1 | (paired && A's read has 0x40)           (35 bits)
//   W1 = paired ? (uB + 2^31) << 1 | oB : 0                                                   (33 bits)
//   W2 = the name key (both mates share it; 0 for a nameless read)
// DUPLICATES: the fragments of one segment with equal (W0, W1) are a GROUP; the one with the smallest W2 is its representative,
// ties to the lowest leader index; every other fragment is a duplicate, and both of its reads are marked.
//
// The signature and W2 depend on the reads' content only, so the same NAMES are marked whatever the file's order or container.
// THIS HOLDS FOR NAMED READS ONLY: nameless fragments of a group tie at W2 = 0, and which of them stays is then the segment's order.
//
// DELIBERATE DIFFERENCES from Picard and samtools (parity intended and unpinned; yardstick tests/dupcases.py):
//   * no base qualities are decoded: the representative is chosen by name hash, not by quality sum;
//   * a pair split over two chromosomes or by a decode filter is two single fragments;
//   * singles compete only with singles (Picard marks a single whose end matches a pair's);
//   * secondary, supplementary, QC-failed and unmapped records are never marked (the user adds --excludeFlags 0x900);
//   * no optical duplicates, no UMIs.
#ifndef SPL_DUP_RULE_H
#define SPL_DUP_RULE_H

#include <stdint.h>

#include "spl_mate_rule.h"

#define SPL_DUP_COUNTERS 7 // reads, examined, pair fragments, single fragments, duplicate pairs, duplicate singles, examined with 0x400
#define SPL_DUP_BINS 256   // group sizes 1 .. 255 and 256+
#define SPL_DUP_HIST 257   // ... and behind them the fragments of the groups in the last bin
#define SPL_DUP_REF_MASK 0x18Du // M, D, N, =, X
#define SPL_DUP_W0_BITS 35u
#define SPL_DUP_W1_BITS 33u

SPL_HD bool spl_dup_is_clip(uint32_t op) { return (op & 15u) == 4u || (op & 15u) == 5u; }

// u of a read: a forward read's walk ends at its first op that is no clip.
template <class Ops>
SPL_HD int64_t spl_dup_end(const Ops &ops, uint32_t n_ops, int64_t pos, uint32_t flag)
{
    uint32_t k = 0;
    int64_t cl = 0, u;
    for (; k < n_ops; ++k) {
        const uint32_t op = ops(k);
        if (!spl_dup_is_clip(op)) break;
        cl += (int64_t)(op >> 4);
    }
    if (!(flag & 0x10u)) u = pos - cl;
    else {
        int64_t len = 0, ct = 0;
        for (; k < n_ops; ++k) {
            const uint32_t op = ops(k);
            if (spl_dup_is_clip(op)) { ct += (int64_t)(op >> 4); continue; }
            ct = 0;
            if ((SPL_DUP_REF_MASK >> (op & 15u)) & 1u) len += (int64_t)(op >> 4);
        }
        u = pos + len - 1 + ct;
    }
    return u < -2147483648LL ? -2147483648LL : u > 2147483647LL ? 2147483647LL : u;
}

struct spl_dup_sig {
    uint64_t w0, w1, w2;
};

// What read r of the n reads of a segment is to the rule (SPL_FRAG_OUT: not examined; SPL_FRAG_SILENT: its leader has the
// fragment; SPL_FRAG_LEADS), without a walk of anybody's ops: the rule's policy -- the table's word, the file's POS (shift 0), the
// counts' predicate -- said once.  other->n_ops != 0: a leader has a mate.
SPL_HD uint32_t spl_dup_sides(const spl_read_view &s, int64_t first, int64_t n, int64_t r, const uint32_t *mate, spl_frag_side *lead, spl_frag_side *other)
{
    return spl_fragment_sides<false>(s, first, n, r, mate, 0, spl_gene_takes{}, lead, other);
}

// The signature of the fragment whose leader is `lead` (other.n_ops = 0: a single); key: the leader's name key.
SPL_HD spl_dup_sig spl_dup_signature(const spl_read_view &s, const spl_frag_side &lead, const spl_frag_side &other, uint64_t key)
{
    const int64_t ul = spl_dup_end(spl_ops_ptr{s.cigar + lead.c0}, lead.n_ops, lead.p + 1, lead.flag);
    const uint64_t ol = (lead.flag >> 4) & 1u;
    spl_dup_sig sig{0ull, 0ull, key};
    if (!other.n_ops) {
        sig.w0 = (uint64_t)(ul + 2147483648LL) << 3 | ol << 2;
        return sig;
    }
    const int64_t um = spl_dup_end(spl_ops_ptr{s.cigar + other.c0}, other.n_ops, other.p + 1, other.flag);
    const uint64_t om = (other.flag >> 4) & 1u;
    const bool lead_is_a = ul != um ? ul < um : ol != om ? ol < om : (lead.flag & 0x40u) != 0u;
    const int64_t ua = lead_is_a ? ul : um, ub = lead_is_a ? um : ul;
    const uint64_t oa = lead_is_a ? ol : om, ob = lead_is_a ? om : ol;
    const uint64_t a_first = ((lead_is_a ? lead.flag : other.flag) >> 6) & 1u;
    sig.w0 = (uint64_t)(ua + 2147483648LL) << 3 | oa << 2 | 2ull | a_first;
    sig.w1 = (uint64_t)(ub + 2147483648LL) << 1 | ob;
    return sig;
}

// (W0, W1) of element a below / equal to that of element b
SPL_HD bool spl_dup_same(const uint64_t *w0, const uint64_t *w1, int64_t a, int64_t b) { return w0[a] == w0[b] && w1[a] == w1[b]; }

// The end of the group whose head is element j of the n elements sorted by (W0, W1): the first place behind j whose (W0, W1) is
// greater -- a binary search, nothing linear in the group's length.
SPL_HD int64_t spl_dup_group_end(const uint64_t *w0, const uint64_t *w1, int64_t n, int64_t j)
{
    const uint64_t a = w0[j], b = w1[j];
    int64_t lo = j + 1, hi = n;
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (w0[mid] < a || (w0[mid] == a && w1[mid] <= b)) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// The mark stage for element j of the sorted elements (perm[j]: its number in leader order; lead[e]: element e's leader): -> whether
// it is a duplicate; then dup[leader] and dup[mate] are set (dup: the segment's n bytes, cleared by the caller).
SPL_HD bool spl_dup_mark_element(const uint64_t *w0, const uint64_t *w1, const uint32_t *perm, const uint32_t *lead, int64_t n_el, int64_t j, const uint32_t *mate, int64_t n,
                                 uint8_t *dup)
{
    if (j < 1 || !spl_dup_same(w0, w1, j - 1, j)) return false;
    const uint32_t e = perm[j];
    if ((int64_t)e >= n_el) return false; // (a permutation of the elements: said for the memory's sake)
    const uint32_t r = lead[e];
    if ((int64_t)r >= n) return false;
    dup[r] = 1u;
    if (w0[j] & 2ull) {
        const uint32_t m = mate[r];
        if ((int64_t)m < n) dup[m] = 1u;
    }
    return true;
}

#endif // SPL_DUP_RULE_H
