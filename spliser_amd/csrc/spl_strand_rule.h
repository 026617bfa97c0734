// spl_strand_rule.h -- what ONE read says about the library's strandedness, as straight-line C++: the rule of spl_strand_tally.
//
// The kernel (spl_strand.hip) includes this header with SPL_HD = __device__ __forceinline__.  It contains no HIP intrinsics, so
// that tests/ compile it with g++ too (spl_strand_rule_host, tests/hostsim/strand_rule_asan.cpp); the product never calls it on
// the host.
//
// Replaces a manual step: the reference's README tells the user to open the BAM in IGV, colour the reads by first-in-pair and
// compare them with a junction to learn whether the library is unstranded, fr or rf.  The reference has no counterpart.
//
// A read is ELIGIBLE when it is mapped, primary, QC-passed and not supplementary.  Its MATE CLASS follows the branch
// spl_read_strand takes (0 unpaired, 1 first, 2 second), its FR STRAND is spl_read_strand(flag, 1).  Two independent sources
// say what strand the read's transcript has:
//   tag         the read's strand byte when that is '+' or '-' (the aligner's XS:A tag: spl_bam_set_aux_strand, spl_soa_upload3);
//   annotation  a strand cover map of the chromosome: ascending int32 start[n] with uint8 code[n], code[k] holding for positions
//               start[k] <= p < start[k + 1] (the last entry to +infinity; 0 below start[0]); 0 = no gene, 1 = only '+' genes,
//               2 = only '-' genes, 3 = both.  The read has evidence when its whole reference span [POS, POS + ref_len - 1],
//               introns included, lies in ONE stretch whose code is 1 or 2 (ref_len >= 1; all in int64).
// Counters, int64[14]: [0] reads seen, [1] eligible, [2 + 2 m + d] eligible reads of mate class m with tag evidence, d = 0 when
// the fr strand equals the evidence and 1 when it does not; [8 + 2 m + d] the same for annotation evidence.
#ifndef SPL_STRAND_RULE_H
#define SPL_STRAND_RULE_H

#include <stdint.h>

#include "spl_classify.h"

#define SPL_STRAND_COUNTERS 14

SPL_HD bool spl_strand_eligible(uint32_t flag) { return (flag & (0x4u | 0x100u | 0x200u | 0x800u)) == 0u; }

SPL_HD uint32_t spl_strand_mate_class(uint32_t flag)
{
    if (!(flag & 1u)) return 0u;
    return (flag & 64u) ? 1u : 2u;
}

// The bases of the reference a read covers, introns included: the op lengths under SPL_PROG_MASK.
SPL_HD int64_t spl_strand_ref_len(const uint32_t *ops, uint32_t n_ops)
{
    int64_t len = 0;
    for (uint32_t k = 0; k < n_ops; ++k) {
        const uint32_t op = ops[k];
        if ((SPL_PROG_MASK >> (op & 15u)) & 1u) len += (int64_t)(op >> 4);
    }
    return len;
}

// The last k of [lo, hi) with start[k] <= pos; lo - 1 when there is none.  start is ascending.
SPL_HD int64_t spl_cover_find(const int32_t *start, int64_t lo, int64_t hi, int64_t pos)
{
    int64_t a = lo, b = hi; // the first k of [lo, hi) with start[k] > pos is in [a, b]
    while (a < b) {
        const int64_t mid = a + (b - a) / 2;
        if ((int64_t)start[mid] <= pos) a = mid + 1;
        else b = mid;
    }
    return a - 1;
}

// The strand the map gives a read at pos with ref_len bases, entry k being the last one with start[k] <= pos (k < 0: none):
// '+', '-' or 0.
SPL_HD uint8_t spl_cover_evidence(int64_t k, int64_t n_cover, const int32_t *start, const uint8_t *code, int64_t pos, int64_t ref_len)
{
    if (ref_len < 1 || k < 0 || k >= n_cover) return 0;
    if (k + 1 < n_cover && pos + ref_len - 1 >= (int64_t)start[k + 1]) return 0;
    const uint8_t c = code[k];
    return c == 1 ? (uint8_t)'+' : c == 2 ? (uint8_t)'-' : (uint8_t)0;
}

// Bit i = the read adds one to counter i.  tag: the strand byte (0 = none); ann: the map's strand for the read (0 = none).
SPL_HD uint32_t spl_strand_bits(uint32_t flag, uint8_t tag, uint8_t ann)
{
    uint32_t bits = 1u;
    if (!spl_strand_eligible(flag)) return bits;
    bits |= 2u;
    const uint32_t m = spl_strand_mate_class(flag);
    const uint8_t fr = spl_read_strand(flag, 1);
    if (tag == (uint8_t)'+' || tag == (uint8_t)'-') bits |= 1u << (2u + 2u * m + (fr != tag ? 1u : 0u));
    if (ann == (uint8_t)'+' || ann == (uint8_t)'-') bits |= 1u << (8u + 2u * m + (fr != ann ? 1u : 0u));
    return bits;
}

// The whole rule for one read from arrays the caller can index as they are (the host's form; the kernel finds k in two steps).
SPL_HD uint32_t spl_strand_read_bits(uint32_t flag, int64_t pos, const uint32_t *ops, uint32_t n_ops, uint8_t tag, int64_t n_cover, const int32_t *start,
                                     const uint8_t *code)
{
    uint8_t ann = 0;
    if (n_cover > 0 && spl_strand_eligible(flag))
        ann = spl_cover_evidence(spl_cover_find(start, 0, n_cover, pos), n_cover, start, code, pos, spl_strand_ref_len(ops, n_ops));
    return spl_strand_bits(flag, tag, ann);
}

#endif // SPL_STRAND_RULE_H
