// spl_mate_rule.h -- which two reads of a chromosome are MATES, what a read is to a per-fragment call (A FRAGMENT'S SIDES: the
// gene, exon and coverage rules all ask it here), and which gene a FRAGMENT counts for, as straight-line C++: the rule of
// spl_mate_table (spl_mates.hip) and of spl_gene_count_fragments (spl_genecount.hip).
//
// The kernels include this header with SPL_HD = __device__ __forceinline__.  It contains no HIP intrinsics, so that tests/ compile
// it with g++ too (spl_name_key_host, spl_mate_table_host, spl_gene_fragment_rule_host, tests/hostsim/mate_rule_asan.cpp); the
// product never calls it on the host.
//
// Replaces the name-sorted second pass of `htseq-count` / `featureCounts -p --countReadPairs` over the file this library has just
// decoded: paired-end libraries are counted per fragment by both.  The reference has no counterpart.
//
// THE NAME KEY of a read is 64 bits of its QNAME as the file has it (BAM: l_read_name - 1 bytes, without the NUL; SAM: column 1):
// FNV-1a over the bytes -- h = 0xcbf29ce484222325, per byte h = (h ^ b) * 0x100000001b3 -- then the finisher h ^= h >> 33,
// h *= 0xff51afd7ed558ccd, h ^= h >> 33, h *= 0xc4ceb9fe1a85ec53, h ^= h >> 33, all mod 2^64.  An empty name and the name `*` have
// key 0, "no name"; any other name whose hash comes to 0 has key 1.
//
// THE MATE TABLE of a segment (one chromosome's reads, in the segment's order).  A read is PAIRABLE when it is spl_gene_eligible
// (mapped, primary, QC-passed, not supplementary, POS >= 1, an op at least), has flag 0x1, exactly one of 0x40 and 0x80, and a
// key that is not 0.  Its SORT KEY is the name key with bit 0 replaced by its kind: 0 = first in pair (0x40), 1 = second (0x80).
// A GROUP is all pairable reads of the segment with equal key >> 1.  In a group the j-th first read and the j-th second read, in
// the segment's order, are mates; every other read has none.  mate[i] = the mate's index within the segment or SPL_MATE_NONE;
// the table is symmetric.  A group is one first and one second read unless a name occurs twice in the file or two names' upper 63
// hash bits collide; the rank rule only makes what happens then deterministic.  WHAT A COLLISION COSTS: two fragments of one
// chromosome may swap mates (each is then counted with the other's second read).  HOW LIKELY: for n distinct names on a chromosome
// about n^2 / 2^64 colliding pairs -- 5e-6 for 10 M names.  (Derived from the 63 bits, not measured.)
//
// THE PAIR STAGE works on the pairable reads' sort keys in ascending order, equal keys in the segment's order (a stable sort): all
// first reads of a group stand before its second reads.  For the element at place j the group's start, its first second-kind
// element and its end are three binary searches; the partner's place is an offset.  Nothing is linear in a group's length.
//
// A FRAGMENT'S SIDES (spl_fragment_sides): what read r of a segment is to a per-fragment call, asked ONCE for every such command.
// A read that does not TAKE PART in the call (the caller's predicate: spl_gene_eligible for the gene and exon counts; eligible and
// on the track for the coverage) is OUT.  A read that takes part and whose mate has a lower index is SILENT: its LEADER does the
// fragment's work.  Every other read that takes part LEADS, with its mate as the second side if it has one.  A mate index that is
// SPL_MATE_NONE, at or beyond n, or r itself means no mate (a table of this segment: said for the memory's sake).  ONE POLICY differs
// between the commands: the counts take the table's word -- pairable reads are eligible ones, so "silent" is decided before the
// mate is looked at -- while the coverage wants the mate to take part in this same call, and a mate that does not (on the other
// track of a stranded run) is no partner: the read then leads alone.
//
// A FRAGMENT'S GENE.  A read that is out is NOT COUNTED, one per read; a silent read adds nothing.  A leader folds its blocks over
// the map of its own strand (spl_gene_uses_b of its own flag) and, if it has a mate, the mate's blocks over the map of the mate's
// strand, by the mate's own flag, into the same gene set: empty -> NO FEATURE, one gene -> that gene, else AMBIGUOUS.  (Under fr,
// flags 99 and 147 land on the same map; a pair whose mates' strands disagree looks at both maps, as htseq-count does.)  The rows
// sum to reads - pairs.
#ifndef SPL_MATE_RULE_KEY_H
#define SPL_MATE_RULE_KEY_H

#include <stdint.h>

#define SPL_MATE_NONE 0xFFFFFFFFu
#define SPL_MATE_NAME_OFFSET 36 // a BAM record's read_name, from the record's block_size field

// ---- the key --------------------------------------------------------------------------------------------------------------------
// (The decoders include this part alone -- SPL_MATE_KEY_ONLY defined around the #include -- and call it on the host and on the
// device alike.)
#if defined(__HIPCC__)
#define SPL_KEY_HD __host__ __device__ inline
#else
#define SPL_KEY_HD inline
#endif
SPL_KEY_HD uint64_t spl_name_hash_begin() { return 0xcbf29ce484222325ull; }
SPL_KEY_HD uint64_t spl_name_hash_byte(uint64_t h, uint8_t b) { return (h ^ (uint64_t)b) * 0x100000001b3ull; }
// len: the name's bytes; only: its first byte (anything when len == 0)
SPL_KEY_HD uint64_t spl_name_hash_end(uint64_t h, uint64_t len, uint8_t only)
{
    if (len == 0 || (len == 1 && only == (uint8_t)'*')) return 0ull;
    h ^= h >> 33; h *= 0xff51afd7ed558ccdull;
    h ^= h >> 33; h *= 0xc4ceb9fe1a85ec53ull;
    h ^= h >> 33;
    return h ? h : 1ull;
}
SPL_KEY_HD uint64_t spl_name_key(const uint8_t *name, uint64_t len)
{
    uint64_t h = spl_name_hash_begin();
    for (uint64_t k = 0; k < len; ++k) h = spl_name_hash_byte(h, name[k]);
    return spl_name_hash_end(h, len, len ? name[0] : (uint8_t)0);
}
// The key of a BAM record's name: l_read_name - 1 bytes at `name`, and none at or beyond rec_end.
SPL_KEY_HD uint64_t spl_name_key_bam(const uint8_t *name, uint32_t l_read_name, const uint8_t *rec_end)
{
    uint64_t len = l_read_name ? l_read_name - 1u : 0u;
    if (name >= rec_end) len = 0;
    else if (len > (uint64_t)(rec_end - name)) len = (uint64_t)(rec_end - name);
    return spl_name_key(name, len);
}
// The key of a SAM line's column 1: the bytes from the line's start to its first TAB, and none at or beyond `end`.
SPL_KEY_HD uint64_t spl_name_key_sam(const uint8_t *line, const uint8_t *end)
{
    const uint8_t *q = line;
    uint64_t h = spl_name_hash_begin();
    for (; q < end && *q != (uint8_t)'\t'; ++q) h = spl_name_hash_byte(h, *q);
    return spl_name_hash_end(h, (uint64_t)(q - line), q > line ? line[0] : (uint8_t)0);
}

#endif // SPL_MATE_RULE_KEY_H

#if !defined(SPL_MATE_KEY_ONLY) && !defined(SPL_MATE_RULE_H)
#define SPL_MATE_RULE_H
#include "spl_genecount_rule.h"

// ---- the table ------------------------------------------------------------------------------------------------------------------
SPL_HD bool spl_mate_pairable(uint32_t flag, int64_t pos, uint32_t n_ops, uint64_t key)
{
    return spl_gene_eligible(flag, pos, n_ops) && (flag & 0x1u) && (((flag >> 6) ^ (flag >> 7)) & 1u) && key != 0ull;
}
SPL_HD uint64_t spl_mate_sort_key(uint64_t key, uint32_t flag) { return (key & ~1ull) | (uint64_t)((flag >> 7) & 1u); }

// the first j of [lo, hi) with keys[j] >= k (hi: none) / with keys[j] > k
SPL_HD int64_t spl_mate_lower(const uint64_t *keys, int64_t lo, int64_t hi, uint64_t k)
{
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (keys[mid] < k) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}
SPL_HD int64_t spl_mate_upper(const uint64_t *keys, int64_t lo, int64_t hi, uint64_t k)
{
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (keys[mid] <= k) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}
// The pair stage for the element at place j of the n sorted keys: -> its partner's place, or -1.
SPL_HD int64_t spl_mate_partner(const uint64_t *keys, int64_t n, int64_t j)
{
    const uint64_t k = keys[j], k0 = k & ~1ull, k1 = k | 1ull;
    const int64_t begin = spl_mate_lower(keys, 0, j + 1, k0);   // (keys[j] >= k0: the group begins at j at the latest)
    const int64_t end = spl_mate_upper(keys, j, n, k1);         // (keys[j] <= k1: it ends behind j)
    const int64_t second = spl_mate_lower(keys, begin, end, k1);
    if (k & 1ull) {
        const int64_t rank = j - second;
        return rank < second - begin ? begin + rank : -1;
    }
    const int64_t rank = j - begin;
    return rank < end - second ? second + rank : -1;
}
// ... and what it writes: index[] = the sorted elements' reads (within the segment of n_reads); mate[] was filled with
// SPL_MATE_NONE.  -> whether element j has a partner.
SPL_HD bool spl_mate_pair_element(const uint64_t *keys, const uint32_t *index, int64_t n, int64_t j, uint32_t *mate, int64_t n_reads)
{
    const int64_t q = spl_mate_partner(keys, n, j);
    if (q < 0) return false;
    const uint32_t me = index[j], other = index[q];
    if ((int64_t)me >= n_reads || (int64_t)other >= n_reads) return false; // (indexes of this segment: said for the memory's sake)
    mate[me] = other;
    return true;
}

// ---- a fragment's sides, and its gene ---------------------------------------------------------------------------------------------
// The arrays of a segment as the rule reads them, and one read of a fragment as a walk takes it (spl_frag_side; its FLAG says
// which map serves it: spl_gene_uses_b): spl_read_view.h's spl_read_view.  mate[] is the segment's table.

#define SPL_FRAG_OUT 0u
#define SPL_FRAG_SILENT 1u
#define SPL_FRAG_LEADS 2u // to be walked

// The counts' predicate.
struct spl_gene_takes {
    SPL_HD bool operator()(uint32_t flag, int64_t pos, uint32_t n_ops) const { return spl_gene_eligible(flag, pos, n_ops); }
};

// What read r of the n reads of a segment is to a call.  *lead: the read itself when it takes part (n_ops = 0: it is out); *other:
// a leader's mate (n_ops = 0: it has none).  MateMustTake: the policy above -- false, the table's word; true, a mate that does
// not take part is no partner.
template <bool MateMustTake, class Takes>
SPL_HD uint32_t spl_fragment_sides(const spl_read_view &s, int64_t first, int64_t n, int64_t r, const uint32_t *mate, int64_t shift, const Takes &takes, spl_frag_side *lead,
                                   spl_frag_side *other)
{
    const spl_frag_side none{0u, 0u, 0, 0u};
    *lead = *other = none;
    spl_frag_side me, its = none;
    if (!s.side_of(first + r, shift, takes, &me)) return SPL_FRAG_OUT;
    *lead = me;
    const uint32_t m = mate[r];
    bool has_mate = m != SPL_MATE_NONE && (int64_t)m < n && (int64_t)m != r; // (a table of this segment: said for the memory's sake)
    if (MateMustTake && has_mate) has_mate = s.side_of(first + (int64_t)m, shift, takes, &its);
    if (has_mate && (int64_t)m < r) return SPL_FRAG_SILENT;
    if (!MateMustTake && has_mate) (void)s.side_of(first + (int64_t)m, shift, takes, &its); // (a read that is silent by the table's word never looks at its mate)
    if (has_mate) *other = its;
    return SPL_FRAG_LEADS;
}

// What read r of the n reads of a segment adds: a gene, SPL_GENE_NO_FEATURE, SPL_GENE_AMBIGUOUS, SPL_GENE_NOT_COUNTED -- or
// SPL_GENE_IDLE: nothing, its leader counts the fragment.  Ops: made from a pointer to the read's first op.
template <class Ops, class Map>
SPL_HD uint32_t spl_gene_fragment_result(const spl_read_view &s, int64_t first, int64_t n, int64_t r, const uint32_t *mate, int64_t shift, int stranded, const Map &map_a,
                                         const Map &map_b)
{
    spl_frag_side lead, other;
    const uint32_t what = spl_fragment_sides<false>(s, first, n, r, mate, shift, spl_gene_takes{}, &lead, &other);
    if (what != SPL_FRAG_LEADS) return what == SPL_FRAG_SILENT ? SPL_GENE_IDLE : SPL_GENE_NOT_COUNTED;
    uint32_t set = spl_gene_set_add_blocks(0u, Ops{s.cigar + lead.c0}, lead.n_ops, lead.p, spl_gene_uses_b(lead.flag, stranded) ? map_b : map_a);
    if (other.n_ops) set = spl_gene_set_add_blocks(set, Ops{s.cigar + other.c0}, other.n_ops, other.p, spl_gene_uses_b(other.flag, stranded) ? map_b : map_a);
    return spl_gene_result_of_set(set);
}

#endif // SPL_MATE_RULE_H
