// spl_genecount_rule.h -- which gene ONE read counts for, as straight-line C++: the rule of spl_gene_count.
//
// The kernel (spl_genecount.hip) includes this header with SPL_HD = __device__ __forceinline__.  It contains no HIP intrinsics, so
// that tests/ compile it with g++ too (spl_gene_count_rule_host, tests/hostsim/genecount_rule_asan.cpp); the product never calls it
// on the host.
//
// Replaces a second pass over the alignment file by another program: the diffSpliSER analysis is an edgeR analysis, and the gene's
// expression beside a change in SSE comes from `htseq-count` or `featureCounts` over the file this library has just decoded.  The
// reference has no counterpart.
//
// A GENE MAP of the set's coordinate space is an ascending int32 start[n] with a uint32 code[n], code[k] holding for the 0-based
// positions start[k] <= p < start[k + 1] (the last entry to +infinity; 0 below start[0]): 0 = no feature, g + 1 = features of the
// one gene g only, 0xFFFFFFFF = features of two or more genes.  A read is ELIGIBLE when it is mapped, primary, QC-passed and not
// supplementary (spl_strand_eligible; duplicates count), POS >= 1 and it has at least one op; any other read is NOT COUNTED.  An
// eligible read's BLOCKS are the block walk's (spl_coverage_rule.h) from the 0-based p = POS - 1 + shift, in int64, not clipped: M, =
// and X cover, D and N are gaps, covering ops that abut are one block.  Its GENE SET is the union, over every stretch of the map
// that a block overlaps by a base or more, of that stretch's code: empty -> NO FEATURE, exactly one gene -> that gene, anything
// else -> AMBIGUOUS (htseq-count's --mode union --nonunique none, featureCounts' default, per read).  With stranded = 1 (fr) or 2
// (rf) the read looks only at the map of spl_read_strand(flag, stranded): map a for '+', map b for '-'.
#ifndef SPL_GENECOUNT_RULE_H
#define SPL_GENECOUNT_RULE_H

#include <stdint.h>

#include "spl_classify.h"
#include "spl_coverage_rule.h"
#include "spl_read_view.h"
#include "spl_strand_rule.h"

#define SPL_GENE_MANY 0xFFFFFFFFu         // a map code: two or more genes
#define SPL_GENE_SPECIALS 3               // counters behind the genes': no feature, ambiguous, not counted
// What a read comes to: a gene index below SPL_GENE_INDEX_MAX, or one of these.  (SPL_GENE_IDLE: a lane without a read.)
#define SPL_GENE_NO_FEATURE 0xFFFFFFFCu
#define SPL_GENE_AMBIGUOUS 0xFFFFFFFDu
#define SPL_GENE_NOT_COUNTED 0xFFFFFFFEu
#define SPL_GENE_IDLE 0xFFFFFFFFu
#define SPL_GENE_INDEX_MAX 0xFFFFFFF0u    // n_genes at most: every code g + 1 and every result stays clear of the values above

SPL_HD bool spl_gene_eligible(uint32_t flag, int64_t pos, uint32_t n_ops) { return spl_strand_eligible(flag) && pos >= 1 && n_ops >= 1u; }

// A map searched in one step, as the host has it.  (The kernel's has the top level in LDS: spl_genecount.hip.)
struct spl_gene_map_flat {
    int64_t n;
    const int32_t *start;
    const uint32_t *code;
    SPL_HD int64_t size() const { return n; }
    SPL_HD int64_t find(int64_t pos) const { return spl_cover_find(start, 0, n, pos); } // the last k with start[k] <= pos, -1: none
    SPL_HD int64_t start_at(int64_t k) const { return (int64_t)start[k]; }
    SPL_HD uint32_t code_at(int64_t k) const { return code[k]; }
};

// The fold of a read's blocks over a map: what the block walk's blocks go into.  set: 0 = empty, g + 1 = the one gene g, SPL_GENE_MANY.
template <class Map>
struct spl_gene_fold {
    const Map &map;
    uint32_t set;
    SPL_HD void add(uint32_t code)
    {
        if (code == 0u) return;
        set = (set == 0u || set == code) ? code : SPL_GENE_MANY;
    }
    SPL_HD void operator()(int64_t s, int64_t e) // the block [s, e), s < e
    {
        if (set == SPL_GENE_MANY) return; // (nothing takes "many" back: the fold is over)
        const int64_t n = map.size();
        int64_t k = map.find(s);
        if (k >= 0) add(map.code_at(k)); // the stretch s lies in
        for (++k; k < n && set != SPL_GENE_MANY && map.start_at(k) < e; ++k) add(map.code_at(k)); // ... and those that begin inside the block
    }
};

// The form that CONTINUES a set (a fragment's: spl_mate_rule.h): `set` as a fold has it -> the set with the blocks of these ops
// folded in, p = POS - 1 + shift.  ops(k) = the read's k-th op (BAM form).
// THE SECOND STATEMENT OF THE BLOCK WALK, kept on purpose: spl_cov_walk's former loop without the clipping.  Over spl_block_walk's
// step (spl_coverage_rule.h) spl_gene_count_kernel measured 2.8 and 3.6 % slower than with this loop, beyond the 2 % it was allowed
// (DESIGN.md, section 3).  A change of the rule changes both; tests/test_blockwalk_host.py holds both to one restatement.
template <class Ops, class Map>
SPL_HD uint32_t spl_gene_set_add_blocks(uint32_t set, const Ops &ops, uint32_t n_ops, int64_t p, const Map &map)
{
    spl_gene_fold<Map> fold{map, set};
    int64_t bs = 0, be = 0; // the open block [bs, be); bs == be: none
    for (uint32_t k = 0; k <= n_ops; ++k) {
        int64_t len = 0;
        bool covers = false;
        if (k < n_ops) {
            const uint32_t op = ops(k);
            len = (int64_t)(op >> 4);
            if (len == 0 || !((SPL_PROG_MASK >> (op & 15u)) & 1u)) continue;
            covers = ((SPL_MAPPED_MASK >> (op & 15u)) & 1u) != 0u;
        }
        if (covers && be > bs && p == be) { be += len; p += len; continue; } // abuts the open block
        if (be > bs) { fold(bs, be); bs = be = 0; }
        if (covers) { bs = p; be = p + len; }
        p += len;
    }
    return fold.set;
}
// What a finished set comes to.
SPL_HD uint32_t spl_gene_result_of_set(uint32_t set) { return set == 0u ? SPL_GENE_NO_FEATURE : set == SPL_GENE_MANY ? SPL_GENE_AMBIGUOUS : set - 1u; }

// What an ELIGIBLE read with these ops comes to over `map`.
template <class Ops, class Map>
SPL_HD uint32_t spl_gene_of_blocks(const Ops &ops, uint32_t n_ops, int64_t p, const Map &map)
{
    return spl_gene_result_of_set(spl_gene_set_add_blocks(0u, ops, n_ops, p, map));
}

// Map b serves this read (stranded = 1 / 2 and a '-' read); map a every other.
SPL_HD bool spl_gene_uses_b(uint32_t flag, int stranded) { return stranded != 0 && spl_read_strand(flag, stranded) == (uint8_t)'-'; }

// The whole rule for one read from arrays the caller can index as they are (the host's form).
SPL_HD uint32_t spl_gene_read_result(uint32_t flag, int64_t pos, const uint32_t *ops, uint32_t n_ops, int64_t shift, int stranded, const spl_gene_map_flat &a,
                                     const spl_gene_map_flat &b)
{
    if (!spl_gene_eligible(flag, pos, n_ops)) return SPL_GENE_NOT_COUNTED;
    return spl_gene_of_blocks(spl_ops_ptr{ops}, n_ops, pos - 1 + shift, spl_gene_uses_b(flag, stranded) ? b : a);
}

// A map as the entries take it: strictly ascending starts, codes 0 .. n_genes or SPL_GENE_MANY.  -> -1 when it is one, else the
// first entry that is not (*why: 0 = its start, 1 = its code).
SPL_HD int64_t spl_gene_map_flaw(int64_t n, const int32_t *start, const uint32_t *code, int64_t n_genes, int *why)
{
    for (int64_t k = 0; k < n; ++k) {
        if (k && start[k] <= start[k - 1]) { *why = 0; return k; }
        if (code[k] != SPL_GENE_MANY && (int64_t)code[k] > n_genes) { *why = 1; return k; }
    }
    return -1;
}

#endif // SPL_GENECOUNT_RULE_H
