// spl_exoncount_rule.h -- which exon counting bins ONE read counts for, as straight-line C++: the rule of spl_exon_count.
//
// The kernel (spl_exoncount.hip) includes this header with SPL_HD = __device__ __forceinline__.  It contains no HIP intrinsics, so
// that tests/ compile it with g++ too (spl_exon_count_rule_host, tests/hostsim/exoncount_rule_asan.cpp); the product never calls it
// on the host.
//
// Replaces a second pass over the alignment file by another program: whoever looks at a change in splice-site strength also asks
// about exon usage (edgeR::diffSpliceDGE, DEXSeq), which needs reads per exon counting bin -- `featureCounts -f -O` or
// `dexseq_count.py` over the file this library has just decoded.  The reference has no counterpart.
//
// FEATURES and SELECTIONS are genecounts' own: a feature is an interval [left, right) of one gene, features with right <= left are
// ignored; unstranded, map a is made of all of a chromosome's features; stranded, map a of those whose strand is not '-', map b of
// those whose strand is not '+' (a '.' is in both).
// BINS.  For one selection, cut the chromosome at every left and every right of its features.  A piece between two consecutive cuts
// that no feature covers has code 0; one covered by features of exactly one gene g is the BIN (g, start, end); one covered by
// features of two or more genes is SHARED, code 0xFFFFFFFF, and no bin.  Two abutting exons of one gene are two bins, the same exon
// in two transcripts is one, and the same (gene, start, end) out of both maps is one.  A chromosome's bins are numbered
// 0 .. n_bins - 1 in the order (start, end, gene) over the distinct triples of both maps.
// A BIN MAP has the shape of a gene map (spl_genecount_rule.h): an ascending int32 start[n] with a uint32 code[n], code[k] holding
// for start[k] <= p < start[k + 1] (the last entry to +infinity; 0 below start[0]): 0 = none, b + 1 = bin b, 0xFFFFFFFF = shared; an
// entry only where the code changes.  bin_gene[n_bins] is every bin's gene, a uint32 that is only ever compared for equality.
// A READ.  Eligibility and map are spl_gene_count's (spl_gene_eligible, spl_gene_uses_b).  Its BLOCKS are the block walk's from
// p = POS - 1 + shift, in int64, nothing clipped.  Its HIT STRETCHES are the stretches of its map that a block overlaps by a base or
// more, each taken once however many of its blocks overlap it (a deletion or an intron inside one bin gives two blocks in one
// stretch).  VERDICT: any hit stretch shared, or two hit stretches with bins of different genes -> AMBIGUOUS, and no bin is
// incremented; no hit stretch with a bin -> NO FEATURE; otherwise COUNTED, and every hit stretch's bin gets +1; every other read of
// the set is NOT COUNTED.  This is DEXSeq's counting (dexseq_count.py: reads with bins of more than one gene are _ambiguous) and
// `featureCounts -f -O` restricted to reads of one gene, applied per READ: a paired fragment adds up to two to a bin.  Parity with
// both is intended and unpinned.  By construction the verdict is the one spl_gene_count gives the read on the gene maps of the
// same features.
#ifndef SPL_EXONCOUNT_RULE_H
#define SPL_EXONCOUNT_RULE_H

#include <stdint.h>

#include "spl_genecount_rule.h"

#define SPL_EXON_SHARED SPL_GENE_MANY // a map code: features of two or more genes
#define SPL_EXON_VERDICTS 4           // counters behind the bins': counted, no feature, ambiguous, not counted
// What a read comes to: the index of its counter behind the bins'.  (SPL_EXON_IDLE: a lane without a read.)
#define SPL_EXON_COUNTED 0u
#define SPL_EXON_NO_FEATURE 1u
#define SPL_EXON_AMBIGUOUS 2u
#define SPL_EXON_NOT_COUNTED 3u
#define SPL_EXON_IDLE 4u

// The hit stretches of one eligible read over `map`, one by one: the block walk (spl_block_walk, spl_coverage_rule.h), not
// clipped, every block held against the map.  A stretch that consecutive blocks hit is given once: blocks and stretches both
// ascend, so the index of the last stretch given is all there is to remember.  Stretches of code 0 are hit and passed over: they
// hold no bin and decide nothing.
template <class Ops, class Map>
struct spl_exon_hits {
    const Ops ops;      // (both by value: a few words, and a lane's walk then points at nothing of the caller's)
    uint32_t n_ops;
    const Map map;
    uint32_t k;         // the next op (n_ops + 1: the walk is over)
    spl_block_walk walk;
    int64_t s, e;       // the block held against the map, s == e: none
    int64_t j, last;    // the next stretch to look at for [s, e); the last one given (-1: none)

    SPL_HD spl_exon_hits(const Ops &ops_, uint32_t n_ops_, int64_t p_, const Map &map_) : ops(ops_), n_ops(n_ops_), map(map_), k(0u), walk(p_), s(0), e(0), j(0), last(-1) {}

    // The read's next block into [s, e), not clipped.  -> false: there is none.
    SPL_HD bool next_block()
    {
        while (k <= n_ops) {
            const uint32_t at = k++;
            if (walk.feed(at == n_ops, at < n_ops ? ops(at) : 0u, &s, &e)) return true;
        }
        return false;
    }

    // *code = the code of the read's next hit stretch that is not 0.  -> false: there is none (and from then on).
    SPL_HD bool next(uint32_t *code)
    {
        const int64_t n = map.size();
        for (;;) {
            if (s >= e) {
                if (!next_block()) return false;
                j = map.find(s); // the stretch s lies in; those that begin inside the block follow it
                if (j < 0) j = 0;
            }
            while (j < n && map.start_at(j) < e) {
                const int64_t hit = j++;
                if (hit == last) continue;
                last = hit;
                *code = map.code_at(hit);
                if (*code != 0u) return true;
            }
            s = e = 0;
        }
    }
};

// The verdict of an ELIGIBLE read with these ops over `map`, p = POS - 1 + shift.  bin_gene: n_bins genes (codes are 1 .. n_bins).
template <class Ops, class Map>
SPL_HD uint32_t spl_exon_verdict(const Ops &ops, uint32_t n_ops, int64_t p, const Map &map, const uint32_t *bin_gene)
{
    spl_exon_hits<Ops, Map> hits(ops, n_ops, p, map);
    bool have = false;
    uint32_t gene = 0u, code = 0u;
    while (hits.next(&code)) {
        if (code == SPL_EXON_SHARED) return SPL_EXON_AMBIGUOUS;
        const uint32_t g = bin_gene[code - 1u];
        if (have && g != gene) return SPL_EXON_AMBIGUOUS;
        have = true;
        gene = g;
    }
    return have ? SPL_EXON_COUNTED : SPL_EXON_NO_FEATURE;
}

// The bins of a COUNTED read, one by one (its walk again: every code is a bin's).  -> the bin, `none` when there is no further one.
template <class Ops, class Map>
SPL_HD uint32_t spl_exon_next_bin(spl_exon_hits<Ops, Map> &hits, uint32_t none)
{
    uint32_t code = 0u;
    return hits.next(&code) && code != SPL_EXON_SHARED ? code - 1u : none;
}

// The whole rule for one read from arrays the caller can index as they are (the host's form): -> the verdict; bins_out[0 .. cap)
// gets a counted read's bins in ascending order of their stretches, *n_hits_out their number (all of them, also beyond cap); any
// other verdict has no hit.
SPL_HD uint32_t spl_exon_read_result(uint32_t flag, int64_t pos, const uint32_t *ops, uint32_t n_ops, int64_t shift, int stranded, const spl_gene_map_flat &a, const spl_gene_map_flat &b,
                                     const uint32_t *bin_gene, int64_t *bins_out, int64_t cap, int64_t *n_hits_out)
{
    *n_hits_out = 0;
    if (!spl_gene_eligible(flag, pos, n_ops)) return SPL_EXON_NOT_COUNTED;
    const spl_gene_map_flat &map = spl_gene_uses_b(flag, stranded) ? b : a;
    const spl_ops_ptr o{ops};
    const uint32_t verdict = spl_exon_verdict(o, n_ops, pos - 1 + shift, map, bin_gene);
    if (verdict != SPL_EXON_COUNTED) return verdict;
    spl_exon_hits<spl_ops_ptr, spl_gene_map_flat> hits(o, n_ops, pos - 1 + shift, map);
    for (uint32_t bin; (bin = spl_exon_next_bin(hits, 0xFFFFFFFFu)) != 0xFFFFFFFFu;) {
        if (*n_hits_out < cap) bins_out[*n_hits_out] = (int64_t)bin;
        ++*n_hits_out;
    }
    return verdict;
}

#endif // SPL_EXONCOUNT_RULE_H
