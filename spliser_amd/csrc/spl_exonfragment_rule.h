// spl_exonfragment_rule.h -- which exon counting bins ONE FRAGMENT of a paired-end library counts for, as straight-line C++: the
// rule of spl_exon_count_fragments (the `exoncounts --countReadPairs` switch).
//
// The kernel (spl_exoncount.hip) includes this header with SPL_HD = __device__ __forceinline__.  It contains no HIP intrinsics, so
// that tests/ compile it with g++ too (spl_exon_fragment_rule_host, tests/hostsim/exonfragment_rule_asan.cpp,
// tests/hostsim/exonfragment_wave_host.cpp); the product never calls it on the host.
//
// Replaces the name-sorted second pass of `featureCounts -f -O -p --countReadPairs` / DEXSeq's paired counting over the file this
// library has just decoded: on a 2 x 150 library with 300-base inserts most fragments' mates overlap in an exon, and counting per
// read adds two to that exon's bin where both tools add one.  The reference has no counterpart.
//
// Mates, pairable reads, groups and A FRAGMENT'S SIDES -- which read is out, which is silent, which leads -- are spl_mate_rule.h's
// (spl_fragment_sides with spl_gene_eligible, by the table's word); eligibility, maps, blocks, hit stretches and bins are
// spl_exoncount_rule.h's.  THE RULE, per read r of a segment with its mate table:
//   a read that is out is NOT COUNTED, one per read; a silent read adds nothing and enters no counter;
//   a leader's hit stretches are its own, over the map of its own strand, and -- if it has a mate -- the mate's, over the map of
//   the mate's strand, by the mate's own flag (as in spl_gene_fragment_result).  VERDICT over the union of both reads' hit
//   stretches: any stretch shared, or two stretches with bins of different genes -> AMBIGUOUS, and NO bin is incremented; no
//   stretch with a bin -> NO FEATURE; otherwise COUNTED, and every DISTINCT bin of the union gets +1: a bin both mates hit counts
//   once, whether the mates saw it through the same map or through the two maps of a stranded run (a `.` feature).
// The four verdict counters ADDED sum to the reads minus the pairs.  By construction a fragment's verdict is the one
// spl_gene_count_fragments gives it on the gene maps of the same features.
//
// EACH BIN ONCE, WITH NOTHING STORED PER LANE.  A chromosome's bins are numbered in the order (start, end, gene) over both maps, and
// a map's stretches are disjoint and ascend: the bins ONE read's walk gives (spl_exon_next_bin) ascend strictly in bin number, on
// whichever map the read walks.  A fragment's bins are the two-way merge of two strictly ascending sequences (spl_exon_merge): hold
// both walks' heads, give the smaller one and advance that walk, and where the heads are equal give the bin once and advance both.
// "No further bin" is 0xFFFFFFFF, above every bin, so an ended walk never has the smaller head.
#ifndef SPL_EXONFRAGMENT_RULE_H
#define SPL_EXONFRAGMENT_RULE_H

#include <stdint.h>

#include "spl_exoncount_rule.h"
#include "spl_mate_rule.h"

#define SPL_EXON_NO_BIN 0xFFFFFFFFu // what a walk that has ended gives: above every bin (n_bins <= SPL_GENE_INDEX_MAX)

// One read of a fragment as a walk takes it: its ops (n_ops = 0: there is no such read), p = POS - 1 + shift, and whether map b
// serves it.
struct spl_exon_side {
    uint32_t c0, n_ops;
    int64_t p;
    bool on_b;
};

// What read r of the n reads of a segment is (spl_fragment_sides, by the table's word): SPL_EXON_NOT_COUNTED, SPL_EXON_IDLE (silent:
// its leader counts the fragment), or SPL_EXON_COUNTED -- to be walked: *lead is the read itself, *other its mate (n_ops = 0: it
// has none).  A side's map is settled here, from its read's own flag.
SPL_HD uint32_t spl_exon_fragment_sides(const spl_read_view &s, int64_t first, int64_t n, int64_t r, const uint32_t *mate, int64_t shift, int stranded, spl_exon_side *lead,
                                        spl_exon_side *other)
{
    spl_frag_side x, y;
    const uint32_t what = spl_fragment_sides<false>(s, first, n, r, mate, shift, spl_gene_takes{}, &x, &y);
    *lead = *other = spl_exon_side{0u, 0u, 0, false};
    if (what != SPL_FRAG_LEADS) return what == SPL_FRAG_SILENT ? SPL_EXON_IDLE : SPL_EXON_NOT_COUNTED;
    *lead = spl_exon_side{x.c0, x.n_ops, x.p, spl_gene_uses_b(x.flag, stranded)};
    if (y.n_ops) *other = spl_exon_side{y.c0, y.n_ops, y.p, spl_gene_uses_b(y.flag, stranded)};
    return SPL_EXON_COUNTED;
}

// One read's hit stretches into a verdict that is being made: have / gene = whether a bin was seen, and its gene.  -> false: the
// verdict is AMBIGUOUS (and nothing further needs a look).
template <class Ops, class Map>
SPL_HD bool spl_exon_verdict_add(const Ops &ops, uint32_t n_ops, int64_t p, const Map &map, const uint32_t *bin_gene, bool *have, uint32_t *gene)
{
    spl_exon_hits<Ops, Map> hits(ops, n_ops, p, map);
    uint32_t code = 0u;
    while (hits.next(&code)) {
        if (code == SPL_EXON_SHARED) return false;
        const uint32_t g = bin_gene[code - 1u];
        if (*have && g != *gene) return false;
        *have = true;
        *gene = g;
    }
    return true;
}

// The verdict of a fragment that is to be walked (spl_exon_fragment_sides said SPL_EXON_COUNTED).  cigar: the segment's ops.
template <class Ops, class Map>
SPL_HD uint32_t spl_exon_fragment_verdict(const uint32_t *cigar, const spl_exon_side &lead, const spl_exon_side &other, const Map &map_a, const Map &map_b, const uint32_t *bin_gene)
{
    bool have = false;
    uint32_t gene = 0u;
    if (!spl_exon_verdict_add(Ops{cigar + lead.c0}, lead.n_ops, lead.p, lead.on_b ? map_b : map_a, bin_gene, &have, &gene)) return SPL_EXON_AMBIGUOUS;
    if (other.n_ops && !spl_exon_verdict_add(Ops{cigar + other.c0}, other.n_ops, other.p, other.on_b ? map_b : map_a, bin_gene, &have, &gene)) return SPL_EXON_AMBIGUOUS;
    return have ? SPL_EXON_COUNTED : SPL_EXON_NO_FEATURE;
}

// The distinct bins of a COUNTED fragment, one by one in ascending order: the merge of its two reads' walks.  A side without ops
// gives nothing; with both sides so, next() is SPL_EXON_NO_BIN from the start.
template <class Ops, class Map>
struct spl_exon_merge {
    spl_exon_hits<Ops, Map> x, y;
    uint32_t hx, hy; // the walks' heads

    SPL_HD spl_exon_merge(const uint32_t *cigar, const spl_exon_side &lead, const spl_exon_side &other, const Map &map_a, const Map &map_b)
        : x(Ops{cigar + lead.c0}, lead.n_ops, lead.p, lead.on_b ? map_b : map_a), y(Ops{cigar + other.c0}, other.n_ops, other.p, other.on_b ? map_b : map_a), hx(SPL_EXON_NO_BIN),
          hy(SPL_EXON_NO_BIN)
    {
        if (lead.n_ops) hx = spl_exon_next_bin(x, SPL_EXON_NO_BIN);
        if (other.n_ops) hy = spl_exon_next_bin(y, SPL_EXON_NO_BIN);
    }

    SPL_HD uint32_t next()
    {
        const uint32_t bin = hx < hy ? hx : hy;
        if (bin == SPL_EXON_NO_BIN) return bin;
        if (hx == bin) hx = spl_exon_next_bin(x, SPL_EXON_NO_BIN);
        if (hy == bin) hy = spl_exon_next_bin(y, SPL_EXON_NO_BIN);
        return bin;
    }
};

// The whole rule for read r of a segment from arrays the caller can index as they are (the host's form): -> the verdict, or
// SPL_EXON_IDLE for a silent read; bins_out[0 .. cap) gets a counted fragment's distinct bins in ascending order, *n_hits_out their
// number (all of them, also beyond cap); any other verdict has no hit.
SPL_HD uint32_t spl_exon_fragment_result(const spl_read_view &s, int64_t n, int64_t r, const uint32_t *mate, int64_t shift, int stranded, const spl_gene_map_flat &a,
                                         const spl_gene_map_flat &b, const uint32_t *bin_gene, int64_t *bins_out, int64_t cap, int64_t *n_hits_out)
{
    *n_hits_out = 0;
    spl_exon_side lead, other;
    const uint32_t what = spl_exon_fragment_sides(s, 0, n, r, mate, shift, stranded, &lead, &other);
    if (what != SPL_EXON_COUNTED) return what;
    const uint32_t verdict = spl_exon_fragment_verdict<spl_ops_ptr>(s.cigar, lead, other, a, b, bin_gene);
    if (verdict != SPL_EXON_COUNTED) return verdict;
    spl_exon_merge<spl_ops_ptr, spl_gene_map_flat> merge(s.cigar, lead, other, a, b);
    for (uint32_t bin; (bin = merge.next()) != SPL_EXON_NO_BIN;) {
        if (*n_hits_out < cap) bins_out[*n_hits_out] = (int64_t)bin;
        ++*n_hits_out;
    }
    return verdict;
}

#endif // SPL_EXONFRAGMENT_RULE_H
