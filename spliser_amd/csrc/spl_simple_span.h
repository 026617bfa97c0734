// spl_simple_span.h -- the fused range kernel's question about a thread's SIMPLE reads (one aligned op, mapped, in range: run 0),
// as straight-line C++: the position index's arithmetic, the range of one simple read, and the span test that asks ONE pair of
// bucket entries for all of a thread's simple reads.
//
// The kernel (spl_kernels.hip: dbk_slot, dbk_resolve, SimpleInPlace) includes this header with SPL_HD = __device__
// __forceinline__.  It contains no HIP intrinsics, so that the host compiles it too (spl_simple_span_host: the CPU suite holds
// it to a plain restatement); the product never calls it on the host.
//
// The position index: 32 bp buckets from dbase on, entry s = {first: distinct-position index ("dpos") of the first site at or
// after the bucket's start, occ: which of its 32 positions are sites}.  The table begins with empty buckets in front of the first
// site and ends with an empty one whose first is the number of distinct positions, so clamping s is all the range handling there
// is: for x outside the table the clamped entry is empty and its popcounts are 0 whatever the bit index says.
//
// A simple read with bases [a, b) counts for the sites t that have t and t + 1 under it -- the distinct positions [lo, ub), lo =
// (sites <= a - 1), ub = (sites < b - 1), from the entries of a - 1 and b - 1 -- and for nothing when ub <= lo.  lo does not fall when a grows, ub
// does not fall when b grows (clamped entries included), so with a_min = the least a and b_max = the greatest b of ANY set of
// simple reads, ub(b_max) <= lo(a_min) means that every one of them has an empty range: two entries answer for the whole set.
// The other way round the test says nothing (two reads 150 bases apart with a site between them: the span holds a site, no
// read does) -- a flagged thread's reads are then looked at one by one.  The order of the reads does not matter.
#ifndef SPL_SIMPLE_SPAN_H
#define SPL_SIMPLE_SPAN_H

#include <stdint.h>

#include "spl_classify.h"

SPL_HD uint32_t spl_dbk_slot_of(int32_t dbase, uint32_t n_dbuckets, int32_t x)
{
    // x - dbase cannot wrap: coordinates stay <= SPL_COORD_MAX = 2^31 - 67 and dbase >= -64
    int32_t b = (x - dbase) >> 5;
    b = b < 0 ? 0 : b;
    const int32_t last = (int32_t)n_dbuckets - 1;
    return (uint32_t)(b > last ? last : b);
}

// u = distinct positions below x, nv = x is a site
SPL_HD void spl_dbk_resolve_at(int32_t dbase, int32_t x, uint32_t first, uint32_t occ, int32_t &u, uint32_t &nv)
{
    const uint32_t bit = (uint32_t)(x - dbase) & 31u;
    u = (int32_t)(first + (uint32_t)__builtin_popcount(occ & ((1u << bit) - 1u)));
    nv = (occ >> bit) & 1u;
}

// The bases [a, b) of a simple read from its record's two words: w0 = POS in the segment's coordinates, w1 = length << 16 | flag.
SPL_HD void spl_simple_bases(uint32_t w0, uint32_t w1, int32_t shift, int32_t &a, int32_t &b)
{
    a = (int32_t)w0 + shift;
    b = a + (int32_t)(w1 >> 16);
}

// [lo, ub) of bases [a, b) from the entries of a - 1 (first0, occ0) and b - 1 (first1, occ1); -> the range is not empty.
SPL_HD bool spl_simple_range(int32_t dbase, int32_t a, int32_t b, uint32_t first0, uint32_t occ0, uint32_t first1, uint32_t occ1, int32_t &lo, int32_t &ub)
{
    int32_t ua;
    uint32_t nva, nvb;
    spl_dbk_resolve_at(dbase, a - 1, first0, occ0, ua, nva);
    spl_dbk_resolve_at(dbase, b - 1, first1, occ1, ub, nvb);
    lo = ua + (int32_t)nva;
    return ub > lo;
}

// The span of a thread's simple reads: a true minimum and maximum, whatever the reads' order.  Without a simple read it stays as
// it began, a_min > b_max (a read has b >= a), which is how spl_span_any tells.
struct spl_simple_span {
    int32_t a_min, b_max;
};

SPL_HD void spl_span_begin(spl_simple_span &s)
{
    s.a_min = INT32_MAX;
    s.b_max = INT32_MIN;
}

SPL_HD bool spl_span_any(const spl_simple_span &s) { return s.a_min <= s.b_max; }

SPL_HD void spl_span_take(spl_simple_span &s, bool is_simple, uint32_t w0, uint32_t w1, int32_t shift)
{
    int32_t a, b;
    spl_simple_bases(w0, w1, shift, a, b);
    s.a_min = is_simple && a < s.a_min ? a : s.a_min;
    s.b_max = is_simple && b > s.b_max ? b : s.b_max;
}

// The thread is FLAGGED: the span's range, from the entries of a_min - 1 and b_max - 1, is not empty.  A thread that is not
// flagged has no simple read that counts for anything.
SPL_HD bool spl_span_flagged(int32_t dbase, const spl_simple_span &s, uint32_t first0, uint32_t occ0, uint32_t first1, uint32_t occ1)
{
    int32_t lo, ub;
    return spl_span_any(s) && spl_simple_range(dbase, s.a_min, s.b_max, first0, occ0, first1, occ1, lo, ub);
}

#endif // SPL_SIMPLE_SPAN_H
