// spl_intron_wave.h -- how a team of lanes takes the trimmed depth of ONE intron (spl_intron.hip), written against spl_wave.h's
// primitives: the same source runs on the device and under tests/hostsim/wave_emul.h on a CPU (tests/test_intron_wave_host.py).
// The rule is spl_intron_rule.h's, which reaches the same numbers by sorting.
//
// A TEAM is a workgroup: one wave for an ordinary intron, SPL_INTRON_TEAM lanes for a long one (wv::sync is the workgroup's
// barrier; the lanes of every wave call each primitive from team-uniform control flow).  No per-base work: under a piece
// [ps, pe) the depth is constant between boundaries, so the piece is STRETCHES (depth, bases) -- the one that enters it from
// before ps (the depth of the last boundary at or before ps, 0 when there is none) and one per boundary inside it.  A binary
// search gives a piece's first boundary and another its last; up to PIECES of them are kept in shared memory, so an intron of few
// pieces is searched once and an intron of more in groups, again in every pass.  The lanes then stride over a piece's stretches.
//
// The two rank values D[lo] and D[hi - 1] are found by 8-bit radix passes from the top byte down: a pass adds every stretch whose
// bytes above agree with a rank's prefix to a 256-bucket histogram of bases in shared memory (two histograms once the prefixes
// differ: 2 KiB), and the bucket in which the rank falls is found by every wave alike -- four buckets a lane, a scan, a ballot.
// Bases are below 2^31 (pieces are disjoint and inside an int32 reference), so 32-bit buckets are exact.  A first pass ORs the
// depths: the radix starts at the highest byte any depth has, and an intron nobody covers ends there.  The sum is then
//     value_lo * (its ties inside [lo, hi)) + value_hi * (its ties inside) + the sum of depth * bases strictly between the two,
// the last by one more pass, in 64 bits; both tie counts fall out of the last radix pass.  Integers throughout.
#ifndef SPL_INTRON_WAVE_H
#define SPL_INTRON_WAVE_H
#include <stdint.h>

#include "spl_wave.h"

namespace splintron {

constexpr uint32_t PIECES = 64u;  // pieces whose searches shared memory keeps at a time
constexpr uint32_t BUCKETS = 256u;

struct Shared {
    uint32_t hist[2u * BUCKETS]; // bases per value of the pass's byte: for the rank lo, and for the rank hi - 1 once their prefixes differ
    int32_t first[PIECES];       // per kept piece: the boundary of its first stretch (-1: the depth 0 in front of the first boundary)
    uint32_t count[PIECES];      // and its number of stretches (>= 1)
    uint32_t total, covered, bits;
    uint64_t sum;
};

struct Depth { // bound_pos strictly ascending; depth[k] holds from pos[k] to pos[k + 1], the last to the end, 0 before pos[0]
    const int32_t *pos;
    const uint32_t *depth;
    int64_t n;
};
struct Pieces { // one intron's: disjoint, ascending, end > start
    const int32_t *start, *end;
    int64_t n;
};

// The boundaries at or before v (at_or_before) / before v: indices into pos.
WV_DEV int64_t bounds_upto(const Depth &d, int64_t v, bool at_or_before)
{
    int64_t a = 0, b = d.n; // pos[k] qualifies for k < a, does not for k >= b
    while (a < b) {
        const int64_t m = a + (b - a) / 2;
        const int64_t x = (int64_t)d.pos[m];
        if (at_or_before ? x <= v : x < v) a = m + 1;
        else b = m;
    }
    return a;
}

// The searches of the pieces [g, g + PIECES) of the intron, a piece a lane (the first PIECES lanes of the team).
WV_DEV void keep_pieces(uint32_t tid, const Depth &d, const Pieces &p, int64_t g, Shared *sh)
{
    if (tid < PIECES && g + (int64_t)tid < p.n) {
        const int64_t in_front = bounds_upto(d, (int64_t)p.start[g + tid], true), inside_end = bounds_upto(d, (int64_t)p.end[g + tid], false);
        sh->first[tid] = (int32_t)(in_front - 1);
        sh->count[tid] = (uint32_t)(inside_end - in_front + 1); // (start < end: every boundary at or before start is before end)
    }
}

// f(depth, bases) for every stretch of the intron, each from one lane of the team.  Called by the whole team.
template <class F>
WV_DEV void for_each_stretch(uint32_t tid, uint32_t team, const Depth &d, const Pieces &p, Shared *sh, F &&f)
{
    for (int64_t g = 0; g < p.n; g += PIECES) { // (uniform over the team)
        if (p.n > (int64_t)PIECES) { // (else the one group is kept from the start: team_intron)
            wv::sync();
            keep_pieces(tid, d, p, g, sh);
            wv::sync();
        }
        const uint32_t here = p.n - g < (int64_t)PIECES ? (uint32_t)(p.n - g) : PIECES;
        for (uint32_t q = 0; q < here; ++q) {
            const int64_t first = (int64_t)sh->first[q], ps = (int64_t)p.start[g + q], pe = (int64_t)p.end[g + q];
            const uint32_t count = sh->count[q];
            for (uint32_t j = tid; j < count; j += team) {
                const int64_t b = first + (int64_t)j; // -1 .. d.n - 1
                const int64_t from = b < 0 ? ps : (int64_t)d.pos[b];
                const int64_t to = b + 1 < d.n ? (int64_t)d.pos[b + 1] : pe;
                const int64_t s = from > ps ? from : ps, e = to < pe ? to : pe;
                f(b < 0 ? 0u : d.depth[b], (uint32_t)(e - s));
            }
        }
    }
}

// The bucket of hist (BUCKETS words) in which the 0-based rank falls: -> bucket, its bases in `count`, and rank becomes the rank
// inside the bucket.  Called by every wave of the team, all 64 lanes; rank is below the histogram's sum.
WV_DEV uint32_t find_rank(const uint32_t *hist, uint32_t &rank, uint32_t &count)
{
    const uint32_t lane = wv::lane();
    uint32_t h[4], own = 0u;
#pragma unroll
    for (uint32_t k = 0; k < 4u; ++k) { h[k] = hist[4u * lane + k]; own += h[k]; }
    const uint32_t incl = wv::scan_add(own), excl = incl - own;
    const bool here = rank >= excl && rank < incl;
    const uint64_t who = wv::ballot(here);
    uint32_t bucket = BUCKETS - 1u, r = 0u, c = 0u;
    if (here) {
        r = rank - excl;
        bool found = false;
#pragma unroll
        for (uint32_t k = 0; k < 4u; ++k)
            if (!found) {
                if (r < h[k]) { bucket = 4u * lane + k; c = h[k]; found = true; }
                else r -= h[k];
            }
    }
    const uint32_t src = who ? wv::ffs64(who) : 0u; // (one lane: the rank is below the sum)
    rank = wv::readlane(r, src);
    count = wv::readlane(c, src);
    return wv::readlane(bucket, src);
}

// One intron by one team (tid of team lanes, team a multiple of 64): out4 = L, covered, depth_n, depth_sum, written by lane 0.
WV_DEV void team_intron(uint32_t tid, uint32_t team, const Depth &d, const Pieces &p, uint32_t trim_percent, Shared *sh, int64_t *out4)
{
    wv::sync(); // (the team's last intron is done with the shared memory)
    if (tid == 0u) { sh->total = 0u; sh->covered = 0u; sh->bits = 0u; sh->sum = 0ull; }
    wv::sync();
    uint32_t bases = 0u;
    for (int64_t q = tid; q < p.n; q += team) bases += (uint32_t)(p.end[q] - p.start[q]);
    if (bases) wv::lds_add(&sh->total, bases);
    if (p.n <= (int64_t)PIECES) keep_pieces(tid, d, p, 0, sh);
    wv::sync();
    const uint32_t total = sh->total;
    const uint32_t lo = (uint32_t)((uint64_t)total * trim_percent / 100u), hi = total - lo;
    // which bits any depth has, and the covered bases
    uint32_t bits = 0u, covered = 0u;
    for_each_stretch(tid, team, d, p, sh, [&](uint32_t depth, uint32_t w) { bits |= depth; if (depth) covered += w; });
    if (bits) wv::lds_or(&sh->bits, bits);
    if (covered) wv::lds_add(&sh->covered, covered);
    wv::sync();
    bits = sh->bits;
    uint64_t sum = 0ull;
    if (total != 0u && bits != 0u) { // (uniform)
        uint32_t value_lo = 0u, value_hi = 0u, rank_lo = lo, rank_hi = hi - 1u, ties_lo = 0u, ties_hi = 0u;
        for (int byte = bits >> 24 ? 3 : bits >> 16 ? 2 : bits >> 8 ? 1 : 0; byte >= 0; --byte) {
            const uint32_t shift = 8u * (uint32_t)byte;
            const bool one = value_lo == value_hi; // the two ranks have followed one prefix so far: one histogram serves both
            for (uint32_t k = tid; k < 2u * BUCKETS; k += team) sh->hist[k] = 0u;
            wv::sync();
            for_each_stretch(tid, team, d, p, sh, [&](uint32_t depth, uint32_t w) {
                const uint32_t above = byte == 3 ? 0u : depth >> (shift + 8u), bucket = (depth >> shift) & (BUCKETS - 1u);
                if (above == value_lo) wv::lds_add(&sh->hist[bucket], w);
                if (!one && above == value_hi) wv::lds_add(&sh->hist[BUCKETS + bucket], w);
            });
            wv::sync();
            value_lo = value_lo << 8 | find_rank(sh->hist, rank_lo, ties_lo);
            value_hi = value_hi << 8 | find_rank(one ? sh->hist : sh->hist + BUCKETS, rank_hi, ties_hi);
            wv::sync(); // (every wave has read the histograms before the next pass clears them)
        }
        // D[lo .. hi): the ties of value_lo from rank_lo on, the ties of value_hi up to rank_hi, everything between the two values
        if (value_lo == value_hi) sum = (uint64_t)value_lo * (uint64_t)(hi - lo);
        else {
            sum = (uint64_t)value_lo * (uint64_t)(ties_lo - rank_lo) + (uint64_t)value_hi * (uint64_t)(rank_hi + 1u);
            if (value_hi - value_lo > 1u) {
                uint64_t between = 0ull;
                for_each_stretch(tid, team, d, p, sh, [&](uint32_t depth, uint32_t w) { if (depth > value_lo && depth < value_hi) between += (uint64_t)depth * (uint64_t)w; });
                if (between) wv::lds_add64(&sh->sum, between);
                wv::sync();
            }
        }
    }
    if (tid == 0u) {
        out4[0] = (int64_t)total;
        out4[1] = (int64_t)sh->covered;
        out4[2] = (int64_t)(hi - lo);
        out4[3] = (int64_t)(sum + sh->sum);
    }
}

} // namespace splintron
#endif
