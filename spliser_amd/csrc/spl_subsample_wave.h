// spl_subsample_wave.h -- the bodies of spl_subsample.hip's kernels, written against spl_wave.h's primitives: the same source runs as
// one wave per workgroup on the device and under tests/hostsim/wave_emul.h on a CPU (tests/test_subsample_host.py holds it against
// numpy's boolean mask).  The rule that keeps or drops a read is spl_subsample_rule.h.
//
// What is made: from the arrays of a fused read set (POS, FLAG, cig_off, the ragged CIGAR words, and the strand bytes and name keys
// where the set has them) a second set of arrays that holds the kept reads only, in their order -- an order-preserving stream
// compaction, out of place.  The reads of the set's segments are cut into TILES of TILE reads, a segment's tiles from its first read
// (no tile holds reads of two segments), the tiles of all segments numbered through; a tile is a wave's work.
//   1. tile_count   the tile's two totals: the reads it keeps and the ops of those reads
//   2. (the caller scans the two rows of totals: spl_sort.hip's device-wide scan)
//   3. tile_write   the rule once more; 64 reads a round in the arrays' order: a kept read's place is the tile's first place plus
//                   the kept reads of the rounds before plus the kept lanes in front of it (a ballot), its ops' place likewise by
//                   a prefix sum over the lanes; the read arrays are written side by side, cig_off as the running op offset, and
//                   the ops copied: a CIGAR of up to LANE_OPS ops by the read's own lane, a longer one by the whole wave, 64 ops a
//                   turn, so that one read of thousands of ops does not hold 63 lanes up
// No mark array is written and nothing here is atomic: the result is the same words from run to run.
#ifndef SPL_SUBSAMPLE_WAVE_H
#define SPL_SUBSAMPLE_WAVE_H
#include <stddef.h>
#include <stdint.h>

#include "spl_read_view.h"
#include "spl_subsample.h"
#include "spl_subsample_rule.h"
#include "spl_wave.h"

namespace splsub {

// Tile t of the call: the entries [*lo, *hi) of the arrays and the set's number of the read at *lo.  segs ascend by tile0; t lies
// in one of them.
WV_DEV void tile_range(const Seg *segs, uint32_t n_seg, uint64_t t, int64_t *lo, int64_t *hi, int64_t *base)
{
    uint32_t a = 0, b = n_seg;
    while (b - a > 1u) {
        const uint32_t mid = a + (b - a) / 2u;
        if (segs[mid].tile0 <= t) a = mid;
        else b = mid;
    }
    const Seg s = segs[a];
    const int64_t at = (int64_t)(t - s.tile0) * (int64_t)TILE;
    *lo = s.first + (at < s.n ? at : s.n);
    *hi = s.first + (at + (int64_t)TILE < s.n ? at + (int64_t)TILE : s.n);
    *base = s.base + (at < s.n ? at : s.n);
}

// THE KEEP DECISION is a parameter of the two bodies: keep(s, i, key, n_ops) for entry i of the arrays, whose key and op count the
// body has loaded.  HashKeep is the subsampling rule (POS and FLAG are read only for a read without a name); spl_dups_wave.h has
// the second one, a byte a read (spl_reads_dedup).
struct HashKeep {
    uint64_t salt, threshold;
    SPL_HD bool operator()(const Src &s, int64_t i, uint64_t key, uint32_t n_ops) const
    {
        if (key != 0ull) return (uint64_t)spl_subsample_draw(key, salt) < threshold;
        return spl_subsample_keep(0ull, (int64_t)s.pos[i], (uint32_t)s.flag[i], n_ops, salt, threshold);
    }
};

// Entry i of the arrays: its key, ops and the decision.
template <class Keep>
WV_DEV bool keep_at(const Src &s, int64_t i, const Keep &keep, uint64_t *key, uint32_t *c0, uint32_t *n_ops)
{
    *key = s.key[i];
    spl_ops_of(s.cig_off, i, s.n_ops, c0, n_ops);
    return keep(s, i, *key, *n_ops);
}

// Launch 1: tile t's totals -> reads_out[t], ops_out[t].
template <class Keep>
WV_DEV void tile_count_by(const Src &s, int64_t lo, int64_t hi, const Keep &keep, uint32_t *reads_out, uint32_t *ops_out)
{
    const uint32_t lane = wv::lane();
    uint32_t reads = 0u, ops = 0u;
#pragma unroll
    for (uint32_t r = 0; r < ROUNDS; ++r) {
        const int64_t i = lo + (int64_t)(64u * r + lane);
        if (i >= hi || i >= s.n_rec) continue; // (i < n_rec always: said for the memory's sake)
        uint64_t key;
        uint32_t c0, n_ops;
        if (keep_at(s, i, keep, &key, &c0, &n_ops)) { reads += 1u; ops += n_ops; }
    }
    const uint32_t reads_inc = wv::scan_add(reads), ops_inc = wv::scan_add(ops);
    if (lane == 63u) { *reads_out = reads_inc; *ops_out = ops_inc; }
}

WV_DEV void tile_count(const Src &s, int64_t lo, int64_t hi, uint64_t salt, uint64_t threshold, uint32_t *reads_out, uint32_t *ops_out)
{
    tile_count_by(s, lo, hi, HashKeep{salt, threshold}, reads_out, ops_out);
}

// Launch 3: the tile's kept reads to the places read0 .. of d, their ops to op0 ..; base: the source set's number of the read at lo.
template <class Keep>
WV_DEV void tile_write_by(const Src &s, const Dst &d, int64_t lo, int64_t hi, int64_t base, const Keep &keep_rule, uint32_t read0, uint32_t op0)
{
    const uint32_t lane = wv::lane();
    const uint64_t in_front = lane ? (~0ull >> (64u - lane)) : 0ull; // the lanes below this one
    for (uint32_t r = 0; r < ROUNDS; ++r) {
        if (lo + (int64_t)(64u * r) >= hi) break; // (uniform)
        const int64_t i = lo + (int64_t)(64u * r + lane);
        const bool have = i < hi && i < s.n_rec;
        uint64_t key = 0ull;
        uint32_t c0 = 0u, n_ops = 0u;
        const bool keep = have && keep_at(s, i, keep_rule, &key, &c0, &n_ops);
        const uint64_t kept = wv::ballot(keep);
        const uint32_t mine = keep ? n_ops : 0u;
        const uint32_t ops_inc = wv::scan_add(mine);
        const uint32_t ops_round = wv::shfl(ops_inc, 63u);
        const uint64_t at = (uint64_t)read0 + wv::popc64(kept & in_front);
        const uint32_t op_at = op0 + ops_inc - mine;
        const bool room = keep && (int64_t)at < d.n_rec && (int64_t)op_at + (int64_t)n_ops <= d.n_ops; // (always: the scan's totals are these counts' sums)
        if (room) {
            d.pos[at] = s.pos[i];
            d.flag[at] = s.flag[i];
            if (d.xs) d.xs[at] = s.xs[i];
            d.key[at] = key;
            if (d.index) d.index[at] = (uint32_t)(base + (int64_t)(64u * r + lane));
            d.cig_off[at] = op_at;
            if (n_ops <= LANE_OPS)
                for (uint32_t k = 0; k < n_ops; ++k) d.cigar[op_at + k] = s.cigar[c0 + k];
        }
        uint64_t longs = wv::ballot(room && n_ops > LANE_OPS);
        while (longs) { // (uniform) a long CIGAR: the wave copies it, 64 ops a turn
            const uint32_t l = wv::ffs64(longs);
            longs &= longs - 1ull;
            const uint32_t from = wv::readlane(c0, l), count = wv::readlane(n_ops, l), to = wv::readlane(op_at, l);
            for (uint32_t k = lane; k < count; k += 64u) d.cigar[to + k] = s.cigar[from + k];
        }
        read0 += wv::popc64(kept);
        op0 += ops_round;
    }
}

WV_DEV void tile_write(const Src &s, const Dst &d, int64_t lo, int64_t hi, int64_t base, uint64_t salt, uint64_t threshold, uint32_t read0, uint32_t op0)
{
    tile_write_by(s, d, lo, hi, base, HashKeep{salt, threshold}, read0, op0);
}

} // namespace splsub
#endif
