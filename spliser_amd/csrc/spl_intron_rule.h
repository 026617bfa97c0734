// spl_intron_rule.h -- the depth of ONE intron over its measurable pieces, as straight-line C++: the rule of spl_intron_depth (the
// `intronretention` command).  No HIP intrinsics: the host compiles it (spl_intron_depth_host, tests/hostsim/intron_rule_asan.cpp);
// the kernel (spl_intron.hip, spl_intron_wave.h) reaches the same numbers by another method, and the product never calls this one.
//
// Replaces IRFinder / iREAD over the file this library has just decoded: the trimmed depth of every annotated intron.  The
// reference has no counterpart.
//
// The DEPTH is given as boundaries: bound_pos strictly ascending, bound_depth[k] holds for bound_pos[k] <= p < bound_pos[k + 1]
// (the last one to the end; 0 before the first) -- what spl_coverage's stages leave on the device.  An intron's measurable PIECES
// are disjoint [start, end), strictly ascending, inside [0, length]; L = the sum of their lengths.  With D the ascending multiset
// of the depth at each of the L bases and t = trim_percent (0..49):
//     lo = (L * t) / 100,  hi = L - lo,  depth_n = hi - lo,  depth_sum = the sum of D[lo .. hi),  covered = #{d > 0}.
// All int64, exact while depth_sum < 2^63; t = 0 is the plain sum.  L = 0: four zeros.
#ifndef SPL_INTRON_RULE_H
#define SPL_INTRON_RULE_H

#include <stdint.h>

#include <algorithm>
#include <utility>
#include <vector>

#define SPL_INTRON_TRIM_MAX 49
#define SPL_INTRON_OUT 4 // per intron: L, covered, depth_n, depth_sum

// The first flaw of the pieces [first, last) of one intron: -1 none; else the piece's index, *why = 0 end <= start, 1 outside
// [0, length], 2 not strictly ascending and disjoint (it begins before the piece in front of it ends).
inline int64_t spl_intron_piece_flaw(const int32_t *piece_start, const int32_t *piece_end, int64_t first, int64_t last, int64_t length, int *why)
{
    for (int64_t k = first; k < last; ++k) {
        const int64_t s = piece_start[k], e = piece_end[k];
        if (e <= s) { *why = 0; return k; }
        if (s < 0 || e > length) { *why = 1; return k; }
        if (k > first && s < (int64_t)piece_end[k - 1]) { *why = 2; return k; }
    }
    return -1;
}

// The first boundary that is not beyond the one in front of it, or -1.
inline int64_t spl_intron_bound_flaw(int64_t n_bound, const int32_t *bound_pos)
{
    for (int64_t k = 1; k < n_bound; ++k)
        if (bound_pos[k] <= bound_pos[k - 1]) return k;
    return -1;
}

// One intron (its pieces and the boundaries as above, all checked by the caller): (depth, bases) of every stretch of equal depth
// under a piece are collected, sorted by depth and walked once.  out4 = L, covered, depth_n, depth_sum.
inline void spl_intron_depth_of(int64_t n_bound, const int32_t *bound_pos, const uint32_t *bound_depth, int64_t n_pieces, const int32_t *piece_start, const int32_t *piece_end,
                                int trim_percent, int64_t *out4)
{
    std::vector<std::pair<uint32_t, int64_t>> runs; // (depth, bases)
    int64_t total = 0, covered = 0;
    for (int64_t q = 0; q < n_pieces; ++q) {
        const int64_t ps = piece_start[q], pe = piece_end[q];
        int64_t k = std::upper_bound(bound_pos, bound_pos + n_bound, (int32_t)ps) - bound_pos; // the first boundary beyond ps
        int64_t at = ps;
        uint32_t depth = k > 0 ? bound_depth[k - 1] : 0u;
        while (at < pe) {
            const int64_t next = k < n_bound && (int64_t)bound_pos[k] < pe ? (int64_t)bound_pos[k] : pe;
            runs.emplace_back(depth, next - at);
            if (depth) covered += next - at;
            total += next - at;
            at = next;
            if (k < n_bound) depth = bound_depth[k];
            ++k;
        }
    }
    std::sort(runs.begin(), runs.end());
    const int64_t lo = total * (int64_t)trim_percent / 100, hi = total - lo;
    uint64_t sum = 0;
    int64_t seen = 0; // bases of D in front of this run
    for (const std::pair<uint32_t, int64_t> &r : runs) {
        const int64_t a = std::max(seen, lo), b = std::min(seen + r.second, hi);
        if (b > a) sum += (uint64_t)r.first * (uint64_t)(b - a);
        seen += r.second;
    }
    out4[0] = total;
    out4[1] = covered;
    out4[2] = hi - lo;
    out4[3] = (int64_t)sum;
}

#endif // SPL_INTRON_RULE_H
