// spl_intron.h -- geometry and launcher of spl_intron.hip: the trimmed depth of annotated introns over the depth boundaries the
// coverage stages leave on the device (spl_intron_depth; the rule is spl_intron_rule.h, the team's body spl_intron_wave.h).
//
// Replaces IRFinder / iREAD over the alignment file; the reference has no counterpart.
#ifndef SPL_INTRON_H
#define SPL_INTRON_H
#include <stdint.h>

#define SPL_INTRON_LONG_BASES 16384 // an intron of this many measurable bases or more is a LONG one: a team of its own
#define SPL_INTRON_TEAM 512         // lanes of a long intron's team (one workgroup); every other intron has one wave
#define SPL_INTRON_GRID_MAX 8192    // workgroups a launch has at most (32 waves a CU); the rest is grid-stride

#ifdef __cplusplus
extern "C" {
#endif
// Workgroups of a launch over n introns.
uint32_t spl_dev_intron_grid(int64_t n);
// The introns items[0 .. n_items) (indices into piece_off), each by one team of `team` lanes (64 or SPL_INTRON_TEAM): intron i has
// the pieces piece_off[i] .. piece_off[i + 1] of (piece_start, piece_end), disjoint and ascending; (bound_pos, bound_depth): n_bound
// boundaries, positions strictly ascending.  out: 4 x 64 bits per intron (at its index), L, covered, depth_n, depth_sum.  All in
// device memory.
int spl_dev_launch_intron(int team, const int32_t *bound_pos, const uint32_t *bound_depth, int64_t n_bound, const int64_t *piece_off, const int32_t *piece_start,
                          const int32_t *piece_end, const uint32_t *items, int64_t n_items, int trim_percent, int64_t *out, void *stream);
#ifdef __cplusplus
}
#endif
#endif
