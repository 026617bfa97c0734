// spl_coverage.h -- geometry and launchers of spl_coverage.hip: per-base read depth of one reference from the BAM-native arrays of a
// fused read set, as runs (spl_coverage; the rule is spl_coverage_rule.h).
//
// Replaces `samtools sort` + `index` for IGV, or `bedtools genomecov -bg -split` / deepTools `bamCoverage`, in front of the look at
// the alignments the reference's README asks for; the reference has no counterpart.
#ifndef SPL_COVERAGE_H
#define SPL_COVERAGE_H
#include <stdint.h>

#include "spl_devpack.h"

#define SPL_COV_TILE 256          // mark: reads a workgroup takes per grid-stride step, a read a lane
#define SPL_COV_GRID_MAX 1024     // mark: workgroups a launch has at most (four a CU); the rest is grid-stride
#define SPL_COV_POS_TILE 1024     // compact: positions a workgroup takes per step, four a lane (one 16-byte load)
#define SPL_COV_POS_GRID_MAX 4096 // compact: workgroups a launch has at most

#ifdef __cplusplus
extern "C" {
#endif
// Workgroups of a mark launch over n reads / of a compact launch over n_tiles tiles.
uint32_t spl_dev_cov_grid(int64_t n);
uint32_t spl_dev_cov_pos_grid(int64_t n_tiles);
// Words the difference array of `length` positions needs: length + 1, up to whole tiles (a lane's load never leaves it).
int64_t spl_dev_cov_diff_words(int64_t length);
// mark: reads [first, first + n) of the arrays add +1 / -1 (mod 2^32) at the ends of their clipped blocks to diff (zeroed by the
// caller, spl_dev_cov_diff_words(length) words), and to out4 (device memory, 4 x 64 bits, cleared by the caller): reads seen,
// reads that contributed, reads past the end, covered bases.  n_rec / n_ops: the arrays' sizes, beyond which nothing is loaded.
int spl_dev_launch_cov_mark(const spl_devreads *src, int64_t n_rec, int64_t n_ops, int64_t first, int64_t n, int32_t shift, int64_t length, int stranded, int strand,
                            uint32_t *diff, unsigned long long *out4, void *stream);
// mark, per fragment (spl_covfragment_rule.h): the same over the segment's mate table -- mate: n words of device memory, a read's
// mate within [0, n) or SPL_MATE_NONE.  out5: the four sums where spl_dev_launch_cov_mark has them, and [4] the pairs whose union
// was taken.
int spl_dev_launch_cov_mark_fragments(const spl_devreads *src, int64_t n_rec, int64_t n_ops, int64_t first, int64_t n, int32_t shift, int64_t length, int stranded, int strand,
                                      const uint32_t *mate, uint32_t *diff, unsigned long long *out5, void *stream);
// compact, pass 1: tile_count[t] = the non-zero words of diff among the positions [t * SPL_COV_POS_TILE, ...) below length.
int spl_dev_launch_cov_count(const uint32_t *diff, int64_t length, uint32_t *tile_count, void *stream);
// compact, pass 2: tile_sum = the INCLUSIVE prefix sums of tile_count; the non-zero words below length go to (pos, delta) in
// ascending order of position, n_out of them (nothing is written beyond).
int spl_dev_launch_cov_emit(const uint32_t *diff, int64_t length, const uint32_t *tile_sum, int32_t *pos, uint32_t *delta, int64_t n_out, void *stream);
#ifdef __cplusplus
}
#endif
#endif
