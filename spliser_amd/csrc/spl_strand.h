// spl_strand.h -- geometry and launcher of spl_strand.hip: the tally of read strand against evidence strand over the BAM-native
// arrays of a fused read set (spl_strand_tally; the rule is spl_strand_rule.h).
//
// Replaces the IGV paragraph of the reference's README (is the library unstranded, fr or rf?); the reference has no counterpart.
#ifndef SPL_STRAND_H
#define SPL_STRAND_H
#include <stdint.h>

#include "spl_devpack.h"

#define SPL_STRAND_TILE 256       // reads a workgroup takes per grid-stride step, a read a lane
#define SPL_STRAND_GRID_MAX 1024  // workgroups a launch has at most (four a CU); the rest is grid-stride
#define SPL_STRAND_TOP 1024       // entries of the cover map's top level a workgroup keeps in LDS (4 KB)

#ifdef __cplusplus
extern "C" {
#endif
// Workgroups of a launch over n reads.
uint32_t spl_dev_strand_grid(int64_t n);
// Adds what reads [first, first + n) of the arrays say to out14 (device memory, 14 x 64 bits; the caller clears it): xs = their
// strand bytes or null; (n_cover, cover_start, cover_code) = the strand cover map in device memory, in the coordinates of
// POS + shift, or n_cover = 0.  n_rec / n_ops: the arrays' sizes, beyond which nothing is loaded.
int spl_dev_launch_strand_tally(const spl_devreads *src, const uint8_t *xs, int64_t n_rec, int64_t n_ops, int64_t first, int64_t n, int32_t shift, int64_t n_cover,
                                const int32_t *cover_start, const uint8_t *cover_code, unsigned long long *out14, void *stream);
#ifdef __cplusplus
}
#endif
#endif
