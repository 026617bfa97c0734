// spl_mates.h -- geometry and launchers of spl_mates.hip: the mate table of one segment of a fused read set, from the reads' name
// keys (spl_mate_table; the rule is spl_mate_rule.h, the sort between the two stages is spl_sort.hip's).
//
// Replaces the name-sorted pass of `htseq-count` / `featureCounts -p`; the reference has no counterpart.
#ifndef SPL_MATES_H
#define SPL_MATES_H
#include <stdint.h>

#include "spl_devpack.h"

#define SPL_MATE_TILE 256       // reads (elements) a workgroup takes per grid-stride step, one a lane
#define SPL_MATE_GRID_MAX 1024  // workgroups a launch has at most (four a CU); the rest is grid-stride
#define SPL_MATE_COUNTERS 3     // pairable reads, paired reads (twice the pairs), pairable reads without a mate whose 0x8 is clear

#ifdef __cplusplus
extern "C" {
#endif
// Workgroups of a launch over n reads (elements).
uint32_t spl_dev_mate_grid(int64_t n);
// Stage 1a: mark[r] = 1 where read first + r of the arrays is pairable, else 0 (r < n).  The caller turns mark into its inclusive
// prefix sums (spl_dev_launch_sort_scan): mark[n - 1] is then the number of pairable reads.
int spl_dev_launch_mate_mark(const spl_devreads *src, const uint64_t *name_key, int64_t n_rec, int64_t first, int64_t n, uint32_t *mark, void *stream);
// Stage 1b: the pairable reads, in the segment's order, as (sort key, index within the segment): element scan[r] - 1 is read r's.
int spl_dev_launch_mate_compact(const spl_devreads *src, const uint64_t *name_key, int64_t n_rec, int64_t first, int64_t n, const uint32_t *scan, uint64_t *keys, uint32_t *index,
                                void *stream);
// Stage 3, over the n_pairable elements sorted by key (stable): mate[index[j]] = the partner's read for every element that has one
// (mate: n words the caller has filled with 0xFFFFFFFF), counters[1] += the elements with a partner, counters[2] += those without
// whose read's flag (flag: the segment's, by the same index) has 0x8 clear.
int spl_dev_launch_mate_pair(const uint64_t *keys, const uint32_t *index, int64_t n_pairable, const uint16_t *flag, int64_t n, uint32_t *mate, unsigned long long *counters,
                             void *stream);
// out[i] = in[perm[i]] for i < n: the name keys into the order of a sort (spl_bam_set_any_order).
int spl_dev_launch_gather_u64(const uint32_t *perm, uint64_t n, const uint64_t *in, uint64_t *out, void *stream);
#ifdef __cplusplus
}
#endif
#endif
