// spl_exoncount.h -- geometry and launcher of spl_exoncount.hip: per-exon-bin read counts over the BAM-native arrays of a fused
// read set (spl_exon_count; the rule is spl_exoncount_rule.h, the commit spl_exoncount_wave.h).
//
// Replaces a second pass over the alignment file by `featureCounts -f -O` / `dexseq_count.py`; the reference has no counterpart.
#ifndef SPL_EXONCOUNT_H
#define SPL_EXONCOUNT_H
#include <stdint.h>

#include "spl_devpack.h"
#include "spl_genecount.h" // spl_count_maps: a bin map is a gene map whose codes are bins'

#define SPL_EXON_TILE 256       // reads a workgroup takes per grid-stride step, a read a lane
#define SPL_EXON_GRID_MAX 1024  // workgroups a launch has at most (four a CU); the rest is grid-stride
#define SPL_EXON_TOP 1024       // entries of a bin map's top level a workgroup keeps in LDS (4 KB a map, two maps)

#ifdef __cplusplus
extern "C" {
#endif
// Workgroups of a launch over n reads.
uint32_t spl_dev_exon_grid(int64_t n);
// Adds what reads [first, first + n) of the arrays come to to counts (device memory, n_bins + 4 words of 64 bits: the bins, then
// counted, no feature, ambiguous, not counted; the caller clears it).  maps: the bin maps; bin_gene: n_bins genes in device memory;
// stranded = 0: map a serves every read, 1 (fr) / 2 (rf): map a the '+' reads, map b the '-' reads.  n_rec / n_ops: the arrays'
// sizes, beyond which nothing is loaded.
int spl_dev_launch_exon_count(const spl_devreads *src, int64_t n_rec, int64_t n_ops, int64_t first, int64_t n, int32_t shift, int stranded, const spl_count_maps *maps, uint32_t n_bins,
                              const uint32_t *bin_gene, unsigned long long *counts, void *stream);
// The same per FRAGMENT (spl_exonfragment_rule.h): mate = the segment's mate table in device memory, n words, indexes relative to
// `first`; a pair of mates adds one to every distinct bin of both reads, and one to one verdict counter.
int spl_dev_launch_exon_count_fragments(const spl_devreads *src, int64_t n_rec, int64_t n_ops, int64_t first, int64_t n, int32_t shift, int stranded, const spl_count_maps *maps,
                                        uint32_t n_bins, const uint32_t *bin_gene, const uint32_t *mate, unsigned long long *counts, void *stream);
#ifdef __cplusplus
}
#endif
#endif
