// spl_genecount.h -- geometry and launcher of spl_genecount.hip: per-gene read counts over the BAM-native arrays of a fused read
// set (spl_gene_count; the rule is spl_genecount_rule.h, the histogram spl_genecount_wave.h).
//
// Replaces a second pass over the alignment file by `htseq-count` / `featureCounts`; the reference has no counterpart.
#ifndef SPL_GENECOUNT_H
#define SPL_GENECOUNT_H
#include <stdint.h>

#include "spl_devpack.h"

#define SPL_GENE_TILE 256       // reads a workgroup takes per grid-stride step, a read a lane
#define SPL_GENE_GRID_MAX 1024  // workgroups a launch has at most (four a CU); the rest is grid-stride
#define SPL_GENE_TOP 1024       // entries of a gene map's top level a workgroup keeps in LDS (4 KB a map, two maps)

#ifdef __cplusplus
extern "C" {
#endif
// Workgroups of a launch over n reads.
uint32_t spl_dev_gene_grid(int64_t n);
// Adds what reads [first, first + n) of the arrays come to to counts (device memory, n_genes + 3 words of 64 bits: the genes, then
// no feature, ambiguous, not counted; the caller clears it).  (n_a, a_start, a_code) / (n_b, b_start, b_code): the gene maps in
// device memory, in the coordinates of POS - 1 + shift, either may have no entry; stranded = 0: map a serves every read, 1 (fr) /
// 2 (rf): map a the '+' reads, map b the '-' reads.  n_rec / n_ops: the arrays' sizes, beyond which nothing is loaded.
int spl_dev_launch_gene_count(const spl_devreads *src, int64_t n_rec, int64_t n_ops, int64_t first, int64_t n, int32_t shift, int stranded, int64_t n_a, const int32_t *a_start,
                              const uint32_t *a_code, int64_t n_b, const int32_t *b_start, const uint32_t *b_code, uint32_t n_genes, unsigned long long *counts, void *stream);
// The same per FRAGMENT (spl_mate_rule.h): mate[r] = the mate of read first + r as an index within [0, n), or 0xFFFFFFFF (device
// memory, n words: spl_mates.hip); a read whose mate has a lower index adds nothing.
int spl_dev_launch_gene_count_fragments(const spl_devreads *src, int64_t n_rec, int64_t n_ops, int64_t first, int64_t n, int32_t shift, int stranded, int64_t n_a,
                                        const int32_t *a_start, const uint32_t *a_code, int64_t n_b, const int32_t *b_start, const uint32_t *b_code, uint32_t n_genes,
                                        const uint32_t *mate, unsigned long long *counts, void *stream);
#ifdef __cplusplus
}
#endif
#endif
