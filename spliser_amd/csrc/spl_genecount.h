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
// The two maps of a counting launch (gene maps; the bin maps of spl_exoncount.h have the same shape): n entries, start[] and
// code[] in device memory, in the coordinates of POS - 1 + shift; either map may have no entry.  stride / top are the launcher's:
// it fills them for the kernel (spl_genemap_dev.h), which takes the struct by value; a caller leaves them 0.
typedef struct spl_count_map {
    int64_t n;
    const int32_t *start;
    const uint32_t *code;
    uint32_t stride, top;
} spl_count_map;
typedef struct spl_count_maps {
    spl_count_map a, b;
} spl_count_maps;

// Workgroups of a launch over n reads.
uint32_t spl_dev_gene_grid(int64_t n);
// Adds what reads [first, first + n) of the arrays come to to counts (device memory, n_genes + 3 words of 64 bits: the genes, then
// no feature, ambiguous, not counted; the caller clears it).  stranded = 0: map a serves every read, 1 (fr) / 2 (rf): map a the
// '+' reads, map b the '-' reads.  n_rec / n_ops: the arrays' sizes, beyond which nothing is loaded.
int spl_dev_launch_gene_count(const spl_devreads *src, int64_t n_rec, int64_t n_ops, int64_t first, int64_t n, int32_t shift, int stranded, const spl_count_maps *maps, uint32_t n_genes,
                              unsigned long long *counts, void *stream);
// The same per FRAGMENT (spl_mate_rule.h): mate[r] = the mate of read first + r as an index within [0, n), or 0xFFFFFFFF (device
// memory, n words: spl_mates.hip); a read whose mate has a lower index adds nothing.
int spl_dev_launch_gene_count_fragments(const spl_devreads *src, int64_t n_rec, int64_t n_ops, int64_t first, int64_t n, int32_t shift, int stranded, const spl_count_maps *maps,
                                        uint32_t n_genes, const uint32_t *mate, unsigned long long *counts, void *stream);
#ifdef __cplusplus
}
#endif
#endif
