// spl_motif.h -- the launchers of spl_motif.hip: the reads' strand bytes from the genome's splice motifs (spl_reads_motif_strand),
// the motif codes of a junction table's rows (spl_junction_motifs).  The rule is spl_motif_rule.h.
#ifndef SPL_MOTIF_H
#define SPL_MOTIF_H
#include <stdint.h>

#include "spl_devpack.h"

#define SPL_MOTIF_TILE 256
#define SPL_MOTIF_GRID_MAX 2048

#ifdef __cplusplus
extern "C" {
#endif
// Reads [first, first + n) of the arrays, moved by `shift`, against the sequence of `length` bases packed at `packed` (spl_genome.h):
// xs[i] = the read's strand byte, out12 += the tally (SPL_MOTIF_TALLY sums in device memory).
int spl_dev_launch_motif_strand(const spl_devreads *src, uint8_t *xs, int64_t n_rec, int64_t n_ops, int64_t first, int64_t n, int32_t shift, const uint8_t *packed, int64_t length,
                                unsigned long long *out12, void *stream);
// code[i] = the motif code of row i (left[i], right[i]); all three in device memory.
int spl_dev_launch_junction_motifs(const int32_t *left, const int32_t *right, int64_t n, const uint8_t *packed, int64_t length, uint8_t *code, void *stream);
#ifdef __cplusplus
}
#endif
#endif
