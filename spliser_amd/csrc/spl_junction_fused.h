// spl_junction_fused.h -- geometry and launchers of the junction kernel of a fused read set (spl_junctions.hip).
#ifndef SPL_JUNCTION_FUSED_H
#define SPL_JUNCTION_FUSED_H
#include <stdint.h>

#include "spl_devpack.h"

// A tile of reads, a read a lane
#define SPL_JTILE 256
#define SPL_JSTAGE 2048                  // words of ops staged per tile: eight a read on average, 8 KB
#define SPL_JSCAN 16                     // ops a lane looks through for an N op; a longer read is listed without looking

#ifdef __cplusplus
extern "C" {
#endif
int spl_dev_launch_junctions_count(const spl_devreads *src, const spl_layout_chunk *chunks, uint32_t n_chunks, uint32_t min_intron, uint32_t max_intron,
                                   unsigned long long *n_count, void *stream);
int spl_dev_launch_junctions_fused(const spl_devreads *src, int64_t n_rec, int64_t n_ops, const spl_layout_chunk *chunks, uint32_t n_chunks,
                                   int stranded, uint32_t min_anchor, uint32_t min_intron, uint32_t max_intron, unsigned long long *keys,
                                   uint32_t *vals, uint32_t n_slots, unsigned long long *out_keys, uint32_t *out_vals, uint32_t *n_out,
                                   int32_t *err, const uint8_t *xs, void *stream); // xs: the reads' strand bytes, with stranded = 3 and only then
// ... per fragment (spl_junctionfragment_rule.h): mates = the set's mate table, a word a read of the arrays; seg_first / seg_n (device
// memory, n_segs >= 1 entries): the set's segments, ascending in their first read, each inside the arrays.
int spl_dev_launch_junctions_fused_fragments(const spl_devreads *src, int64_t n_rec, int64_t n_ops, const spl_layout_chunk *chunks, uint32_t n_chunks, int stranded,
                                             uint32_t min_anchor, uint32_t min_intron, uint32_t max_intron, unsigned long long *keys, uint32_t *vals, uint32_t n_slots,
                                             unsigned long long *out_keys, uint32_t *out_vals, uint32_t *n_out, int32_t *err, const uint8_t *xs, const uint32_t *mates,
                                             const int64_t *seg_first, const int64_t *seg_n, uint32_t n_segs, void *stream);
#ifdef __cplusplus
}
#endif
#endif
