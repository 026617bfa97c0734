// spl_dups.h -- geometry and launchers of spl_dups.hip: the duplicate marks of one segment of a fused read set
// (spl_reads_duplicates; the rule is spl_dup_rule.h, the sort between the stages is spl_sort.hip's) and the compaction of a set by
// those marks (spl_reads_dedup; the tile bodies are spl_subsample_wave.h's, the keep decision spl_dups_wave.h's).
//
// Replaces Picard MarkDuplicates / samtools markdup; the reference has no counterpart.
#ifndef SPL_DUPS_H
#define SPL_DUPS_H
#include <stdint.h>

#include "spl_subsample.h"

#define SPL_DUP_TILE 256 // reads (elements) a workgroup takes per grid-stride step, one a lane: spl_mates.h's geometry

#ifdef __cplusplus
extern "C" {
#endif
// Stage 1a: lead[r] = 1 where read first + r of the arrays LEADS a fragment, else 0 (r < n); counters[1] += the examined reads,
// [2] += the leaders with a mate, [3] += those without, [6] += the examined reads whose FLAG has 0x400.  mate: the segment's table.
// The caller turns lead into its inclusive prefix sums (spl_dev_launch_sort_scan): lead[n - 1] is then the number of fragments.
int spl_dev_launch_dup_lead(const splsub::Src *src, int64_t first, int64_t n, const uint32_t *mate, uint32_t *lead, unsigned long long *counters, void *stream);
// Stage 1b: the fragments in leader order: element scan[r] - 1 is leader r's -- its three words and r.  n_el: the room of the four.
int spl_dev_launch_dup_signature(const splsub::Src *src, int64_t first, int64_t n, const uint32_t *mate, const uint32_t *scan, int64_t n_el, uint64_t *w0, uint64_t *w1, uint64_t *w2,
                                 uint32_t *leader, void *stream);
// Stage 3, over the n_el elements sorted by (W0, W1, W2), stable: w0 / w1 in the sorted order, perm[j] = the element's number in
// leader order.  dup: the segment's n bytes, cleared by the caller; a duplicate sets its leader's and its mate's.
int spl_dev_launch_dup_mark(const uint64_t *w0, const uint64_t *w1, const uint32_t *perm, const uint32_t *leader, int64_t n_el, const uint32_t *mate, int64_t n, uint8_t *dup,
                            void *stream);
// Stage 4: every group's head adds one to hist[min(size, 256) - 1], size to hist[256] when size >= 256, and size - 1 to
// counters[4] (a pair) or counters[5] (a single).  hist: SPL_DUP_HIST 64-bit sums, cleared by the caller.
int spl_dev_launch_dup_groups(const uint64_t *w0, const uint64_t *w1, int64_t n_el, unsigned long long *hist, unsigned long long *counters, void *stream);
// The compaction by mark: spl_dev_launch_subsample_count / _write with the keep decision dup[i] == 0 (dup: a byte per entry of the
// arrays); the ends between them are spl_dev_launch_subsample_ends'.
int spl_dev_launch_dedup_count(const splsub::Src *src, const splsub::Seg *d_segs, uint32_t n_seg, uint64_t n_tiles, const uint8_t *dup, uint32_t *rows, void *stream);
int spl_dev_launch_dedup_write(const splsub::Src *src, const splsub::Dst *dst, const splsub::Seg *d_segs, uint32_t n_seg, uint64_t n_tiles, const uint8_t *dup, const uint32_t *rows,
                               void *stream);
#ifdef __cplusplus
}
#endif
#endif
