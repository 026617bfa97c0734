// spl_sam.h -- SAM text on the device: the launchers of spl_sam.hip and what they exchange with the host (spl_capi.cpp: SamDecode; the line starts: LineIndex, for every text source).
//
// The second decoder behind spl_bam: where spl_inflate.hip makes POS, FLAG, the CIGAR offsets and words and the strand byte from
// the inflated BAM stream, these make them from the text an aligner writes, by the one rule of spl_sam_line.h.  Everything works
// on a WINDOW of the text in device memory that holds whole lines (spl_text_windows.h): bytes [lo, hi) of the file, `text` indexed with whole-file
// offsets (the caller passes the buffer's address minus the offset of its first byte, which is lo rounded down to 16: the
// kernels' 16-byte loads are aligned in the file and in memory alike).  Loads stay inside [lo & ~15, (hi + 15) & ~15): the
// buffer is SPL_SAM_PAD bytes longer than the window.
//
//   line starts   a wave per chunk of SPL_SAM_CHUNK bytes (chunk k = bytes [base + k * CHUNK, ...), base = lo & ~15): a count
//                 launch, the caller's prefix sum (spl_dev_launch_sort_scan), a fill launch.  A line belongs to the chunk its
//                 first byte lies in; line_start[] holds offsets from `base`, 32 bits (a window is below 2^32 bytes).
//   scan          a lane per line: the rule; kept or not and the op count per line, the filter's drop counters, the flagstat words
//                 per wave (spl_dev_launch_bam_flagstat_reduce's layout), the first declined line and its reason.
//   extract       after the caller's prefix sums of kept lines and ops: a lane per kept line writes the arrays.
//   order         whether reference ids or POS go down anywhere along the extracted records.
//
// Replaces `samtools view -b` in front of SpliSER_v0_1_8.py:422: the reference reads what samtools prints, text either way.
#ifndef SPL_SAM_H
#define SPL_SAM_H
#include <stddef.h>
#include <stdint.h>

#define SPL_SAM_CHUNK 16384u
#define SPL_SAM_PAD 16u
#define SPL_SAM_SCAN_LANES 256u // lanes of a workgroup of the scan (four waves: four rows of flagstat words)

// What a window's scan adds up (zeroed by the caller before every window except where it says otherwise).
struct spl_sam_counts {
    unsigned long long first_bad; // index of the first declined line of the window << 8 | its reason (atomicMin; set to ~0 first)
    uint32_t n_drop_flags, n_drop_mapq;
    uint32_t unordered;           // (spl_dev_launch_sam_order: not zeroed per window)
    uint32_t overflow;            // the extraction was asked to write beyond the room it was told of (never, unless the caller's sums are wrong)
};

#ifdef __cplusplus
extern "C" {
#endif
// chunk_count[k] = lines that begin in chunk k, k < n_chunks = spl_sam_chunks(lo, hi)
uint32_t spl_sam_chunks(uint64_t lo, uint64_t hi);
int spl_dev_launch_sam_line_count(const uint8_t *text, uint64_t lo, uint64_t hi, uint32_t *chunk_count, void *stream);
// chunk_end[k] = the inclusive prefix sums of the counts; line_start[i] = where line i begins, counted from lo & ~15
int spl_dev_launch_sam_line_fill(const uint8_t *text, uint64_t lo, uint64_t hi, const uint32_t *chunk_end, uint32_t *line_start, void *stream);
// Line i is [base + line_start[i], base + line_start[i + 1] - 1), the last one ends at last_end (hi, or hi - 1 when byte hi - 1 is
// its '\n').  names: the header's look-up table in device memory (spl_sam_line.h).  kept[i] = 1 when line i is extracted, n_ops[i]
// = its CIGAR ops (0 otherwise), line_tid[i] = its reference id.  fstat = null, or 16 words per wave of lines ((n_lines + 63) / 64
// rows).  counts: see above.
struct spl_sam_names;
int spl_dev_launch_sam_scan(const uint8_t *text, uint64_t base, const uint32_t *line_start, uint32_t n_lines, uint64_t last_end, const struct spl_sam_names *names,
                            uint32_t min_mapq, uint32_t require_flags, uint32_t exclude_flags, int want_xs, uint32_t *kept, uint32_t *n_ops, int32_t *line_tid,
                            uint32_t *fstat, struct spl_sam_counts *counts, void *stream);
// kept_end / ops_end: the inclusive prefix sums of kept / n_ops.  Kept line i is record rec0 + kept_end[i] - 1, its ops begin at
// op0 + ops_end[i] - (its count); cig_off[record + 1] = where they end.  Nothing is written at or beyond record cap_rec or op
// cap_ops (counts->overflow says so).  xs may be null.  ref_max_end[tid]: atomicMax of the reads' last bases.
int spl_dev_launch_sam_extract(const uint8_t *text, uint64_t base, const uint32_t *line_start, uint32_t n_lines, uint64_t last_end, const struct spl_sam_names *names,
                               uint32_t min_mapq, uint32_t require_flags, uint32_t exclude_flags, const uint32_t *kept_end, const uint32_t *ops_end, const int32_t *line_tid,
                               uint64_t rec0, uint64_t op0, uint64_t cap_rec, uint64_t cap_ops, int32_t *pos, uint16_t *flag, int32_t *tid, uint32_t *cig_off, uint32_t *cigar,
                               uint8_t *xs, unsigned long long *ref_max_end, struct spl_sam_counts *counts, void *stream);
// ... and with name_key: null (the call above), or one more array beside flag -- per kept line the key of its column 1
// (spl_name_key_sam): the kernel's instantiation for spl_bam_set_mate_keys.
int spl_dev_launch_sam_extract_keys(const uint8_t *text, uint64_t base, const uint32_t *line_start, uint32_t n_lines, uint64_t last_end, const struct spl_sam_names *names,
                                    uint32_t min_mapq, uint32_t require_flags, uint32_t exclude_flags, const uint32_t *kept_end, const uint32_t *ops_end, const int32_t *line_tid,
                                    uint64_t rec0, uint64_t op0, uint64_t cap_rec, uint64_t cap_ops, int32_t *pos, uint16_t *flag, int32_t *tid, uint32_t *cig_off, uint32_t *cigar,
                                    uint8_t *xs, uint64_t *name_key, unsigned long long *ref_max_end, struct spl_sam_counts *counts, void *stream);
// counts->unordered = 1 when (tid, pos) of any record in [first, first + n), first > 0: or of record first, is below its predecessor's
int spl_dev_launch_sam_order(const int32_t *tid, const int32_t *pos, uint64_t first, uint64_t n, struct spl_sam_counts *counts, void *stream);
// ---- for text that arrives without regard to lines (compressed SAM, spl_capi.cpp: SamZDecode) --------------------------------
// The inflated bytes of a window end where its last BGZF block ends.  *last (zero it first) = the offset behind the last '\n' of
// [lo, hi), unchanged where there is none: the window's lines end there, the bytes behind go to the front of the next window.
// `text` as above: indexed with offsets into the whole stream, address and offset equal modulo 16, readable in
// [lo & ~15, (hi + 15) & ~15).
int spl_dev_launch_sam_last_newline(const uint8_t *text, uint64_t lo, uint64_t hi, unsigned long long *last, void *stream);
// *first_long (set it to ~0 first) = the first of the window's lines that is longer than max_line bytes, its newline counted --
// such a line may lie INSIDE a window whose front is a carried piece (carry and new text are a window each).  end_off: where the
// last line ends, from the window's base, its newline counted if it has one.
int spl_dev_launch_sam_long_line(const uint32_t *line_start, uint32_t n_lines, uint32_t end_off, uint32_t max_line, uint32_t *first_long, void *stream);
#ifdef __cplusplus
}
#endif
#endif
