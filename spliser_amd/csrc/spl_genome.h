// spl_genome.h -- a FASTA's sequences packed in device memory: the launchers of spl_genome.hip and what they exchange with the
// host (spl_capi.cpp: GenomeLoad).  The rule is spl_motif_rule.h.
//
// STORED FORM: two base codes a byte; base p (1-based) of a sequence is nibble p - 1 from the sequence's first byte, the low
// nibble first.  A sequence takes 16 * ceil(length / 32) bytes and starts on a 16-byte boundary: no byte belongs to two sequences,
// the nibbles behind a sequence's last base are 0.
//
// A WINDOW of the text in device memory holds whole lines (bytes [lo, hi) of the file, `text` indexed with whole-file offsets as
// in spl_sam.h; the windows are spl_text_windows.h's, the lines are found by the LineIndex the SAM decoders use).  Then
//   classify   a lane per line: header, bases or empty (hdr[i] = 1 for a header), the bases of the line (nb[i]), the first line
//              the rule declines;
//   (the caller's inclusive prefix sums of nb and hdr: spl_dev_launch_sort_scan)
//   headers    a lane per line: header number k of the window leaves where its name is in the file, the name's length and the
//              window's bases in front of it; a line of bases in front of the file's first header is declined here;
//   (the host closes the sequences the headers end, gives every piece of a sequence in the window -- a SEGMENT -- its place)
//   pack       OUTPUT-driven: a lane owns 32 consecutive bases of a sequence, one 16-byte store; it finds its segment and its first
//              line by binary search, loads the lines' bytes, codes them, stores once.  No two lanes write one byte.  The one
//              16-byte word a window's first segment shares with the window before is read back by the lane that owns it (the
//              launches of a load are ordered on one stream): the join of a sequence across windows.
#ifndef SPL_GENOME_H
#define SPL_GENOME_H
#include <stddef.h>
#include <stdint.h>

struct spl_genome_header { uint64_t name_at; uint32_t name_len, bases_before, line, pad; }; // name_at: file offset; bases_before: the window's bases in front of the header; line: of the window
// A piece of one sequence inside a window: the window's bases [wb, wb + n) are bases seq_first + 1 .. seq_first + n of the sequence
// whose first byte is at dst; group_first: the 32-base groups of the window's segments in front of this one.
struct spl_genome_segment { uint64_t dst, seq_first; uint32_t wb, n, group_first, pad; };

struct spl_genome_counts { unsigned long long first_bad; }; // index of the first declined line of the window << 8 | the reason (atomicMin; ~0 first)

#ifdef __cplusplus
extern "C" {
#endif
// Line i is [base + line_start[i], base + line_start[i + 1] - 1) and has a newline; the last one ends at last_end (hi when it has none).
int spl_dev_launch_genome_classify(const uint8_t *text, uint64_t base, const uint32_t *line_start, uint32_t n_lines, uint64_t last_end, uint64_t hi, uint32_t *nb, uint32_t *hdr,
                                   struct spl_genome_counts *counts, void *stream);
// nb_end / hdr_end: the inclusive prefix sums.  open_before: a header stood in an earlier window.
int spl_dev_launch_genome_headers(const uint8_t *text, uint64_t base, const uint32_t *line_start, uint32_t n_lines, uint64_t last_end, uint64_t hi, const uint32_t *nb_end,
                                  const uint32_t *hdr_end, int open_before, struct spl_genome_header *headers, struct spl_genome_counts *counts, void *stream);
// segs[n_segs] in device memory, n_groups = all their groups; store: the genome's bytes, store_bytes of them (nothing is written beyond).
int spl_dev_launch_genome_pack(const uint8_t *text, uint64_t base, const uint32_t *line_start, uint32_t n_lines, const uint32_t *nb_end, const struct spl_genome_segment *segs,
                               uint32_t n_segs, uint32_t n_groups, uint8_t *store, uint64_t store_bytes, void *stream);
#ifdef __cplusplus
}
#endif
#endif
