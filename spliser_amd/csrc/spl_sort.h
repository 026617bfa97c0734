// spl_sort.h -- the launchers of spl_sort.hip: a stable radix sort of the placed records of a BAM file that is not in coordinate
// order (spl_bam_set_any_order), and the gather of their arrays into the sorted order.  spl_sort_wave.h has the method.
//
// Replaces `samtools sort` in front of SpliSER_v0_1_8.py:422 (`samtools view BAM region` needs the index of a sorted file): the
// reference cannot read what the aligner wrote.
#ifndef SPL_SORT_H
#define SPL_SORT_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
// n keys (n <= 0xfffffff0: the payload is a 32-bit index) are cut into this many parts, a wave each ...
uint32_t spl_dev_sort_parts(uint64_t n);
// ... and a pass wants this many bytes of device memory beside the keys and payloads: the parts' histograms and the digits' totals
size_t spl_dev_sort_work_bytes(uint64_t n);
// the passes of a key whose low word (POS) has pos_bits bits that can differ and whose high word (reference id) has tid_bits:
// their shifts, least significant first, into shifts[0 .. 8) -> how many
uint32_t spl_dev_sort_passes(uint32_t pos_bits, uint32_t tid_bits, uint32_t *shifts);
// keys[i] = (uint32)tid[i] << 32 | (uint32)pos[i]
int spl_dev_launch_sort_make_keys(const int32_t *tid, const int32_t *pos, uint64_t n, uint64_t *keys, void *stream);
// One pass: the keys by their digit at `shift`, equal digits in the order they come in; a key's payload goes with it (perm_in =
// null: the payload of key i is i).  keys_out / perm_out must not be the inputs.  work: spl_dev_sort_work_bytes(n) bytes.
int spl_dev_launch_sort_pass(const uint64_t *keys_in, const uint32_t *perm_in, uint64_t n, uint32_t shift, uint64_t *keys_out, uint32_t *perm_out, void *work, void *stream);
// The fixed-size fields in the new order: record i of the output is record perm[i] of the input; tid from the sorted keys' high
// words.  xs / xs_out may be null.  cig_off_out[0] = 0 and cig_off_out[i + 1] = the op COUNT of output record i, which
// spl_dev_launch_sort_scan turns into the offsets.
int spl_dev_launch_sort_gather(const uint32_t *perm, const uint64_t *keys, uint64_t n, const int32_t *pos, const uint16_t *flag, const uint8_t *xs, const uint32_t *cig_off,
                               int32_t *pos_out, uint16_t *flag_out, uint8_t *xs_out, int32_t *tid_out, uint32_t *cig_off_out, void *stream);
// v[0 .. n) becomes its inclusive prefix sums (32 bits: the caller knows the total fits).  work: spl_dev_sort_work_bytes(n) bytes.
int spl_dev_launch_sort_scan(uint32_t *v, uint64_t n, void *work, void *stream);
// the CIGAR words, run by run: output record i's are cigar[cig_off[perm[i]] .. cig_off[perm[i] + 1]) (none for a read without a CIGAR)
int spl_dev_launch_sort_cigar(const uint32_t *perm, uint64_t n, const uint32_t *cig_off, const uint32_t *cigar, const uint32_t *cig_off_out, uint32_t *cigar_out, void *stream);
#ifdef __cplusplus
}
#endif
#endif
