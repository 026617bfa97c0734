// spl_bam.h -- internal: what spl_capi.cpp needs from the BAM decoder (bam_reader.cpp).
#ifndef SPL_BAM_H
#define SPL_BAM_H

#include "../../include/spliser.h"
#include "spl_pack.h"

// ---- read filters (spl_bam_set_filter): samtools view's -q / -f / -F ---------------------------------------------------
// THE definition of which records a filter keeps: the host decoder (bam_reader.cpp) and the device's scan and walking extraction
// (spl_inflate.hip) all call this and nothing else.  A record that has a reference and a position is kept when none of its flag
// bits is excluded, all required ones are set, and its MAPQ -- a number: 255 passes every threshold, as in samtools -- is
// at least min_mapq.  All zero keeps every record.
struct spl_bam_filter { uint32_t min_mapq, require_flags, exclude_flags; };
#if defined(__HIPCC__)
#define SPL_BAM_HD __host__ __device__
#else
#define SPL_BAM_HD
#endif
#define SPL_BAM_KEPT 0
#define SPL_BAM_DROP_FLAGS 1 // (flags are tested first: a record that fails both ways counts here)
#define SPL_BAM_DROP_MAPQ 2
SPL_BAM_HD inline int spl_bam_filter_verdict(const spl_bam_filter &f, uint32_t flag, uint32_t mapq)
{
    if ((flag & f.exclude_flags) != 0u || (flag & f.require_flags) != f.require_flags) return SPL_BAM_DROP_FLAGS;
    return mapq >= f.min_mapq ? SPL_BAM_KEPT : SPL_BAM_DROP_MAPQ;
}

// ---- what a decoder is asked to do, and what it counted -----------------------------------------------------------------
// The file's decode switches, one record: set through spl_bam_set_filter / _aux_strand / _flagstat / _any_order while nobody
// decodes the file, fixed from then on.  A decoder takes ONE copy (spl_bam_get_opts) before its first record.  A new switch is
// one field here, one setter body (bam_reader.cpp) and one field of process.DecodeOptions.
struct spl_bam_decode_opts {
    spl_bam_filter filter = {0, 0, 0}; // which placed records are kept
    bool aux_strand = false;           // a strand byte per placed read beside its flag, from the aligner's XS:A tag
    bool flagstat = false;             // count the flagstat categories (spl_flagstat.h)
    bool mate_keys = false;            // a name key per placed read beside its flag (spl_mate_rule.h), for mate pairing
    bool any_order = false;            // the records may come in any order: the decoder hands every reference's reads out sorted by (POS, place in the file)
};
spl_bam_decode_opts spl_bam_get_opts(spl_bam *bam);
// What a decode counted, of a batch, a share or the whole file -- they add up.  dropped: the placed records the filter dropped by
// their flags / by their MAPQ (spl_bam_filter_counts).  fstat: the counters of spl_bam_flagstat, [2 c + q], over every record the
// filter keeps; zeros when nobody asked.  n_sorted: the reads put in order for any_order (0: the file was in order), by the
// device's sort (sorted_on_device = 1) or the host threads (0).
#define SPL_BAM_N_FSTAT 32 // 2 * SPL_FS_CATEGORIES of spl_flagstat.h, which includes this header: bam_reader.cpp asserts the two agree
struct spl_bam_totals {
    int64_t n_records = 0, dropped[2] = {0, 0}, fstat[SPL_BAM_N_FSTAT] = {0}, n_sorted = 0;
    int sorted_on_device = 0;
    void add(const spl_bam_totals &o)
    {
        n_records += o.n_records;
        dropped[0] += o.dropped[0];
        dropped[1] += o.dropped[1];
        for (int c = 0; c < SPL_BAM_N_FSTAT; ++c) fstat[c] += o.fstat[c];
        n_sorted += o.n_sorted;
        sorted_on_device |= o.sorted_on_device;
    }
};

// The reads of reference `tid` as a packer source: the decoder's own parts, in file order, nothing copied.  Waits until the
// reference is complete (spl_bam_wait_ref).  The views stay valid until spl_bam_release_ref(tid) or spl_bam_close.
int spl_bam_source(spl_bam *bam, int tid, splpack::Source *out, int64_t *max_end_out);

// ---- for the device decoder (spl_capi.cpp: spl_bam_decode_device) -------------------------------------------------------
// A file opened with spl_bam_open_deferred has its header read and nothing else started: the caller then either hands the decode
// to the host threads (spl_bam_start_host) or does it elsewhere and gives the result back (spl_bam_adopt).
struct spl_bam_block_info { uint64_t data_off; uint64_t uoff; uint32_t data_len, isize, crc; };
int spl_bam_walk_all(spl_bam *bam);                       // the whole block directory, now (SPL_OK or the file's error)
void spl_bam_walk_some(spl_bam *bam, size_t bytes);
bool spl_bam_walk_complete(const spl_bam *bam);
size_t spl_bam_block_count(const spl_bam *bam);
void spl_bam_block_get(const spl_bam *bam, size_t i, spl_bam_block_info *out);
const uint8_t *spl_bam_image(const spl_bam *bam, size_t *fsize_out);
int spl_bam_fd(const spl_bam *bam);                        // the open file (pread: bytes without touching the mapping's page tables)
uint64_t spl_bam_header_end(const spl_bam *bam);           // where the first record starts in the inflated stream
int spl_bam_thread_count(const spl_bam *bam);
// records, CIGAR ops and the inflated bytes they were counted in, sampled on the host at three places of blocks [b_lo, b_hi)
bool spl_bam_sample_density(spl_bam *bam, size_t b_lo, size_t b_hi, uint64_t *n_rec_out, uint64_t *n_ops_out, uint64_t *n_bytes_out);
// The placed records of the whole file in file order as four malloc'ed arrays (the file takes them over and frees them with
// free()); reference t has records [ref_first[t], ref_first[t] + ref_n[t]), cig_off holds n_total + 1 offsets into cigar.
// totals: what the decode counted over the whole file.
int spl_bam_adopt(spl_bam *bam, int32_t *pos, uint16_t *flag, uint32_t *cig_off, uint32_t *cigar, const int64_t *ref_first, const int64_t *ref_n,
                  const int64_t *ref_max_end, const spl_bam_totals &totals);
// what the device decoder keeps in device memory for the device packer: an opaque handle, freed with the file
void spl_bam_set_device_reads(spl_bam *bam, void *handle, void (*free_fn)(void *));
void *spl_bam_device_reads(spl_bam *bam, int tid);          // the handle that holds ALL of reference `tid` (null: none does -- no device decode, or the reference lies in several shares)
void *spl_bam_share_reads(spl_bam *bam, int share);         // what share `share` left in device memory (null: nothing)

// ---- a decode in SHARES: each device takes a stretch of the file, cut at ANY BGZF block ---------------------------------
// A share owns the records that BEGIN in blocks [block_lo, block_own) -- in the inflated stream: at offsets [u_lo, u_hi), both
// record boundaries the plan found by inflating a few blocks at every cut on the host -- and inflates blocks [block_lo,
// block_hi): the tail [block_own, block_hi) holds the end of its last record and nothing else of its own.  A reference's records
// may lie in several shares (counters are additive per read, SpliSER_v0_1_8.py:519-559: each device counts its stretch against the
// reference's whole site table); tid_lo <= tid < tid_hi are the references a share CAN hold records of (records without a
// reference count as n_ref; the last share's tid_hi = n_ref + 1).
struct spl_bam_share { uint64_t block_lo, block_hi; int32_t tid_lo, tid_hi; uint64_t block_own, u_lo, u_hi; };
// Cuts the file into up to n_shares stretches of equal size in file bytes.  The whole block directory is walked first.  Once per
// file; later calls return the first plan.
int spl_bam_share_get(spl_bam *bam, int k, spl_bam_share *out);
// A share's decoder is done: `handle` holds its records (share-local first record per reference in ref_first), or failed != 0.
// When the last share has reported the file is complete -- or, if one failed, everything is dropped and the host threads decode
// (and count: the shares' totals go with their reads).  totals: of the records that BEGIN in the share's own blocks, so that the
// shares' add up to the file's.
int spl_bam_share_done(spl_bam *bam, int k, void *handle, void (*free_fn)(void *), const int64_t *ref_first, const int64_t *ref_n,
                       const int64_t *ref_max_end, const spl_bam_totals &totals, int failed);
int spl_bam_shares_on_device(spl_bam *bam);
bool spl_bam_cancelled(const spl_bam *bam);                   // spl_bam_cancel was called: stop at the next window                  // 1: all shares reported and none failed
// spl_bam_adopt with null arrays = the reads stay on the device; `fetch(handle, ...)` brings malloc'ed host copies when a host-side
// reader asks for them (spl_bam_source, spl_bam_reads)
void spl_bam_set_fetch(spl_bam *bam, int (*fetch)(void *, int32_t **, uint16_t **, uint32_t **, uint32_t **));
void spl_bam_set_fetch_xs(spl_bam *bam, int (*fetch)(void *, uint8_t **)); // ... and of the strand bytes (null out = the handle has none)
void spl_bam_set_fetch_keys(spl_bam *bam, int (*fetch)(void *, uint64_t **)); // ... and of the name keys (null out = the handle has none)
int spl_bam_start_host(spl_bam *bam);                      // decode on the host's threads unless somebody decodes already
bool spl_bam_claim_for_device(spl_bam *bam);               // the device decoder takes the file (false: it is taken)
void spl_bam_note_decline(spl_bam *bam, const char *why); // why the device decoder leaves the file to the host threads
int spl_bam_device_gives_up(spl_bam *bam);                 // ... and hands it to the host threads after all
void spl_bam_linger(spl_bam *bam, double seconds);       // a decoder with only its clearing up left: until spl_bam_cancel, `seconds` at most

// ---- SAM text behind the same object (spl_sam_open; the line's rule: spl_sam_line.h) -------------------------------------
// false: the file is BGZF/BAM.  true: the alignment lines are the mapping's bytes [*begin_out, file size) (spl_bam_image), in front of
// them `*header_lines_out` header lines; names_out: the header's reference names as the rule looks them up (host memory, the file's),
// blob_bytes_out: the bytes of all names.  Null outputs are skipped.
// spl_bam_text_compression's values.  A compressed file's offsets (*begin_out below) are offsets in the INFLATED stream, and its
// mapping (spl_bam_image) holds the compressed bytes: BGZF blocks, all in the block directory (spl_bam_block_count / _get: walked
// by spl_sam_open), or gzip members for splsamz::Inflater (spl_sam_zhost.h).
#define SPL_TEXT_PLAIN 0
#define SPL_TEXT_BGZF 1
#define SPL_TEXT_GZIP 2
void spl_bam_note_text_blocks(spl_bam *bam, int64_t n);    // the BGZF blocks a device decoder inflated (spl_bam_text_blocks)
struct spl_sam_names;
bool spl_bam_text(const spl_bam *bam, uint64_t *begin_out, uint64_t *header_lines_out, spl_sam_names *names_out, size_t *blob_bytes_out);
// The rule declines the file at line `line_no` (1-based, header lines counted) for `reason` (SPL_SAM_*): the decode ends with
// SPL_ERR_FORMAT and spl_bam_decline_reason says "line N <reason>" -- whoever opened the file reads it as it was read before this
// decoder existed.  For the decoder that has the file (the device's, claim 1, or the host parser).
void spl_sam_fail(spl_bam *bam, uint64_t line_no, uint32_t reason);
// SPL_SAM_WINDOW_BYTES (64 .. 2^30; default 256 MiB): the bytes of text the device parses at a time, and for BOTH decoders the
// longest line, its newline counted, that the rule takes (SPL_SAM_LONG_LINE)
size_t spl_sam_window_bytes();

#endif
