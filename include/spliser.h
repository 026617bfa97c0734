/*
 * spliser.h -- C ABI of libspliser_hip.so, the MI355X (gfx950) implementation of the hot path of
 * SpliSER v0.1.8 `process`: per-splice-site beta1 / beta2Simple / double-count read classification
 * and the beta2 + SSE vector pass.
 *
 * The reference (pure Python) has no FFI; the seam this library replaces is the batch
 *
 *     processSites(inBAM, qChrom, isStranded, strandedType, isbeta2Cryptic)   SpliSER_v0_1_8.py:681-692
 *       = for every site: checkBam(...)                                       SpliSER_v0_1_8.py:408-559
 *         for every site: findBeta2Counts(...); calculateSSE(...)             SpliSER_v0_1_8.py:581-639
 *
 * and, upstream of it, the per-site `samtools view` child process (SpliSER_v0_1_8.py:422), which is
 * replaced by one whole-file BAM decode into structure-of-arrays buffers (spl_bam_*).
 *
 * Conventions
 *   - every function returns 0 on success and a negative spl_status on failure; the message of the
 *     last failure on the calling thread is available from spl_last_error();
 *   - the caller owns every buffer it passes in; the library never keeps a caller pointer past the
 *     return of the call that received it;
 *   - a spl_ctx is bound to one GPU and one HIP stream; calls on different contexts may run
 *     concurrently from different threads, calls on the same context must be serialised;
 *   - there is NO CPU fallback: spl_create() fails when no gfx950 device is visible.
 *
 * Coordinates: all positions are the reference's integers -- 1-based SAM POS for reads; for sites the
 * values computed at SpliSER_v0_1_8.py:275-276 (left site = last exonic base, right site = last
 * intronic base, both 1-based), so a CIGAR N op of length d ending at cur gives lSite = cur-d-1,
 * rSite = cur-1 (SpliSER_v0_1_8.py:482-483) and equality tests are direct.  One call covers one
 * *shard*: a single int32 coordinate space (one chromosome, or several chromosomes the host has laid
 * side by side with offsets -- see spliser_amd/shard.py); every coordinate must stay at or below 2^31-67.
 */
#ifndef SPLISER_H
#define SPLISER_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SPL_ABI_VERSION 1

typedef enum spl_status {
    SPL_OK = 0,
    SPL_ERR_ARG = -1,       /* bad argument (null pointer, negative size, unsorted table, ...)   */
    SPL_ERR_NO_DEVICE = -2, /* no usable gfx950 device / HIP runtime failure at start-up          */
    SPL_ERR_HIP = -3,       /* a HIP call failed; message carries hipGetErrorString               */
    SPL_ERR_IO = -4,        /* file missing / unreadable / truncated                              */
    SPL_ERR_FORMAT = -5,    /* not BGZF/BAM, corrupt block, unsupported CIGAR op                   */
    SPL_ERR_RANGE = -6,     /* coordinate overflow: a read or site exceeds the int32 shard space   */
    SPL_ERR_NOMEM = -7
} spl_status;

typedef struct spl_ctx spl_ctx;       /* one GPU + one stream                                       */
typedef struct spl_dsites spl_dsites; /* a site table resident in HBM (+ its output counters)       */
typedef struct spl_dreads spl_dreads; /* a read set resident in HBM                                  */
typedef struct spl_bam spl_bam;       /* an opened + decoded BAM file                                */

/* Site table of one shard: the state the reference keeps in Site objects
 * (Gene_Site_Iter_Graph_v0_1_8.py:98-120) after findAlphaCounts + findCompetitorPos
 * (SpliSER_v0_1_8.py:227-372), flattened to SoA + CSR.  Row order = Site.__lt__ order
 * (Gene_Site_Iter_Graph_v0_1_8.py:123-136): ascending pos, '+' before '-' at equal pos. */
typedef struct spl_sites {
    int64_t n_sites;
    const int32_t *pos;        /* [n_sites]   Site.pos, non-decreasing                               */
    const uint8_t *strand;     /* [n_sites]   Site.strand as ASCII ('+', '-', anything else = none)  */
    const uint32_t *part_off;  /* [n_sites+1] CSR offsets into part_*                                */
    const int32_t *part_pos;   /* [n_part]    keys of Site.PartnerCounts, insertion order            */
    const int32_t *part_site;  /* [n_part]    row of that partner in this table, -1 when absent (the
                                              one-way lists of combine's query tables); NULL: spl_sse
                                              is unavailable.  The range kernel takes either.        */
    const uint32_t *comp_off;  /* [n_sites+1] CSR offsets into comp_pos                              */
    const int32_t *comp_pos;   /* [n_comp]    Site.CompetitorPos (sorted unique)                     */
    const int64_t *alpha;      /* [n_sites]   Site.alphaCounts[sample]; may be NULL for spl_count    */
    const int64_t *edge_cnt;   /* [n_part]    Site.PartnerCounts[part_pos][sample]; may be NULL for
                                              spl_count                                             */
} spl_sites;

/* Reads of one shard, in file order (coordinate-sorted input gives the best locality but is not
 * required for correctness).  This is exactly what checkBam consumes from each SAM line:
 * column 2 (flag), column 4 (POS), column 6 (CIGAR)  -- SpliSER_v0_1_8.py:434-437. */
typedef struct spl_reads {
    int64_t n_reads;
    const int32_t *pos;       /* [n_reads]   1-based leftmost position (SAM POS)                     */
    const uint16_t *flag;     /* [n_reads]   SAM FLAG                                                */
    const uint32_t *cig_off;  /* [n_reads+1] offsets into cigar; cig_off[0] == 0                     */
    const uint32_t *cigar;    /* [cig_off[n_reads]] BAM-native ops: len<<4 | op, op = MIDNSHP=X 0..8 */
} spl_reads;

typedef struct spl_opts {
    int32_t stranded;     /* 0 = unstranded, 1 = "fr", 2 = "rf"   (check_strand, SpliSER_v0_1_8.py:374-406) */
    int32_t combine_mode; /* 0 = `process`; 1 = `combine`/`combineShallow`: a flanking read also counts
                             toward beta2Simple (SpliSER_v0_1_8.py:529-536)                            */
    int32_t flags;        /* SPL_OPT_* bits                                                            */
} spl_opts;

/* Force the literal per-(read, site) kernel: an on-device cross-check (tests).  Nothing in the product selects it -- the
 * range kernel takes every table, combine's query tables with their one-way partner lists included (its junction table is
 * built from each row's own lists); both give identical counters. */
#define SPL_OPT_PAIR_KERNEL 1
/* Selects nothing; defined so that ABI v1 callers that set it still build and run.  A pass with this bit set is the default
 * pass and gives the same counters, and a read set that stays fused stays fused. */
#define SPL_OPT_WAVE_AGGREGATION 2

/* ---- library / context ------------------------------------------------------------------------ */
int spl_abi_version(void);
const char *spl_last_error(void);
int spl_device_count(int *n_out);
/* The library keeps device memory it was given back (read sets, site tables, the buffers of a device decode) for its next call
 * in the same process -- fresh device memory costs 30 ms per GB on this stack -- up to half of what was free on the device when it
 * first asked (SPL_DEV_CACHE_GB overrides).  spl_trim returns all of it to the driver: device_id, or -1 for every device. */
int spl_trim(int device_id);
/* Test hooks on that pool.  spl_devmem_stats: since the process began, out[0] buffers handed out, out[1] those of them that were
 * served from the pool, out[2] those that were poisoned (SPL_DEV_POISON=1 fills every buffer with 0xA5 as it is handed out),
 * out[3] the bytes the pool holds now.  spl_devmem_probe takes a buffer of `bytes` from the pool under `tag` the way the library
 * takes its own, copies its whole capacity (at most `room` bytes) to host_out as it was handed over, reports the capacity in
 * *cap_out and gives the buffer back. */
int spl_devmem_stats(int64_t out[4]);
int spl_devmem_probe(spl_ctx *ctx, int64_t bytes, int tag, uint8_t *host_out, int64_t room, int64_t *cap_out);
int spl_create(int device_id, spl_ctx **out);
/* Same, but work is enqueued on a caller-provided hipStream_t (e.g. torch's current stream). */
int spl_create_on_stream(int device_id, void *hip_stream, spl_ctx **out);
void spl_destroy(spl_ctx *ctx);
int spl_sync(spl_ctx *ctx);
/* Device-side barrier: what is launched on the context after this call starts after everything launched before it has
 * finished (the tails of counting passes, which run on a second stream, included).  The host does not wait. */
int spl_pass_barrier(spl_ctx *ctx);
/* HIP-event stopwatch on the context's stream (what bench.py times the kernels with). */
int spl_timer_begin(spl_ctx *ctx);
int spl_timer_end(spl_ctx *ctx, float *elapsed_ms_out);

/* Per-launch stopwatch around the classification kernel ALONE (HIP events recorded on the context's
 * stream immediately before and after each spl_count_kernel launch).  begin() arms up to max_records
 * launches; collect() synchronises and returns their durations in launch order. */
int spl_kernel_timing_begin(spl_ctx *ctx, int max_records);
int spl_kernel_timing_collect(spl_ctx *ctx, float *ms_out, int capacity, int *n_out);
/* The library's own stopwatch over ALL its kernels (process-wide): spl_prof_enable(1) clears what was recorded and brackets every
 * kernel launch from then on -- the device decode's, the device packer's, the counting passes' -- with two events on its stream;
 * spl_prof_report waits for the devices and writes JSON text, [{"kernel", "calls", "ms", "bytes"}, ...] most time first, `bytes`
 * being what the kernel was given to work on (the stretch of the inflated stream, the reads: algorithmic, not fetched).  Returns
 * the length the text needs.  What bench.py's end-to-end legs quote as their `kernels` table. */
int spl_prof_enable(int on);
int spl_prof_report(char *buf, int cap);

/* ---- one-shot entry points on host buffers (what the `process` driver calls per shard) ---------
 * spl_count  == the checkBam loop of processSites (SpliSER_v0_1_8.py:686-688) for all sites at once.
 *   beta1[s]         += reads classified "beta1" for site s           (SpliSER_v0_1_8.py:558-559)
 *   beta2s_reads[s]  += reads that add to beta2SimpleCounts in checkBam (:532, :541, :552)
 *   dbl[e]           += PartnerBeta2DoubleCounts increments for partner edge e (:527, :551)
 * Outputs are overwritten (not accumulated). */
int spl_count(spl_ctx *ctx, const spl_sites *sites, const spl_reads *reads, const spl_opts *opts,
              uint32_t *beta1, uint32_t *beta2s_reads, uint32_t *dbl);

/* spl_sse == findBeta2Counts + calculateSSE for every site (SpliSER_v0_1_8.py:690-692, 581-639).
 * Needs sites->alpha, sites->edge_cnt and sites->part_site.  All arithmetic is IEEE binary64 with
 * no contraction, in the reference's operation order, so results are bit-identical to CPython's. */
int spl_sse(spl_ctx *ctx, const spl_sites *sites, const uint32_t *beta1, const uint32_t *beta2s_reads,
            const uint32_t *dbl, int beta2_cryptic, int64_t *beta2_simple, int64_t *beta2_cryptic_count,
            double *beta2_weighted, double *sse);

/* ---- device-resident pipeline (bench.py, multi-shard overlap) ---------------------------------- */
int spl_sites_upload(spl_ctx *ctx, const spl_sites *sites, spl_dsites **out);
void spl_sites_free(spl_ctx *ctx, spl_dsites *ds);
/* A read set on the device.  The counting kernels do not read the BAM-native arrays: a read set is cut into chunks of 2048
 * (or 4096) reads, each chunk partitioned by the kind of read (unspliced / once-spliced / twice-spliced / anything else) with
 * records as wide as the kind needs (8 / 16 / 24 bytes; spliser_amd/csrc/spl_pack.h).  A caller's HOST arrays are packed that
 * way by host threads on their way up, piece by piece through a ring of page-locked staging buffers, the DMA of one piece
 * running while the next is packed (the records are two thirds of the arrays' bytes, and a hand-over is bound by PCIe); reads
 * that are in device memory already (spl_bam_decode_device, spl_soa_upload) are laid out by the layout kernel
 * (spliser_amd/csrc/spl_devpack.hip).  The caller's arrays are not needed after the call returns. */
int spl_reads_upload(spl_ctx *ctx, const spl_reads *reads, spl_dreads **out);
/* Same, from n_seg host segments laid end to end: segment k is moved by pos_shift[k] into the shard's coordinate space
 * (spliser_amd/shard.py packs several chromosomes into one launch that way).  Reads keep segment order. */
int spl_reads_upload_segments(spl_ctx *ctx, int n_seg, const spl_reads *segs, const int32_t *pos_shift, spl_dreads **out);
/* The same in steps, for segments that become available one after the other (the references of a BAM file while it is still
 * being decoded): begin, add ... add, finish; counting passes need a finished read set.  spl_reads_add_bam takes the reads of
 * reference `tid` straight from the decoder's buffers -- host memory, or the device's own after spl_bam_decode_device -- and
 * waits until that reference is complete (spl_bam_wait_ref). */
int spl_reads_begin(spl_ctx *ctx, spl_dreads **out);
/* ... with the number of reads that are going to be added, if the caller knows it (0 = no idea): sets of 64 M reads and more are
 * cut into chunks of 4096 instead of 2048 reads, which suits launches of that size (3.5 % on 100 M reads) and no others. */
int spl_reads_begin_sized(spl_ctx *ctx, int64_t expected_reads, spl_dreads **out);
int spl_reads_add(spl_ctx *ctx, spl_dreads *dr, const spl_reads *reads, int32_t pos_shift);
/* ... known_max_end: the last base (1-based) any of the reads covers, if the caller knows it (< 0: computed when needed) */
int spl_reads_add2(spl_ctx *ctx, spl_dreads *dr, const spl_reads *reads, int32_t pos_shift, int64_t known_max_end);
int spl_reads_add_bam(spl_ctx *ctx, spl_dreads *dr, spl_bam *bam, int tid, int32_t pos_shift);
int spl_reads_finish(spl_ctx *ctx, spl_dreads *dr);
void spl_reads_free(spl_ctx *ctx, spl_dreads *dr);
/* BAM-native reads RESIDENT IN HBM, as the arrays they are (what checkBam reads from a SAM line, SpliSER_v0_1_8.py:434-437, and
 * nothing else): n_seg host segments laid end to end in device arrays pos / flag / cig_off / cigar -- what a decode on the
 * device leaves (spl_bam_decode_device) and what SURVEY.md 8(d)'s "kernel-only from device-resident SoA" starts from.  A read
 * set is made from them ON THE DEVICE by spl_reads_add_soa + spl_reads_finish.  A set whose segments all lie in ONE such handle
 * stays arrays ("fused"): spl_count_launch reads them itself and makes its records in LDS (spl_kernels.hip, the FUSED range
 * kernel) -- no records in memory, no layout launch, and spl_junctions reads the arrays too; what needs records (the pair kernel), a set of several
 * handles or with host-packed segments, or SPL_FUSED=0, gets them from the layout kernel
 * (spl_devpack.hip: one launch, every read fetched and classified once).  spl_reads_relayout does again what spl_reads_finish
 * launched -- the chunks' descriptors and order, and the layout kernel where the set has records -- so that a bench.py step is
 * arrays -> counters, every step.  The handle may be freed while read sets made from it live (they share the arrays). */
typedef struct spl_dsoa spl_dsoa;
int spl_soa_upload(spl_ctx *ctx, int n_seg, const spl_reads *segs, spl_dsoa **out);
/* ... with max_end[k] = the last base (1-based) any read of segment k covers, where the caller knows it (null, or < 0: computed) */
int spl_soa_upload2(spl_ctx *ctx, int n_seg, const spl_reads *segs, const int64_t *max_end, spl_dsoa **out);
/* ... and with xs[k] = a strand byte per read of segment k ('+', '-', 0 = none): a fifth device array beside flag, which
 * spl_junctions reads with stranded = 3.  How reads the host decoded (spl_bam_aux_strand) and SAM text get there. */
int spl_soa_upload3(spl_ctx *ctx, int n_seg, const spl_reads *segs, const int64_t *max_end, const uint8_t *const *xs, spl_dsoa **out);
/* ... and with name_key[k] = a name key per read of segment k (0 = no name; the key: "mates and fragments" below): a further
 * device array beside flag, which spl_mate_table and spl_gene_count_fragments read.  xs may be null: no strand bytes. */
int spl_soa_upload4(spl_ctx *ctx, int n_seg, const spl_reads *segs, const int64_t *max_end, const uint8_t *const *xs, const uint64_t *const *name_key,
                    spl_dsoa **out);
void spl_soa_free(spl_ctx *ctx, spl_dsoa *soa);
int spl_reads_add_soa(spl_ctx *ctx, spl_dreads *dr, spl_dsoa *soa, int seg, int32_t pos_shift);
int spl_reads_relayout(spl_ctx *ctx, spl_dreads *dr);
/* *out = 1 when the set is fused and its arrays have the fifth one, the reads' strand bytes (a decode after
 * spl_bam_set_aux_strand, spl_soa_upload3): what spl_junctions' stranded = 3 needs.  0 otherwise. */
int spl_reads_has_strand(const spl_dreads *dr, int *out);
/* *out = 1 when the set is fused and its arrays have the reads' name keys (a decode after spl_bam_set_mate_keys, spl_soa_upload4):
 * what spl_mate_table needs.  0 otherwise. */
int spl_reads_has_mate_keys(const spl_dreads *dr, int *out);
/* What the layout moves for a finished read set: the BAM-native arrays read (10 bytes a read + 4 an op) and the records written
 * (0 while the set is fused). */
int spl_reads_layout_bytes(spl_ctx *ctx, const spl_dreads *dr, int64_t *soa_bytes_out, int64_t *record_bytes_out);
/* The range kernel's slots of a finished read set as the last spl_reads_finish / spl_reads_relayout left them, read back (test
 * hook; no product path calls it; waits for the layout).  *n_slots_out = 8 shares of equal length, *n_chunks_out chunks among
 * them; any output may be NULL.  order_out: uint32[n_slots], the chunk of every slot (0xffffffff: none).  A fused set also has
 * slots_out: n_slots descriptors of 64 bytes, and chunks_out: n_chunks descriptors of 32 bytes (spl_fused_slot, spl_layout_chunk
 * of spl_devpack.h); asked of any other set they are an error. */
int spl_reads_slots_download(spl_ctx *ctx, const spl_dreads *dr, int64_t *n_chunks_out, int64_t *n_slots_out, int *fused_out,
                             uint32_t *order_out, void *slots_out, void *chunks_out);
/* ... and the durations of the layout kernel's launches since spl_kernel_timing_begin (call before spl_kernel_timing_collect) */
int spl_layout_timing_collect(spl_ctx *ctx, float *ms_out, int capacity, int *n_out);
/* The host packer alone (no GPU involved; diagnostic and test hook): sizes of what an upload of `reads` would send, and --
 * into buffers of those sizes, when given -- the bytes: chunk descriptors (32 bytes each: record offset u64, wide-op offset
 * u64, first POS i32, cost u32, reads per run u16[4]), the record blob, the wide ops. */
int spl_pack_host(const spl_reads *reads, int n_threads, int64_t *n_chunks_out, int64_t *rec_bytes_out, int64_t *n_wide_out,
                  void *chunk_desc, void *rec, uint32_t *wide);
/* Enqueue one counting pass of dr over ds (asynchronous): the range kernel on the context's stream, then the literal kernel
 * and the scan (which also computes beta2 / SSE when the table has the inputs) on a second stream the context owns, so that
 * the range kernel of the NEXT launch -- next shard, sample or step -- starts as soon as this one's is done.  The counters
 * start from zero (a clean copy of the counter region; the table keeps three).  spl_sync and the download calls wait for
 * everything; a download returns the results of the LAST pass launched on that table.  Environment, read when the context
 * is created: SPL_TAIL_STREAM=0 -- one stream. */
int spl_count_launch(spl_ctx *ctx, spl_dsites *ds, const spl_dreads *dr, const spl_opts *opts);
/* Enqueue the beta2/SSE kernel on the counters currently held by ds (asynchronous). */
int spl_sse_launch(spl_ctx *ctx, spl_dsites *ds, int beta2_cryptic);
/* Synchronise and copy results back; any output pointer may be NULL. */
int spl_counters_download(spl_ctx *ctx, const spl_dsites *ds, uint32_t *beta1, uint32_t *beta2s_reads,
                          uint32_t *dbl);
int spl_sse_download(spl_ctx *ctx, const spl_dsites *ds, int64_t *beta2_simple,
                     int64_t *beta2_cryptic_count, double *beta2_weighted, double *sse);
/* Bytes the classification kernel must move at minimum for (ds, dr): each input once, each output
 * once -- the numerator of bench.py's roofline.achieved. */
int spl_count_algorithmic_bytes(const spl_dsites *ds, const spl_dreads *dr, int64_t *bytes_out);
/* Reads the last range-kernel launch on dr handed to the literal kernel (unmapped-but-placed records and reads
 * whose junction ends have rival sites); synchronises.  Diagnostic. */
int spl_literal_queue_size(spl_ctx *ctx, const spl_dreads *dr, int64_t *n_out);
/* Launch geometry of the last spl_count_launch on this context (for DESIGN.md / profiles). */
int spl_last_launch_info(const spl_ctx *ctx, int32_t *grid_out, int32_t *block_out, int32_t *lds_bytes_out);

/* ---- BAM ingest: replaces `samtools view` (SpliSER_v0_1_8.py:422) ------------------------------
 * The whole BGZF file is inflated and its alignment records are split per reference sequence on n_threads host threads
 * (0 = all cores up to 32).  Like `samtools view` without -F/-q every record that has a reference id is kept (secondary,
 * supplementary, duplicate, QC-fail, unmapped-but-placed ...) -- unless a read filter is set (spl_bam_set_filter below): then
 * only the records that pass it are, as if the file had gone through `samtools view -q / -f / -F` first.
 * spl_bam_open_stream returns once the block directory and the header are read; the decode goes on on threads of its own.
 * spl_bam_wait_ref waits until reference `tid` is complete -- in a file sorted by reference that is when a record of a later
 * reference has been seen, long before the end of the file -- so that its reads can go to the GPU (spl_reads_add_bam) while
 * the rest is still being inflated.  spl_bam_wait_all waits for the end of the file and says whether the file WAS sorted by
 * reference (*sorted_out = 0: records of an earlier reference came after a later one; a consumer that took references early
 * must then take them again).  spl_bam_open = open_stream + wait_all. */
int spl_bam_open(const char *path, int n_threads, spl_bam **out);
int spl_bam_open_stream(const char *path, int n_threads, spl_bam **out);
/* Decode on the DEVICE instead: spl_bam_open_deferred reads the header and starts nothing; spl_bam_decode_device then sends the
 * file to the GPU as it is, inflates its BGZF blocks there (Huffman decoding a wave per block, the copies it leaves a lane per
 * block, CRC32 checked; a window of the stream at a time, the next window's decoding beside this window's checks and the upload
 * beside both), finds and extracts the alignment records there, and keeps what checkBam reads (POS, FLAG, CIGAR: a fifteenth of
 * the inflated bytes) in device memory: spl_reads_add_bam on a context of the same device lays a reference's reads out for the
 * counting kernels with kernels, nothing crosses PCIe again; spl_bam_reads (or a context on another device) makes the host
 * copies, once.  Every reference is complete when the call returns.  *on_device_out = 0: the file is one the device path does not take (not sorted by
 * reference, CIGARs parked in CG tags, anything malformed) and the host threads have been started on it instead -- results and
 * error reporting are the host decoder's either way.  Waiting on a deferred file nobody decoded starts the host decode. */
int spl_bam_open_deferred(const char *path, int n_threads, spl_bam **out);
/* Read filter, samtools view's -q / -f / -F (the reference has none: its pipelines run samtools over the file first): of the
 * records that have a reference and a position only those are kept with (flag & exclude_flags) == 0, (flag & require_flags) ==
 * require_flags and MAPQ >= min_mapq -- MAPQ as a number, 255 passes every threshold.  A record that fails is never extracted,
 * counted or handed out, on the host's decoder and the device's alike; spl_bam_n_records still counts it.  0, 0, 0 (the default)
 * keeps everything.  To be called before anybody decodes the file or waits for it, i.e. on a file from spl_bam_open_deferred
 * (spl_bam_open_stream and spl_bam_open start the decode themselves); later, or with min_mapq outside 0..255 or a mask outside
 * 0..65535, it is SPL_ERR_ARG.  spl_bam_filter_counts: out2 = {records dropped by their flags, records dropped by their MAPQ
 * alone} -- flags are tested first -- once the decode is complete (it waits for that, like spl_bam_n_records). */
int spl_bam_set_filter(spl_bam *bam, int min_mapq, int require_flags, int exclude_flags);
int spl_bam_filter_counts(spl_bam *bam, int64_t *out2);
/* The transcript strand an aligner wrote on its spliced reads for an unstranded library (XS:A:+/-: STAR --outSAMstrandField
 * intronMotif, HISAT2, TopHat; what `regtools junctions extract -s XS` reads; the reference has no counterpart, its README sends
 * the user to regtools).  spl_bam_set_aux_strand(bam, 1): the decode -- the device's and the host's alike -- leaves one more byte
 * per placed read, in file order beside its FLAG: for a read whose own CIGAR holds an N op the value of the FIRST aux field XS of
 * type A if that is '+' or '-', else 0 (no such field, another value, an area that cannot be walked to it; an XS of another type
 * -- BWA's XS:i -- is stepped over like any field); for every other read 0, its aux area untouched.  The same rule as
 * spl_bam_set_filter: before anybody decodes the file or waits for it, SPL_ERR_ARG afterwards.  A dropped read has no byte.
 * spl_bam_aux_strand: borrowed view (until spl_bam_close) of the bytes of the reads spl_bam_reads hands out for `tid`, same order;
 * *out = NULL when the file was decoded without them.  struct spl_reads is unchanged.  spl_bam_aux_strand_host: the walk itself
 * over a caller's bytes [aux, aux + len) -> *out (test hook; no file, no GPU). */
int spl_bam_set_aux_strand(spl_bam *bam, int on);
/* Which two records are mates (what fragment counting needs: "mates and fragments" below).  spl_bam_set_mate_keys(bam, 1): the
 * decode -- the device's and the host's, of BAM and of SAM text alike -- leaves one more array per placed read, in file order
 * beside its FLAG and carried through the sort of spl_bam_set_any_order: the 64-bit key of its name (BAM: the l_read_name - 1
 * bytes 36 bytes into the record, walked no further than the record's end; SAM: column 1), 0 for an empty name and for `*`.  The
 * same rule as spl_bam_set_filter: before anybody decodes the file or waits for it, SPL_ERR_ARG afterwards.  Without the switch
 * the decode is what it was: the kernels that hash names are instantiations of their own.  spl_bam_mate_keys: borrowed view (until
 * spl_bam_close) of the keys of the reads spl_bam_reads hands out for `tid`, same order; *out = NULL when the file was decoded
 * without them.  spl_reads_add_bam picks the keys up where they are on the device; host arrays bring theirs with spl_soa_upload4. */
int spl_bam_set_mate_keys(spl_bam *bam, int on);
int spl_bam_mate_keys(const spl_bam *bam, int tid, const uint64_t **out);
/* Library size without a second pass over the file (the reference's README sends the user to `samtools flagstat` for the
 * Library_size column of the diffSpliSER target file; the reference has no counterpart).  spl_bam_set_flagstat(bam, 1): the
 * decode -- the device's and the host's alike, whole or in shares -- also counts samtools flagstat's sixteen categories, each for
 * QC-passed and QC-failed records (FLAG 0x200), over EVERY record of the file: placed or not, with a reference or without.  Under
 * a read filter a record counts only if it passes the filter, which for this purpose is applied to every record (as `samtools
 * view -q 10` drops an unmapped record of MAPQ 0); spl_bam_filter_counts keeps its meaning and its values.  The same rule as
 * spl_bam_set_filter: before anybody decodes the file or waits for it, SPL_ERR_ARG afterwards.  Off by default, and nothing of
 * the decode changes while it is off.
 * spl_bam_flagstat: out32[2 * c + q] = records of category c that passed (q = 0) / failed (q = 1) quality control, once the decode
 * is complete (it waits for that); SPL_ERR_ARG when counting was not switched on.  Categories, a record being PRIMARY when
 * neither 0x100 nor 0x800 is set: 0 total, 1 primary, 2 secondary (0x100), 3 supplementary (0x800 without 0x100), 4 duplicates
 * (0x400), 5 primary duplicates, 6 mapped (not 0x4), 7 primary mapped, 8 paired in sequencing (primary and 0x1), 9 read1 (8 and
 * 0x40), 10 read2 (8 and 0x80), 11 properly paired (8, 0x2, not 0x4), 12 with itself and mate mapped (8, not 0x4, not 0x8),
 * 13 singletons (8, 0x8, not 0x4), 14 with mate mapped to a different chr (12 and next_refID != refID), 15 ... and MAPQ >= 5.
 * spl_flagstat_add_host: the definition itself on one record's fields, added to inout32 (test hook; no file, no GPU). */
int spl_bam_set_flagstat(spl_bam *bam, int on);
int spl_bam_flagstat(spl_bam *bam, int64_t *out32);
int spl_flagstat_add_host(uint32_t flag, int32_t tid, int32_t next_tid, uint32_t mapq, int64_t *inout32);
/* No `samtools sort` in front of the decode (the reference reads through `samtools view BAM region`, SpliSER_v0_1_8.py:422, which
 * needs the index of a coordinate-sorted file; STAR's and HISAT2's own output is not sorted).  spl_bam_set_any_order(bam, 1): the
 * file's records may come in ANY order, and after the decode -- the device's and the host's alike -- every reference's reads are
 * handed out sorted by (POS, place in the file), to every consumer: spl_bam_reads, spl_reads_add_bam, spl_bam_aux_strand, the
 * junction tables.  spl_bam_wait_all then reports *sorted_out = 1 whatever the file's order was, spl_bam_wait_ref returns at the
 * end of the decode only (a reference of such a file is complete no earlier), and the device decoder does not hand the file to the
 * host for its order.  A file whose reference ids never go down is left exactly as it is without the switch, bytes and order (one
 * sorted by reference but not by POS inside a reference too).  On the device the placed records' arrays are sorted by a stable
 * radix sort of (reference id << 32 | POS) between the last extraction and the bounds kernel (csrc/spl_sort.hip); the host decoder
 * orders each reference's reads with a stable index sort; both leave the same arrays.  The order of reads with equal
 * coordinates is the file's, not `samtools sort`'s tie order: no result depends on it.  The same rule as spl_bam_set_filter:
 * before anybody decodes the file or waits for it, SPL_ERR_ARG afterwards.  Off by default, and nothing of the decode changes
 * while it is off.  A decode in shares (spl_bam_share_plan) cuts the file on the order of references: not for such a file.
 * spl_bam_any_order_sorted: once the decode is complete (it waits for that), *n_sorted_out = the reads that were put in order
 * (0: the file was in order already) and *on_device_out = 1 when the device's sort did it, 0 when the host threads did.
 * spl_sort_keys_device: the device's sort itself on a caller's keys (test hook; no file): uploads n keys (n < 2^32 - 16), runs
 * exactly the passes the decode runs for keys of key_bits bits (1..64: the digits of the low word from bit 0, those of the high
 * word from bit 32, 8 bits a pass) and downloads the permutation -- perm_out[i] = index of the key that comes i-th, equal keys in
 * the order they came in.
 * spl_text_windows_host (test hook, no GPU): how the device's text sources cut a mapped text into windows of whole lines
 * (csrc/spl_text_windows.h) -- bytes [begin, len) of `text` into windows of at most win_bytes that end behind a newline, the last
 * one with the text; rule 0 (SAM text): a line that fits no window ends the plan in front of it, *long_line_out = 1; rule 1
 * (FASTA): it gets a window of its own.  *n_out = the windows, always written; cuts[2k], cuts[2k + 1] = window k's first byte and
 * the byte behind its last where cap >= *n_out, SPL_ERR_ARG otherwise.
 * spl_text_line_index (test hook): the line starts the device's text sources find (csrc/spl_sam.h) in windows [lo[w], hi[w]) of a
 * host text, 0 <= lo < hi <= len, ONE index object over all of them in the order given, its buffers kept, reused and regrown as a
 * decode's are.  n_lines_out[w] = window w's lines, room_out[w] = the lines the index had room for behind it; starts_out = every
 * window's line starts end to end, as offsets from lo[w] & ~15 (cap_starts of them at most, SPL_ERR_ARG otherwise). */
int spl_bam_set_any_order(spl_bam *bam, int on);
int spl_bam_any_order_sorted(spl_bam *bam, int64_t *n_sorted_out, int *on_device_out);
int spl_sort_keys_device(spl_ctx *ctx, const uint64_t *keys, int64_t n, int key_bits, uint32_t *perm_out);
int spl_text_windows_host(const uint8_t *text, int64_t len, int64_t begin, int64_t win_bytes, int rule, int64_t cap, int64_t *cuts, int64_t *n_out, int *long_line_out);
int spl_text_line_index(spl_ctx *ctx, const uint8_t *text, int64_t len, int64_t n_windows, const int64_t *lo, const int64_t *hi, int64_t cap_starts, int64_t *n_lines_out,
                        int64_t *room_out, uint32_t *starts_out);
int spl_bam_aux_strand(const spl_bam *bam, int tid, const uint8_t **out);
int spl_bam_aux_strand_host(const uint8_t *aux, uint32_t len, uint8_t *out);
int spl_bam_decode_device(spl_ctx *ctx, spl_bam *bam, int *on_device_out);
/* For a caller that will call spl_bam_decode_device from another thread in a moment while others may already wait for
 * references: the file is marked as taken by the device decoder now, so that those waits wait instead of starting the host
 * decode.  The promise must be kept (spl_bam_decode_device) or taken back (spl_bam_start), or the waits never end. */
int spl_bam_reserve_device(spl_bam *bam);
/* The same decode in SHARES, one per device (replaces SpliSER_v0_1_8.py:422 for a stretch of the file): a
 * BAM file's BGZF blocks are independent, so every device can take its own stretch -- over its own PCIe link, into its own memory,
 * no exchange.  spl_bam_share_plan cuts the file into up to n_shares stretches of EQUAL size in file bytes, at any BGZF block: a
 * share owns the records that begin in its blocks (the plan finds the record boundary at every cut by inflating a few blocks on
 * the host; a share's decoder must arrive exactly at the next share's first record, or the plan is dropped), so a reference may
 * lie in several shares.  That is what the per-site loop allows (processSites, :681-692: nothing in it needs a whole chromosome)
 * and what checkBam's counters allow (:519-559 only ever add one per read): each device counts its stretch of a reference
 * against the reference's whole site table, the host adds the partial beta1 / beta2s_reads / dbl arrays, and one spl_sse call
 * runs on the sums -- still no collective.  *n_out = the shares made (fewer than asked for only when the file has fewer blocks).
 * spl_bam_share_range: the references share k CAN hold records of (tid_lo <= tid < tid_hi; a superset by at most one at the upper
 * end; the last share also holds the records without a reference); spl_bam_share_info: the bytes of the file its own blocks take
 * (what the balance of the plan is judged by), the stretch [u_lo, u_hi) of the inflated stream its records begin in, and the
 * blocks it inflates behind its own for the end of its last record.  The file is then reserved (spl_bam_reserve_device) and
 * EVERY share decoded by a spl_bam_decode_device_share call, each on the context of the device that is to count it; the file is
 * complete when the last of them returns.  Should any share not be decodable on its device, all of them are dropped and the host
 * threads decode the file (*on_device_out = 0 from that share's call; spl_bam_decoded_on_device says how it ended).  Afterwards
 * spl_bam_share_ref says what share k holds of a reference and spl_reads_add_bam_share adds exactly that to a read set on the
 * share's device.  spl_bam_share_count_host (diagnostic, no GPU): the records of share k per reference by the host's inflate and
 * a plain walk from u_lo that must arrive at u_hi -- per_tid[n_ref + 1], the last entry the records without a reference; records
 * the file's read filter drops are left out. */
int spl_bam_share_plan(spl_bam *bam, int n_shares, int *n_out);
int spl_bam_share_range(spl_bam *bam, int k, int *tid_lo_out, int *tid_hi_out);
int spl_bam_share_info(spl_bam *bam, int k, int64_t *file_bytes_out, int64_t *u_lo_out, int64_t *u_hi_out, int64_t *tail_blocks_out);
int spl_bam_share_count_host(spl_bam *bam, int k, int64_t *per_tid);
int spl_bam_decode_device_share(spl_ctx *ctx, spl_bam *bam, int k, int *on_device_out);
int spl_bam_share_ref(spl_bam *bam, int k, int tid, int64_t *n_reads_out, int64_t *max_end_out);
int spl_reads_add_bam_share(spl_ctx *ctx, spl_dreads *dr, spl_bam *bam, int share, int tid, int32_t pos_shift);
int spl_bam_decoded_on_device(spl_bam *bam, int *on_device_out);
/* For whoever runs spl_bam_decode_device / _share on threads of his own and waits for the outcome elsewhere: returns when the
 * file is no longer the device decoders' to decide about -- *on_device_out = 1: its reads are on the device(s), every reference
 * complete; 0: the host threads have it (and may still be decoding: spl_bam_wait_ref / _all).  It does not wait for the decoders'
 * calls to RETURN: a call gives its buffers, streams and events back after it has made the references complete (10 ms for a
 * large file), and the counting need not stand behind that (`process` Step 3, SpliSER_v0_1_8.py:681-692 per chromosome). */
int spl_bam_wait_device(spl_bam *bam, int *on_device_out);
/* A deferred file's other option, said out loud: decode on the host's threads, starting now.  Also ends a reservation that
 * nobody has taken up (its maker failed before it could call spl_bam_decode_device). */
int spl_bam_start(spl_bam *bam);
/* Inflated bytes per file byte over the first record blocks of a deferred file (0 = cannot tell).  Diagnostic: BGZF inflate is
 * what a decode costs; since the wave-per-block decoder the GPU is the faster side for a real library's file (3...4) and for one
 * that inflates at memset speed (synthetic data: 50) alike, and `process` no longer asks. */
int spl_bam_compression_ratio(spl_bam *bam, double *ratio_out);
/* Records, their CIGAR ops, and the inflated bytes both were counted in, sampled on the host at three places of the file (the
 * whole block directory is walked first): out3 = {records, ops, bytes}.  What the device decoder sizes its extracted arrays by
 * before anything runs on the device (spl_capi.cpp: early_room); here for tests and diagnostics.  SPL_ERR_FORMAT: cannot tell. */
int spl_bam_sample(spl_bam *bam, int64_t *out3);
int spl_bam_wait_ref(spl_bam *bam, int tid, int64_t *n_reads_out, int64_t *max_end_out);
int spl_bam_wait_all(spl_bam *bam, int *sorted_out);
/* spl_bam_close waits for a decode in progress to END.  A caller who only wants to leave (something else failed) says so first:
 * after spl_bam_cancel the decoders stop at their next batch (host) or window (device), a decode that has not begun never
 * does, and waiting calls return with an error. */
void spl_bam_cancel(spl_bam *bam);
/* Why the device decoder (spl_bam_decode_device / _share) left this file to the host threads: "" if it did not, otherwise a few
 * words (not sorted by reference, a CIGAR parked in a CG tag, a block that did not inflate, not enough device memory, ...).  The
 * pointer is good while the file is open.  (The reference has no counterpart: samtools reads whatever it is given, :422.) */
const char *spl_bam_decline_reason(spl_bam *bam);
/* SAM TEXT behind the same object, as the aligner writes it (HISAT2 always, STAR by default): no `samtools view -b` in front.
 * spl_sam_open maps the file, reads the header on the host (@SQ SN / LN, in order: the reference ids) and starts nothing: a
 * deferred file, to which the four spl_bam_set_* setters, spl_bam_decode_device and every consumer apply unchanged (wait_ref /
 * wait_all, spl_reads_add_bam, spl_bam_reads, spl_bam_aux_strand, spl_bam_flagstat, spl_bam_filter_counts, spl_bam_n_records,
 * spl_bam_any_order_sorted).  spl_bam_decode_device parses the text on the GPU: line starts by a wave per 16 KiB, then a lane per
 * line, windows of SPL_SAM_WINDOW_BYTES (default 256 MiB) going up while the one before is parsed; without that call, or where
 * the device cannot (memory, a HIP error), one host thread parses it.  Either way by ONE strict rule (csrc/spl_sam_line.h), and
 * always as spl_bam_set_any_order: lines in any order, sorted on the GPU when reference ids or POS ever go down.  A file with a
 * line the rule does not take is declined as a whole: the decode ends with SPL_ERR_FORMAT, spl_bam_decline_reason says
 * "line N <why>" (1-based, header lines counted), and the caller reads the file by other means (process.py: samio.read_sam, as
 * before).  A line longer than SPL_SAM_WINDOW_BYTES, its newline counted, is such a line for both decoders.  SPL_ERR_FORMAT from
 * spl_sam_open itself: gzip/BGZF data that is no SAM text (a BAM, anything else), no @SQ line, an @SQ line without SN and LN, a
 * repeated name, a line that begins "@SQ" and is no @SQ line, a carriage return in the header.  n_threads is kept and unused: the
 * host parser is one thread.  spl_bam_share_plan, spl_bam_sample and spl_bam_compression_ratio are SPL_ERR_ARG on such a file;
 * spl_bam_open* keep refusing text, compressed or not.  spl_bam_is_text: 1 for such a file.
 * COMPRESSED TEXT, the form such files have on disk: a file that begins 1f 8b is taken when its inflated content is SAM text.  The
 * host inflates as far as the header's end; line numbers and every offset are those of the inflated text.  BGZF (bgzip, samtools
 * view -O sam: the block walk takes the whole file, EOF marker included -- without one SPL_ERR_IO, as for a BAM):
 * spl_bam_decode_device sends the file's blocks up and inflates them there, a block per wave, in windows of whole blocks, and
 * parses the text where it lies; the bytes behind a window's last newline are carried to the front of the next window on the
 * device.  Plain gzip (anything else zlib takes, several members too): one host thread inflates and the text goes up to the same
 * parser.  Every line of at most SPL_SAM_WINDOW_BYTES is taken wherever blocks and windows cut it; line numbers in a decline are
 * the plain text's.  Without a device decode, or where it gives up (a block that does not inflate, a wrong CRC32, memory), one host
 * thread inflates in pieces and parses, holding a line and a piece of the text at a time; damaged data ends the decode with
 * SPL_ERR_FORMAT.  spl_bam_text_compression: 0 plain text (or no text), 1 BGZF, 2 gzip.  spl_bam_text_blocks: the BGZF blocks a
 * device decode of the file inflated.
 * Not read: CRAM, a pipe; no decode in shares.  (process.open_alignments sends a compressed file to spl_sam_open only when it
 * inflates to an '@': compressed text without a header is not read by the commands.) */
int spl_sam_open(const char *path, int n_threads, spl_bam **out);
int spl_bam_is_text(const spl_bam *bam);
int spl_bam_text_compression(const spl_bam *bam);
int64_t spl_bam_text_blocks(const spl_bam *bam);
void spl_bam_close(spl_bam *bam);
int spl_bam_n_ref(const spl_bam *bam);
const char *spl_bam_ref_name(const spl_bam *bam, int tid);
int64_t spl_bam_ref_length(const spl_bam *bam, int tid);
int64_t spl_bam_n_records(const spl_bam *bam); /* all records, including those without a reference */
/* Borrowed view (valid until spl_bam_close) of the reads placed on reference `tid` as BAM-native arrays, assembled on the
 * first call (waits for the whole file); *max_end_out = largest 1-based end coordinate any of them reaches (for shard
 * packing).  The GPU path does not need these arrays (spl_reads_add_bam). */
int spl_bam_reads(const spl_bam *bam, int tid, spl_reads *out, int64_t *max_end_out);

/* Test / synthetic-workload utility (no reference counterpart): write per-reference read sets as a coordinate-ordered
 * BAM with dummy names, SEQ and QUAL of the query length, BGZF blocks deflated on n_threads (0 = all cores). */
int spl_bam_write(const char *path, int n_ref, const char *const *ref_names, const int64_t *ref_lengths,
                  const spl_reads *per_ref, int level, int n_threads);
/* Same with a choice of what SEQ / QUAL hold: seq_mode 0 = constant bytes (spl_bam_write: a file that deflates to a few bytes
 * per record), 1 = pseudo-random bases and binned qualities in runs (deflates about 4x, like a real library). */
int spl_bam_write2(const char *path, int n_ref, const char *const *ref_names, const int64_t *ref_lengths,
                   const spl_reads *per_ref, int level, int n_threads, int seq_mode);

/* ---- junction table of a read set (what the pipeline otherwise takes from `regtools junctions extract`) --------------
 * Every N op of every mapped read is a junction (left, right) in SpliSER's site convention (left = last base before the
 * intron, right = last intronic base, SpliSER_v0_1_8.py:482-483 -- the numbers findAlphaCounts derives from a BED12 line,
 * :275-276).  spl_junctions builds, on the device, the table of distinct (left, right[, read strand]) with the number of
 * reads carrying each and the longest anchors on either side (reference bases of the read between the junction and the
 * previous / next N op or read end: the block sizes of a BED12 line), and returns their number; spl_junctions_get copies
 * the table of the last call, sorted by (left, right, strand), into caller arrays (any may be NULL).  stranded: 0 ->
 * strand '?', 1 = fr / 2 = rf -> '+' / '-' of the read by check_strand's rule (:374-406); 3 -> the strand byte the decode left
 * for the read (spl_bam_set_aux_strand, spl_soa_upload3: the aligner's XS:A tag, regtools' -s XS): '+', '-', or '?' for 0, so
 * that a junction carried by reads of all three kinds is THREE rows, each with its own count and anchors, sorted like every table
 * ('+' < '-' < '?').  3 is for fused sets whose arrays have the bytes; on any other set it is SPL_ERR_ARG, never a table of '?'.
 * Policy knobs in the sense of
 * regtools' -a / -m / -M: a read supports a junction only if both of ITS anchors are >= min_anchor and the intron length
 * is in [min_intron, max_intron] (max_intron 0 = no upper limit); 0, 0, 0 counts every N op.  A fused set stays fused: its
 * table comes straight from the arrays (spl_reads_layout_bytes still reports 0 record bytes afterwards). */
int spl_junctions(spl_ctx *ctx, const spl_dreads *dr, int stranded, int32_t min_anchor, int32_t min_intron, int32_t max_intron,
                  int64_t *n_out);
int spl_junctions_get(const spl_ctx *ctx, int32_t *left, int32_t *right, uint8_t *strand, uint32_t *count,
                      uint32_t *anchor_left, uint32_t *anchor_right);
/* What the last spl_junctions call cost: the bytes of the device table it allocated and, for a fused set between
 * spl_kernel_timing_begin and spl_kernel_timing_collect, the device time of its launches in ms (-1 = not measured). */
int spl_junctions_stats(const spl_ctx *ctx, int64_t *table_bytes_out, float *ms_out);
/* The per-read walk the junction kernels share, on the host (no GPU involved; test hook): every N op of the read at `pos` with
 * the given ops (BAM form) -> left, right, both anchors and whether the read supports it under the knobs; *n_out = their
 * number (the first `capacity` are written), *range_error_out = the walk left the coordinate space. */
int spl_junction_walk_host(const uint32_t *ops, uint32_t n_ops, int32_t pos, int32_t min_anchor, int32_t min_intron, int32_t max_intron,
                           int capacity, int32_t *left, int32_t *right, uint32_t *anchor_left, uint32_t *anchor_right, uint8_t *passes,
                           int *n_out, int *range_error_out);
/* ---- the junction table per FRAGMENT (the splice counts of `intronretention --fragments`) ---------------------------------------
 * Both mates of a pair that cross the same intron are one molecule's evidence for one splicing event; IRFinder, whose measure
 * `intronretention` restates, works on fragments.  The rule (csrc/spl_junctionfragment_rule.h): walks, anchors, knobs, the strand
 * modes 0 / 1 / 2 / 3 and the table keys are spl_junctions', unchanged.  A junction that read r SUPPORTS, with table key K, is a
 * DUPLICATE CARRY when r has a mate m < r by its segment's mate table (m != SPL_MATE_NONE, m < n, m != r) and read m's own walk
 * supports a junction with the same key K, the strand taken by m's own flag (or strand byte) under the same mode.  A duplicate
 * carry adds nothing, no count and no anchors; everything else is inserted exactly as spl_junctions inserts it.  Hence: the key
 * set of the table equals the per-read table's; count_frag(K) = count_read(K) - duplicates(K); the anchors are <= the per-read
 * table's.  Reads that are not pairable behave as in the per-read table.  `junctions` and `process` have NO such switch: the BED
 * score feeds SpliSER's alpha, which stays per read beside beta1 / beta2.
 * spl_junctions_fragments: spl_junctions' arguments, result (spl_junctions_get / spl_junctions_stats) and refusals, and
 * spl_mate_table's: SPL_ERR_ARG for a set without name keys, not fused or not finished; the context stays usable.
 * spl_junction_fragment_rule_host: the rule for every read of one segment's host arrays with its mate table (test hook; no GPU).
 * xs: the reads' strand bytes (stranded = 3) or NULL.  counted_out[r] / duplicate_out[r]: the junctions read r supports that are
 * inserted / that are duplicate carries; rows_out (or NULL) [0 .. cap) x 6: left, right, strand byte, anchor_left, anchor_right,
 * duplicate, of every supported junction in read and walk order; *n_rows_out: all of them. */
int spl_junctions_fragments(spl_ctx *ctx, const spl_dreads *dr, int stranded, int32_t min_anchor, int32_t min_intron, int32_t max_intron,
                            int64_t *n_out);
int spl_junction_fragment_rule_host(int64_t n_reads, const int32_t *pos, const uint16_t *flag, const uint32_t *cig_off, const uint32_t *cigar,
                                    const uint8_t *xs, const uint32_t *mate, int32_t shift, int stranded, int32_t min_anchor, int32_t min_intron,
                                    int32_t max_intron, int64_t *counted_out, int64_t *duplicate_out, int64_t *rows_out, int64_t cap,
                                    int64_t *n_rows_out);

/* ---- strandedness of the library (what the pipeline otherwise asks the user for) -----------------------------------------
 * Replaces a manual step: the reference's README tells the user to open the BAM in IGV, colour the reads by first-in-pair and
 * compare them with a junction, to learn whether the library is unstranded, "fr" or "rf" -- "a common place to trip up": a wrong
 * answer does not fail, it gives no beta1 counts, or half the sites without a gene.  The reference has no counterpart.
 * spl_strand_tally counts, on the device, over the BAM-native arrays of a FUSED read set, how every read's strand compares with
 * two independent sources of its transcript's strand.  The rule (csrc/spl_strand_rule.h), per read the set holds:
 *   eligible    (flag & (0x4 | 0x100 | 0x200 | 0x800)) == 0;
 *   mate class  the branch check_strand takes (:374-406): 0 unpaired (!(flag & 1)), 1 first (flag & 1 and flag & 0x40), 2 second
 *               (every other paired read);
 *   fr strand   check_strand's '+' / '-' for "fr"; the "rf" strand is the opposite, so "agrees under rf" is "disagrees under fr";
 *   tag evidence         the read's strand byte when it is '+' or '-' (spl_bam_set_aux_strand: the aligner's XS:A tag on spliced
 *                        reads; spl_soa_upload3); a set without the fifth array has none;
 *   annotation evidence  from a strand cover map of the set's coordinate space: ascending int32 cover_start[n_cover] with uint8
 *                        cover_code[n_cover], code[k] holding for positions start[k] <= p < start[k + 1] (the last entry to
 *                        +infinity; 0 below start[0]); 0 = no gene, 1 = only '+' genes, 2 = only '-' genes, 3 = both.  With
 *                        ref_len = the sum of the lengths of the read's M, D, N, = and X ops and k = the last entry with start[k] <=
 *                        POS, the read has evidence when ref_len >= 1, POS + ref_len - 1 < start[k + 1] (or k is the last entry)
 *                        and code[k] is 1 ('+') or 2 ('-'): the whole span, introns included, lies in one stretch covered by
 *                        genes of one strand only.  Arithmetic in int64.
 * out14[0] = reads seen, [1] = eligible reads, [2 + 2 m + d] = eligible reads of mate class m with tag evidence, d = 0 when the fr
 * strand equals the evidence and 1 when it does not, [8 + 2 m + d] = the same for annotation evidence.  out14 is overwritten; the
 * call synchronises; integer sums, exact and the same for the reads in any order.  The CIGAR is read only when there is a map; a
 * map of any size is taken (its top level is searched in LDS, the rest where it is); a set without a single read gives fourteen zeros.  SPL_ERR_ARG: a set that is not fused; a set
 * without strand bytes and n_cover == 0 (nothing to tally); a map that is not strictly ascending.
 * spl_strand_rule_host: the same rule for one read on the host, added to inout14 (test hook; no file, no GPU). */
int spl_strand_tally(spl_ctx *ctx, const spl_dreads *dr, int64_t n_cover, const int32_t *cover_start, const uint8_t *cover_code, int64_t *out14);
int spl_strand_rule_host(uint32_t flag, int32_t pos, const uint32_t *ops, uint32_t n_ops, uint8_t xs, int64_t n_cover, const int32_t *cover_start,
                         const uint8_t *cover_code, int64_t *inout14);

/* ---- per-base coverage (what the pipeline otherwise needs a sorted, indexed BAM and a second tool for) ------------------------
 * Replaces a manual step: the reference's README sends the user to IGV whenever something looks wrong, and IGV wants a
 * coordinate-sorted, indexed BAM, or a coverage track from `bedtools genomecov -bg -split` / deepTools `bamCoverage`.  The
 * reference has no counterpart.  spl_coverage computes, on the device, over the BAM-native arrays of a FUSED read set taken as
 * the reads of ONE reference of `length` bases, the per-base read depth of one track as runs.  The rule (csrc/spl_coverage_rule.h):
 *   eligible    (flag & 0x4) == 0, POS >= 1 and at least one op: secondary, supplementary, duplicate and QC-failed reads count,
 *               as in bedtools genomecov (narrow them with the decode's read filter: spl_bam_set_filter);
 *   track       stranded = 0: one track, strand = 0.  stranded = 1 (fr) / 2 (rf): the read belongs to the track check_strand's
 *               rule gives it (:374-406), and strand = '+' or '-' says which track is computed;
 *   walk        from the 0-based p = POS - 1 + the segment's shift, in int64: M, = and X cover [p, p + len) and advance; D and N
 *               advance without covering (a deletion is a gap, as an intron is: genomecov's -split); I, S, H, P and the op codes
 *               above 8 do nothing, nor does an op of length zero; covering ops that abut (10M2I5M) are ONE block;
 *   clipping    blocks are clipped to [0, length); a read that loses a base that way is "past the end", a read left without a
 *               covered base does not contribute.
 * The result: runs (start, end, depth), 0-based and half-open, ascending, maximal (the depth differs from both neighbours'), only
 * depth > 0; the depth is an exact uint32 (sums mod 2^32: exact below 2^32 reads over a base), the same for the reads in any
 * order.  Parity with bedtools / deepTools is intended and not pinned by a test.  The call synchronises.  SPL_ERR_ARG: a set that
 * is not fused; length outside 1 .. 2^31 - 2; stranded outside 0..2; a strand that does not fit stranded.  A set without a single
 * read gives no run.
 * spl_coverage_totals: out5 = runs, reads seen (the whole set's, whatever the track), reads that contributed to this track, reads
 * past the end, covered bases (= the sum of (end - start) * depth over the runs).  spl_coverage_download: the runs into caller
 * arrays of `runs` entries (any may be NULL).  spl_coverage_free: NULL is allowed.
 * spl_coverage_rule_host: the same rule for one read on the host (test hook; no file, no GPU): its clipped blocks on the track,
 * *n_out of them (the first `capacity` are written), *past_end_out = it lost a base to the clipping.
 * spl_bedgraph_append: n runs of one chromosome appended to `path` as "chrom\tstart\tend\tvalue\n" lines; value = the depth as an
 * integer or, with per_million_of = N > 0, the text Python's repr(depth * 1000000 / N) gives.  No GPU involved. */
typedef struct spl_cov spl_cov;
int spl_coverage(spl_ctx *ctx, const spl_dreads *dr, int64_t length, int stranded, int strand /* 0, '+', '-' */, spl_cov **out);
int spl_coverage_totals(const spl_cov *cov, int64_t *out5);
int spl_coverage_download(spl_ctx *ctx, const spl_cov *cov, int32_t *start, int32_t *end, uint32_t *depth);
void spl_coverage_free(spl_ctx *ctx, spl_cov *cov);
int spl_coverage_rule_host(uint32_t flag, int32_t pos, const uint32_t *ops, uint32_t n_ops, int32_t shift, int64_t length, int stranded, int strand,
                           int capacity, int64_t *blk_start, int64_t *blk_end, int *n_out, int *past_end_out);
int spl_bedgraph_append(const char *path, const char *chrom, int64_t n, const int32_t *start, const int32_t *end, const uint32_t *depth,
                        int64_t per_million_of /* 0: integers */);

/* ---- per-base coverage per FRAGMENT (`coverage --fragments`) --------------------------------------------------------------------
 * Replaces deepTools `bamCoverage` (paired-end default) / `bedtools genomecov -pc -split`: where the mates of a pair overlap, one
 * molecule was sequenced, and a base under both counts once.  The rule (csrc/spl_covfragment_rule.h), per call -- one segment with
 * its mate table (spl_mate_table), `length`, `stranded`, `strand`:
 *   participates  a read for which spl_coverage's "eligible" and "track" hold, unchanged: secondary, supplementary, duplicate and
 *                 QC-failed reads still cover; only pairable reads can have a mate;
 *   partner       read r has the partner m = mate[r] when m != SPL_MATE_NONE, m < n, m != r and read m participates in this same
 *                 call.  A mate on the other track of a stranded run is no partner: each mate covers alone on its own track;
 *   silent        a participating read with a partner m < r marks nothing and is only "seen";
 *   union         every other participating read marks the UNION of its own clipped blocks and, if it has one, its partner's
 *                 (spl_coverage's walk and clipping): blocks that overlap OR abut are one interval.  It "contributed" when the
 *                 union has a base, is "past the end" when either read lost a base to the clipping, and its covered bases are
 *                 the union's length.
 * Which mate leads depends on the reads' order; the union does not: runs and totals are the same for the reads in any order.  The
 * deliberate differences are `genecounts --fragments`': a pair split over two references, segments or by the read filter is two
 * single fragments; names are compared by a 63-bit hash.  The gap between two mates is NOT filled (no --extendReads).  Parity with
 * deepTools / bedtools -pc is intended and unpinned.
 * spl_coverage_fragments: spl_coverage's arguments, result (read with spl_coverage_download / spl_coverage_free; spl_coverage_totals
 * keeps giving five numbers) and refusals, and spl_mate_table's: SPL_ERR_ARG for a set without name keys, not fused or not finished;
 * the context stays usable.  The mate table is made at the first call that needs it and kept with the set, per segment.
 * spl_coverage_fragment_totals: out6 = runs, reads seen, contributed (fragments, and reads without a partner), past the end,
 * covered bases (= the sum of (end - start) * depth over the runs), pairs whose union was taken.  After spl_coverage, [5] is 0.
 * spl_intron_depth_fragments: spl_intron_depth's arguments, output and refusals, and spl_mate_table's: the boundaries come from the
 * fragment mark kernel.
 * spl_coverage_fragment_rule_host: the rule for every read of one segment's host arrays with its mate table (test hook; no GPU):
 * status_out[r] = 1 contributed, 0 nothing to mark, -4 silent, -3 not participating; n_iv_out[r] = the intervals of read r's union
 * (all of them); past_out[r] (or NULL) = past the end; iv_start / iv_end [0 .. cap): the intervals, one read after the other in read
 * order; totals6 (or NULL): spl_coverage_fragment_totals' numbers, [0] being the intervals.
 * spl_coverage_cursor_host: spl_coverage_rule_host's arguments and results, by the rule header's resumable block cursor (test hook). */
int spl_coverage_fragments(spl_ctx *ctx, const spl_dreads *dr, int64_t length, int stranded, int strand /* 0, '+', '-' */, spl_cov **out);
int spl_coverage_fragment_totals(const spl_cov *cov, int64_t *out6);
int spl_intron_depth_fragments(spl_ctx *ctx, const spl_dreads *dr, int64_t length, int stranded, int strand /* 0, '+', '-' */, int64_t n_introns,
                               const int64_t *piece_off /* n_introns + 1 */, const int32_t *piece_start, const int32_t *piece_end,
                               int trim_percent, int64_t *out /* 4 per intron */);
int spl_coverage_fragment_rule_host(int64_t n_reads, const int32_t *pos, const uint16_t *flag, const uint32_t *cig_off, const uint32_t *cigar,
                                    const uint32_t *mate, int32_t shift, int64_t length, int stranded, int strand, int64_t *status_out,
                                    int64_t *n_iv_out, uint8_t *past_out, int64_t *iv_start, int64_t *iv_end, int64_t cap, int64_t *totals6);
int spl_coverage_cursor_host(uint32_t flag, int32_t pos, const uint32_t *ops, uint32_t n_ops, int32_t shift, int64_t length, int stranded, int strand,
                             int capacity, int64_t *blk_start, int64_t *blk_end, int *n_out, int *past_end_out);

/* ---- per-gene read counts (what the pipeline otherwise leaves to a second pass by another program) ---------------------------
 * Replaces `htseq-count` / `featureCounts` over the file this library has just decoded: the diffSpliSER analysis is an edgeR
 * analysis, and the gene's expression belongs beside a change in SSE.  The reference has no counterpart.  spl_gene_count counts,
 * on the device, over the BAM-native arrays of a FUSED read set, the reads of every gene.  The rule (csrc/spl_genecount_rule.h):
 *   gene map    of the set's coordinate space: ascending int32 start[n] with uint32 code[n], code[k] holding for the 0-based
 *               positions start[k] <= p < start[k + 1] (the last entry to +infinity; 0 below start[0]); 0 = no feature, g + 1 = only
 *               features of gene g (0 <= g < n_genes), 0xFFFFFFFF = features of two or more genes.  A map of 0 entries is valid;
 *   maps        stranded = 0: map a serves every read.  stranded = 1 (fr) / 2 (rf): map a serves the reads check_strand's rule
 *               (:374-406) calls '+', map b those it calls '-';
 *   eligible    (flag & (0x4 | 0x100 | 0x200 | 0x800)) == 0, POS >= 1 and at least one op; duplicates count.  Every other read
 *               the set holds is "not counted";
 *   blocks      spl_coverage's walk from the 0-based p = POS - 1 + the segment's shift, in int64: M, = and X cover, D and N are
 *               gaps, covering ops that abut are one block; nothing is clipped to a length;
 *   gene set    the union, over every stretch of the read's map that a block overlaps by a base or more, of the stretch's code:
 *               empty = "no feature", exactly one gene = one more read of that gene, anything else = "ambiguous" (htseq-count
 *               --mode union --nonunique none and featureCounts' default, per READ: a paired fragment adds up to two;
 *               spl_gene_count_fragments, below, counts a fragment once).
 * inout[0 .. n_genes) += the genes' reads, inout[n_genes] += no feature, [n_genes + 1] += ambiguous, [n_genes + 2] += not counted:
 * what is ADDED sums to the reads of the set.  The call synchronises; integer sums, exact and the same for the reads in any order
 * (one atomic per run of equal results in a wave: a gene that takes every read is no slower).  Parity with htseq-count /
 * featureCounts is intended and not pinned by a test.  A set without a single read adds nothing.  SPL_ERR_ARG: null arguments; a
 * set that is not fused; stranded outside 0..2; a start that is not strictly ascending; a code above n_genes that is not
 * 0xFFFFFFFF; n_genes above 0xFFFFFFF0.  The context stays usable after a refusal.
 * spl_gene_count_rule_host: the same rule for one read on the host (test hook; no file, no GPU): *result_out = the gene's index,
 * -1 no feature, -2 ambiguous, -3 not counted. */
int spl_gene_count(spl_ctx *ctx, const spl_dreads *dr, int stranded, int64_t n_a, const int32_t *a_start, const uint32_t *a_code, int64_t n_b,
                   const int32_t *b_start, const uint32_t *b_code, int64_t n_genes, int64_t *inout /* n_genes + 3 */);
int spl_gene_count_rule_host(uint32_t flag, int32_t pos, const uint32_t *ops, uint32_t n_ops, int32_t shift, int stranded, int64_t n_a,
                             const int32_t *a_start, const uint32_t *a_code, int64_t n_b, const int32_t *b_start, const uint32_t *b_code,
                             int64_t n_genes, int64_t *result_out);

/* ---- mates and fragments (paired-end libraries: count a fragment once) ----------------------------------------------------------
 * Replaces the name-sorted pass of `htseq-count` / `featureCounts -p --countReadPairs`, which count FRAGMENTS of a paired-end
 * library.  The reference has no counterpart.  The rule is csrc/spl_mate_rule.h, which the kernels and the host hooks compile alike:
 *   name key    64 bits of the QNAME as the file has it (BAM: l_read_name - 1 bytes, SAM: column 1): FNV-1a over the bytes (from
 *               0xcbf29ce484222325, per byte h = (h ^ b) * 0x100000001b3), then h ^= h >> 33, h *= 0xff51afd7ed558ccd, h ^= h >> 33,
 *               h *= 0xc4ceb9fe1a85ec53, h ^= h >> 33, mod 2^64.  An empty name and `*` have key 0, "no name"; another name whose
 *               hash is 0 has key 1.  A decode leaves the keys beside FLAG when asked to (spl_bam_set_mate_keys);
 *   pairable    a read that is eligible as for spl_gene_count, has flag 0x1, exactly one of 0x40 and 0x80, and a key that is not 0;
 *   group       the pairable reads of ONE SEGMENT (a chromosome's reads) whose keys agree in their upper 63 bits;
 *   mates       within a group, in the segment's order, the j-th first read (0x40) and the j-th second read (0x80); every other
 *               read has no mate.  A group is one first and one second read unless a name occurs twice or two names' 63 bits
 *               collide: then two fragments of one chromosome may swap mates.  For n distinct names on a chromosome about
 *               n^2 / 2^64 colliding pairs are expected, 5e-6 for 10 M names (derived, not measured);
 *   fragment    a read that is not eligible is "not counted", one per read.  An eligible read whose mate has a lower index adds
 *               nothing.  Every other eligible read folds its blocks over the map of its own strand and, if it has a mate, the
 *               mate's blocks over the map of the mate's strand (by the mate's own flag) into one gene set: empty = "no feature", one
 *               gene = that gene, else "ambiguous".  What is added sums to the reads minus the pairs.
 * Deliberate differences from the tools: a pair split over two chromosomes, or with one mate filtered out of the decode, counts as
 * two single-end fragments; names are compared by 63 hash bits.  Parity with htseq-count / featureCounts -p is intended and not
 * pinned by a test; the yardstick is tests/matecases.py.
 * spl_mate_table: the table of segment `seg` -- counted over the segments that have reads, in the order they were added; a set
 * without a read has none and gives three zeros -- of a finished, FUSED read set whose arrays have name keys, made on the device at the
 * first call (for every segment: the pairable reads compacted to (key with bit 0 = the kind, index), eight stable passes of the
 * radix sort of spl_sort.hip, then per element three binary searches: O(n log n) whatever the groups; scratch 2 x 12 bytes a
 * pairable read of the largest segment) and kept with the set, 4 bytes a read.  host_out (or null): a word per read of the
 * segment, the mate's index within the segment or 0xFFFFFFFF; the table is symmetric.  counts (or null): [0] pairable reads, [1]
 * reads with a mate (twice the pairs), [2] pairable reads without a mate whose flag has 0x8 clear (a mapped mate that was not
 * found on the chromosome).  SPL_ERR_ARG: a set that is not finished or not fused, or whose arrays have no name keys; no such segment.
 * spl_gene_count_fragments: spl_gene_count's arguments and output, counted per fragment by that table.
 * Test hooks, no GPU: spl_name_key_host (the key of len bytes), spl_mate_table_host (the table of one segment's host arrays: the
 * pair stage's body as the kernel runs it, behind a stable sort on the host), spl_gene_fragment_rule_host (per read of one
 * segment's host arrays and its table: the gene's index, -1 no feature, -2 ambiguous, -3 not counted, -4 nothing: the leader counts). */
int spl_mate_table(spl_ctx *ctx, const spl_dreads *dr, int seg, uint32_t *host_out /* the segment's reads, or null */, int64_t *counts /* 3, or null */);
int spl_gene_count_fragments(spl_ctx *ctx, const spl_dreads *dr, int stranded, int64_t n_a, const int32_t *a_start, const uint32_t *a_code, int64_t n_b,
                             const int32_t *b_start, const uint32_t *b_code, int64_t n_genes, int64_t *inout /* n_genes + 3 */);
int spl_name_key_host(const uint8_t *bytes, int64_t len, uint64_t *out);
int spl_mate_table_host(int64_t n_reads, const int32_t *pos, const uint16_t *flag, const uint32_t *cig_off, const uint64_t *name_key, uint32_t *mate_out,
                        int64_t *counts /* 3, or null */);
int spl_gene_fragment_rule_host(int64_t n_reads, const int32_t *pos, const uint16_t *flag, const uint32_t *cig_off, const uint32_t *cigar, const uint32_t *mate,
                                int32_t shift, int stranded, int64_t n_a, const int32_t *a_start, const uint32_t *a_code, int64_t n_b, const int32_t *b_start,
                                const uint32_t *b_code, int64_t n_genes, int64_t *results_out /* n_reads */);

/* ---- a reproducible fraction of a set's reads ----------------------------------------------------------------------------------
 * Replaces `samtools view -s SEED.FRAC` in front of another run of the whole pipeline (twenty of them for a saturation curve; RSeQC's
 * junction_saturation.py makes one of junctions, from a sorted file, in a Python loop).  The reference has no counterpart.  The rule
 * is csrc/spl_subsample_rule.h, which the kernels and the host hook compile alike.  A read's decision depends on its name and the
 * seed only:
 *   k = name key (above);  if k == 0 ("no name"):  k = (uint64)(uint32)POS << 32 | (uint64)FLAG << 16 | (n_ops & 0xffff)
 *   z = k ^ (seed * 0x9e3779b97f4a7c15)                                                              (mod 2^64)
 *   z = (z ^ z >> 30) * 0xbf58476d1ce4e5b9;  z = (z ^ z >> 27) * 0x94d049bb133111eb;  z ^= z >> 31
 *   u = z >> 32;   keep  <=>  u < threshold,   threshold in 0 .. 2^32  (2^32 keeps every read, 0 none)
 * POS is the file's 1-based position, before any shard shift.  So both mates of a pair, and every secondary and supplementary
 * record of a name, share one decision; for one seed the kept sets are nested (T1 <= T2: kept(T1) is a subset of kept(T2)); and the
 * decision depends neither on the reads' order nor on the container.  Parity with samtools' choice of reads is not intended and
 * would mean nothing for a random subset.
 * spl_reads_subsample: `dr` is a finished, FUSED read set whose arrays have name keys; *out is a finished, fused set on new arrays
 * that it owns -- the kept reads in their order (an order-preserving compaction on the device: two launches, a tile of
 * spl_subsample_tile() reads a wave, a scan of the tiles' totals between them, no atomics: the same words from run to run), the
 * segments of `dr` with their shifts (a segment that keeps no read is none of *out's, as a chromosome without a read is none of any
 * set's), strand bytes and name keys carried when `dr` has them.  Whatever takes a finished fused set takes *out, this call
 * included.  `dr` is untouched and may be freed before or after *out.  kept_per_seg (or null): per segment of `dr` that has reads,
 * in the order they were added, the reads kept.  kept_index_out (or null; room for every read of `dr`): the number within `dr` of
 * the i-th read of *out.  A set without a read gives a set without a read, and so does a selection that keeps none.  SPL_ERR_ARG,
 * after which the context stays usable: a set that is not finished, not fused or without name keys; a threshold beyond 2^32.
 * Test hooks: spl_subsample_keep_host (no GPU: the rule over one segment's host arrays, keep_out[i] = 1 where read i is kept),
 * spl_subsample_tile (the kernels' tile).  spl_reads_n_segments: the segments of a set that have reads, in the order they were
 * added -- the entries kept_per_seg gets, the numbers spl_mate_table takes. */
int spl_reads_subsample(spl_ctx *ctx, const spl_dreads *dr, uint64_t seed, uint64_t threshold, spl_dreads **out, int64_t *kept_per_seg /* n_seg, or NULL */,
                        uint32_t *kept_index_out /* or NULL */);
int spl_subsample_keep_host(int64_t n, const uint64_t *name_key, const int32_t *pos, const uint16_t *flag, const uint32_t *cig_off, uint64_t seed, uint64_t threshold,
                            uint8_t *keep_out);
int spl_subsample_tile(void);
int spl_reads_n_segments(const spl_dreads *dr, int64_t *out);

/* ---- PCR duplicates ------------------------------------------------------------------------------------------------------------
 * Replaces Picard MarkDuplicates / `samtools fixmate` + `samtools markdup` in front of --excludeFlags 0x400: both want a
 * coordinate-sorted copy of the file and rewrite it.  The reference has no counterpart.  The rule is csrc/spl_dup_rule.h, which
 * the kernels (csrc/spl_dups.hip) and the host hook compile alike; tests/dupcases.py restates it.  Per segment of a finished,
 * FUSED set with name keys:
 *   EXAMINED: mapped, primary, QC-passed, not supplementary, POS >= 1, an op at least (an incoming 0x400 is ignored); every other
 *   record is never marked.
 *   FRAGMENTS, over the segment's mate table: an examined read with a mate of higher index LEADS a pair fragment; one without a mate
 *   leads a single fragment; the other read of a pair belongs to its leader's fragment.  examined = 2 * pairs + singles.
 *   THE UNCLIPPED 5' END of a read: cl / ct = the sum of the S and H ops before the first / after the last op that is neither
 *   (every op a clip: cl is their sum, ct = 0), L = the sum of the M, D, N, =, X lengths, o = FLAG bit 0x10;
 *   u = POS - cl when o = 0, else POS + L - 1 + ct, in 64 bits, clamped to [-2^31, 2^31 - 1].
 *   THE SIGNATURE: for a pair, end A is the smaller of the two reads' ends by (u, o), on a tie the read with FLAG 0x40; B the other.
 *     W0 = (uA + 2^31) << 3 | oA << 2 | paired << 1 | (paired && A's read has 0x40)
 *     W1 = paired ? (uB + 2^31) << 1 | oB : 0
 *     W2 = the name key (both mates share it; 0 for a nameless read)
 *   DUPLICATES: fragments of one segment with equal (W0, W1) are a group; the one with the smallest W2 is its representative, ties
 *   to the lowest leader index; every other fragment is a duplicate, and both of its reads are marked.
 * The same NAMES are marked whatever the file's order or container -- for named reads only (nameless fragments tie at W2 = 0).
 * Deliberate differences from Picard and samtools (parity intended and unpinned; yardstick tests/dupcases.py): the representative
 * is chosen by name hash, not by quality sum (no qualities are decoded); a pair split over two chromosomes or by a decode filter is
 * two single fragments; singles compete only with singles; secondary, supplementary, QC-failed and unmapped records are never
 * marked; no optical duplicates, no UMIs.
 * spl_reads_duplicates: `seg` as for spl_mate_table, and SPL_ERR_ARG where that refuses.  The segment's marks are built at the
 * first call (the mate table first) and kept with the set, one byte a read.  host_out (or null): a byte per read of the segment, 1 =
 * duplicate.  counts (or null), seven: reads of the segment, examined, pair fragments, single fragments, duplicate pairs, duplicate
 * singles, examined reads whose incoming FLAG has 0x400.  hist (or null), 257: groups of 1 .. 255 fragments, of 256 or more, and
 * the fragments of the groups in that last bin.  Integer atomics only: the same words from run to run.
 * spl_reads_dedup: spl_reads_subsample's contract with the keep decision "not marked": *out is a finished, fused set on its own
 * arrays, segments and shifts, strand bytes and name keys carried; `dr` is untouched.
 * spl_duplicates_host (no GPU, test hook): the rule header over one segment's host arrays and its mate table behind a stable sort
 * on the host; dup_out: a byte per read; counts: seven; hist: 257, or null. */
int spl_reads_duplicates(spl_ctx *ctx, const spl_dreads *dr, int seg, uint8_t *host_out, int64_t *counts /* 7, or NULL */, int64_t *hist /* 257, or NULL */);
int spl_reads_dedup(spl_ctx *ctx, const spl_dreads *dr, spl_dreads **out, int64_t *kept_per_seg /* n_seg, or NULL */, uint32_t *kept_index_out /* or NULL */);
int spl_duplicates_host(int64_t n_reads, const int32_t *pos, const uint16_t *flag, const uint32_t *cig_off, const uint32_t *cigar, const uint64_t *name_key, const uint32_t *mate,
                        uint8_t *dup_out, int64_t *counts /* 7 */, int64_t *hist /* 257, or NULL */);

/* ---- the lanes of the counting passes (test hook, no GPU) ----------------------------------------------------------------------
 * Which stream a counting pass runs on and which recorded events it waits for is a rule of its own (csrc/spl_lanes.h; INTEGRATION.md,
 * "streams"), which spl_reads_relayout, spl_count_launch, spl_pass_barrier and the joins of every other entry point follow.
 * spl_lanes_plan_host runs that rule over a sequence of calls and hands back what each of them would queue.  calls: four int32 a call,
 * kind, a, b, c -- 0 relayout(set a, fused b), 1 count(table a, set b, piped c: the range kernel on a clean counter copy), 2 barrier,
 * 3 a download (join, the host waits), 4 other work on the main stream (a: behind a join).  out: 6 + 4 * 12 int64 a call -- the lane,
 * piped, the number of ops, how many of them stand behind the call's own launches, how many (before those) between the range kernel
 * and the tail, the tail's stream, then per op (1 wait / 2 record, the stream: 0 main, 1 second lane, 2 tail, the event's kind: 1 a
 * pass's range kernel, 2 a tail on the tail stream, 3 a marker on the main stream, 4 on the second lane, 5 a tail on the second lane,
 * its number).  two_lanes / tail_stream / callers_stream: the context's streams.  At most 64 tables and 64 sets. */
int spl_lanes_plan_host(int two_lanes, int tail_stream, int callers_stream, int n_tables, int n_sets, int64_t n_calls, const int32_t *calls, int64_t *out);

/* ---- per-exon-bin read counts (what the pipeline otherwise leaves to a second pass by another program) -----------------------
 * Replaces `featureCounts -f -O` / `dexseq_count.py` over the file this library has just decoded: whoever looks at a change in
 * splice-site strength also asks about exon usage (edgeR::diffSpliceDGE, DEXSeq), which needs reads per exon counting bin.  The
 * reference has no counterpart.  spl_exon_count counts, on the device, over the BAM-native arrays of a FUSED read set, the reads
 * of every bin of one chromosome.  The rule (csrc/spl_exoncount_rule.h):
 *   features    and selections are spl_gene_count's: a feature is an interval [left, right) of one gene, those with right <= left
 *               are ignored; unstranded, map a is made of all of a chromosome's features; stranded, map a of those whose strand is
 *               not '-', map b of those whose strand is not '+' (a '.' is in both);
 *   bins        for one selection, cut the chromosome at every left and every right of its features, and take a piece between two
 *               consecutive cuts: covered by no feature = code 0; by features of exactly one gene g = the BIN (g, start, end); by
 *               features of two or more genes = shared, code 0xFFFFFFFF, and no bin.  Two abutting exons of one gene are two bins;
 *               the same exon in two transcripts is one; the same (gene, start, end) out of both maps is one.  A chromosome's bins
 *               are numbered 0 .. n_bins - 1 in the order (start, end, gene) over the distinct triples of both maps;
 *   bin map     the shape of a gene map: ascending int32 start[n] with uint32 code[n], 0 = none, b + 1 = bin b, 0xFFFFFFFF =
 *               shared, an entry only where the code changes; bin_gene[n_bins] = every bin's gene, only ever compared for equality;
 *   a read      eligibility, map and blocks are spl_gene_count's (nothing clipped).  Its hit stretches are the stretches of its
 *               map that a block overlaps by a base or more, each taken ONCE however many of its blocks overlap it;
 *   verdict     any hit stretch shared, or two hit stretches with bins of different genes = "ambiguous", and NO bin is
 *               incremented; no hit stretch with a bin = "no feature"; otherwise "counted", and every hit stretch's bin gets + 1;
 *               every other read of the set is "not counted".
 * This is DEXSeq's counting (dexseq_count.py: reads with bins of more than one gene are _ambiguous) and `featureCounts -f -O`
 * restricted to reads of one gene, applied per READ: counting is per read, and a paired fragment adds up to two per bin
 * (spl_exon_count_fragments, below, counts a fragment once per bin).  Parity with DEXSeq / featureCounts is intended and
 * unpinned: it is not pinned by a test, neither tool being where this is built.  By construction a read's verdict is the one
 * spl_gene_count gives it on the gene maps of the same features.
 * inout[0 .. n_bins) += the bins' reads, inout[n_bins] += counted reads, [n_bins + 1] += no feature, [n_bins + 2] += ambiguous,
 * [n_bins + 3] += not counted: the last four ADDED sum to the reads of the set.  Bins are the chromosome's own: a call moves
 * n_bins + 4 words.  The call synchronises; integer sums, exact and the same for the reads in any order (one atomic per run of equal
 * bins in a wave and round).  SPL_ERR_ARG: spl_gene_count's own refusals; a code above n_bins that is not 0xFFFFFFFF; n_bins above
 * 0xFFFFFFF0; a null bin_gene with n_bins > 0.  The context stays usable after a refusal.
 * spl_exon_count_rule_host: the same rule for one read on the host (test hook; no file, no GPU): *verdict_out = 0 counted, -1 no
 * feature, -2 ambiguous, -3 not counted; bins_out[0 .. cap) = a counted read's bins in the order of their stretches, *n_hits_out =
 * their number, also beyond cap; any other verdict has no hit.
 * PER FRAGMENT (csrc/spl_exonfragment_rule.h; DEXSeq's paired counting, `featureCounts -f -O -p --countReadPairs`).  Mates, pairable
 * reads, groups and the leader are those of "mates and fragments" above; eligibility, maps, blocks, hit stretches and bins are
 * unchanged.  A read that is not eligible is "not counted", one per read.  An eligible read whose mate has a lower index in the
 * segment is silent: it adds nothing and enters no counter.  Every other eligible read is a fragment's leader, or a read without
 * a mate: its hit stretches are its own, over the map of its own strand, and, if it has a mate, the mate's, over the map of the
 * mate's strand (by the mate's own flag).  The verdict is taken over the UNION of both reads' hit stretches: any stretch shared,
 * or two stretches with bins of different genes = "ambiguous", and NO bin is incremented; no stretch with a bin = "no feature";
 * otherwise "counted", and every DISTINCT bin of the union gets + 1 -- a bin both mates hit counts once, whether they saw it
 * through the same map or through the two maps of a stranded run (a `.` feature).  The four verdict counters ADDED sum to the
 * reads minus the pairs; a fragment's verdict is the one spl_gene_count_fragments gives it on the gene maps of the same features.
 * How a bin is given once with nothing stored per read: one read's bins ascend strictly in bin number on either map (bins are
 * numbered over both maps), so a fragment's are the two-way merge of its reads' walks, equal heads given once.  The deliberate
 * differences from the tools are spl_gene_count_fragments' own (a pair split over chromosomes or by a filter counts as two
 * single-end fragments; names are compared by 63 hash bits); parity is intended and unpinned, the yardstick is
 * tests/exonfragcases.py.
 * spl_exon_count_fragments: spl_exon_count's arguments, output and refusals, and spl_mate_table's: SPL_ERR_ARG for a set without
 * name keys, not fused or not finished.  The mate table is made at the first call that needs it and kept with the set.
 * spl_exon_fragment_rule_host: the rule for every read of one segment's host arrays with its mate table (test hook; no GPU):
 * verdict_out[r] = 0 counted, -1 no feature, -2 ambiguous, -3 not counted, -4 silent; n_hits_out[r] = a counted leader's distinct
 * bins, all of them; bins_out[0 .. cap) = the counted leaders' merged bins, ascending within a fragment, one fragment after the
 * other in read order, as far as cap reaches.  A mate index at or beyond n_reads, or equal to r, means no mate. */
int spl_exon_count(spl_ctx *ctx, const spl_dreads *dr, int stranded, int64_t n_a, const int32_t *a_start, const uint32_t *a_code, int64_t n_b,
                   const int32_t *b_start, const uint32_t *b_code, int64_t n_bins, const uint32_t *bin_gene, int64_t *inout /* n_bins + 4 */);
int spl_exon_count_rule_host(uint32_t flag, int32_t pos, const uint32_t *ops, uint32_t n_ops, int32_t shift, int stranded, int64_t n_a,
                             const int32_t *a_start, const uint32_t *a_code, int64_t n_b, const int32_t *b_start, const uint32_t *b_code,
                             int64_t n_bins, const uint32_t *bin_gene, int64_t *verdict_out, int64_t *bins_out, int64_t cap,
                             int64_t *n_hits_out);
int spl_exon_count_fragments(spl_ctx *ctx, const spl_dreads *dr, int stranded, int64_t n_a, const int32_t *a_start, const uint32_t *a_code, int64_t n_b,
                             const int32_t *b_start, const uint32_t *b_code, int64_t n_bins, const uint32_t *bin_gene, int64_t *inout /* n_bins + 4 */);
int spl_exon_fragment_rule_host(int64_t n_reads, const int32_t *pos, const uint16_t *flag, const uint32_t *cig_off, const uint32_t *cigar, const uint32_t *mate,
                                int32_t shift, int stranded, int64_t n_a, const int32_t *a_start, const uint32_t *a_code, int64_t n_b, const int32_t *b_start,
                                const uint32_t *b_code, int64_t n_bins, const uint32_t *bin_gene, int64_t *verdict_out /* n_reads */,
                                int64_t *n_hits_out /* n_reads */, int64_t *bins_out, int64_t cap);

/* ---- intron depth (what the pipeline otherwise needs IRFinder or iREAD and a sorted BAM for) ------------------------------------
 * Replaces a second tool over the file this library has just decoded: how deeply every annotated intron is covered, beside the
 * change in SSE at its donor.  The reference has no counterpart.  The rule (csrc/spl_intron_rule.h; the command builds the
 * introns and their pieces: spliser_amd/intronretention.py):
 *   features    genecounts': the lines of type -t, their gene the value of --idAttr; unstranded ONE selection of all features
 *               with right > left, track '.'; stranded, selection a = the features whose strand is not '-', measured on the '+'
 *               track, selection b = those whose strand is not '+', on the '-' track;
 *   introns     per selection, chromosome and gene: the gene's features merged (overlapping or abutting ones are one interval);
 *               every gap [s, e), 0-based and half-open, between two consecutive merged intervals is an intron (gene, s, e,
 *               track); a gene of '.' features gives the same (gene, s, e) on both tracks, two rows;
 *   pieces      the intron minus the union of ALL features of its selection, of any gene, clipped to [0, length): sorted,
 *               disjoint [ps, pe); L = the sum of their lengths, which may be 0;
 *   depth       spl_coverage's on the intron's track (eligibility, walk, -split gaps and clipping of csrc/spl_coverage_rule.h).
 *               With D the ascending multiset of the depth at each of the L measurable bases and t = trim_percent (0..49):
 *               lo = (L * t) / 100, hi = L - lo, depth_n = hi - lo, depth_sum = the sum of D[lo .. hi), covered = #{d > 0}:
 *               int64, exact while depth_sum < 2^63, the same for the reads in any order; t = 0 is the plain sum;
 *   splicing    from the junction table of the same set (spl_junctions with knobs 0, 0, 0 and the command's `stranded`; under a
 *               stranded run only rows of the intron's track): an intron [s, e) is the junction left == s, right == e;
 *               splice_left = the counts of the junctions with left == s, splice_right of those with right == e, splice_exact
 *               of the one with both;
 *   IR ratio    depth = depth_sum / depth_n; IRratio = depth / (depth + max(splice_left, splice_right)); NA where depth_n == 0
 *               or the denominator is 0.
 * This is IRFinder's published measure (a trimmed mean over max-side splicing) as this project restates it; IRFinder is not on
 * the build machine: parity with it is intended and unpinned.
 * spl_intron_depth: runs spl_coverage's stages on the device over a FUSED, finished read set taken as the reads of ONE reference
 * of `length` bases, keeps their boundaries there, and takes the four numbers of every intron from them with one kernel
 * (csrc/spl_intron.hip); only `out` comes down: 4 per intron, L, covered, depth_n, depth_sum.  Intron i has the pieces
 * piece_off[i] .. piece_off[i + 1] of (piece_start, piece_end).  Pieces of different introns may overlap.  A set without a read:
 * every intron is L, 0, depth_n, 0.  SPL_ERR_ARG (the context stays usable): spl_coverage's refusals; a null argument;
 * trim_percent outside 0..49; piece_off not non-decreasing from 0; a piece with end <= start or outside [0, length]; pieces of
 * ONE intron not strictly ascending and disjoint.  n_introns = 0 is valid.
 * spl_intron_depth_runs: the same kernel and checks over a caller's boundaries, which are uploaded (test hook; no reads, no
 * file): bound_pos strictly ascending (else SPL_ERR_ARG), bound_depth[k] holds from bound_pos[k] to bound_pos[k + 1], the last to
 * the end, 0 before the first; n_bound = 0 is valid.
 * spl_intron_depth_host: the rule for ONE intron on the host by another method -- (depth, bases) pairs collected, sorted and
 * walked (test hook; no GPU): out4 = L, covered, depth_n, depth_sum. */
int spl_intron_depth(spl_ctx *ctx, const spl_dreads *dr, int64_t length, int stranded, int strand /* 0, '+', '-' */, int64_t n_introns,
                     const int64_t *piece_off /* n_introns + 1 */, const int32_t *piece_start, const int32_t *piece_end, int trim_percent,
                     int64_t *out /* 4 per intron */);
int spl_intron_depth_runs(spl_ctx *ctx, int64_t n_bound, const int32_t *bound_pos, const uint32_t *bound_depth, int64_t length,
                          int64_t n_introns, const int64_t *piece_off, const int32_t *piece_start, const int32_t *piece_end,
                          int trim_percent, int64_t *out);
int spl_intron_depth_host(int64_t n_bound, const int32_t *bound_pos, const uint32_t *bound_depth, int64_t n_pieces,
                          const int32_t *piece_start, const int32_t *piece_end, int trim_percent, int64_t *out4);

/* ---- the fused counting kernel's rule for simple reads, on the host (test hook; no file, no GPU) ---------------------------
 * A simple read (one aligned op) with bases [a, b), a = pos + shift, b = a + len, counts for the sites t with t and t + 1 both under it: the
 * distinct positions [lo, ub), lo = number of site positions <= a - 1, ub = number of site positions < b - 1.  The kernel asks one
 * question for the simple reads of a thread together: with a_min the least a and b_max the greatest b among them, the thread is
 * FLAGGED when ub(b_max) > lo(a_min); a thread that is not flagged has no simple read with a range.  A flagged thread's simple
 * reads are then looked at one by one.  site_pos: n_pos >= 1 strictly ascending positions in [0, 2^31 - 67] (the shard coordinate space); the reads of
 * thread t are [t * reads_per_thread, (t + 1) * reads_per_thread) of pos / len / is_simple, in any order of position.
 * flagged[n_threads]; emits / lo / ub[n_threads * reads_per_thread]: for a flagged thread's simple reads the range and whether it
 * is not empty, 0 for every other read.  SPL_ERR_RANGE: a simple read outside that space. */
int spl_simple_span_host(const int32_t *site_pos, int64_t n_pos, int64_t n_threads, int reads_per_thread, const int32_t *pos,
                         const uint16_t *len, const uint8_t *is_simple, int32_t shift, uint8_t *flagged, uint8_t *emits, int32_t *lo,
                         int32_t *ub);

/* ---- the position index of an uploaded site table, read back (test hooks; no product path calls them) ----------------------
 * The index every counting kernel finds its sites through: one entry per 32-base bucket counted from dbase, bucket b beginning at
 * start = dbase + 32 b -- first: the number of distinct site positions below start; occ: bit k set when start + k is a site
 * position; rival: bit k set when start + k is an end of a junction that has rivals (a partner or competitor position of a row
 * that has both lists; not necessarily a site).  dbase = lo - 64 (-64 when lo < 64) and n_dbuckets = ((hi - dbase) >> 5) + 2, lo
 * and hi the least and the greatest of the site and flagged positions; a table without rows has no buckets.
 * spl_sites_index_info: any output may be NULL.  spl_sites_index_download: buckets [first_bucket, first_bucket + count) into out,
 * three words a bucket (first, occ, rival); it waits for the context's stream first.  SPL_ERR_ARG: a null argument,
 * first_bucket + count > n_dbuckets. */
int spl_sites_index_info(const spl_dsites *ds, int32_t *dbase, uint32_t *n_dbuckets, int32_t *n_dpos);
int spl_sites_index_download(spl_ctx *ctx, const spl_dsites *ds, uint32_t first_bucket, uint32_t count,
                             uint32_t *out /* 3 words a bucket: first, occ, rival */);

/* ---- junction strand from the genome's splice motifs (what the pipeline otherwise needs the aligner's XS:A tag for) ----------
 * For a file whose aligner was not asked for the tag (STAR writes it only with --outSAMstrandField intronMotif; BWA, minimap2 and
 * GSNAP never do) the strand of a junction is in the genome: the intron's first and last two bases.  The reference has no
 * counterpart: it reads the strand a BED line says.  The rule (csrc/spl_motif_rule.h; the yardstick is tests/motifcases.py):
 *   base codes   four bits: A = 1, C = 2, G = 4, T = 8 in either letter case, every other byte 0.
 *   FASTA        a line that begins with '>' opens a sequence, its name the bytes behind '>' up to the first space, tab, CR or the
 *                line's end; every other line is a sequence line, each byte of it a base except one CR directly in front of the
 *                newline.  Any line lengths, empty lines skipped, a last line without a newline taken, a sequence of no bases
 *                legal.  SPL_ERR_FORMAT, the message naming the 1-based line ("line N"): bytes before the first '>', an empty name,
 *                a repeated name, no sequence; and a file that begins 1f 8b (pass the uncompressed FASTA the aligner's index was
 *                built from).  Plain text only, no .fai.
 *   motif code   of a junction (left, right) in spl_junctions' site convention: donor pair = bases left + 1, left + 2, acceptor
 *                pair = bases right - 1, right; 1 GT..AG, 2 CT..AC, 3 GC..AG, 4 CT..GC, 5 AT..AC, 6 GT..AT (column 5 of STAR's
 *                SJ.out.tab), 0 everything else: a pair with a 0 base, right - left < 4, a pair outside [1, length].  Odd codes are
 *                '+', even ones that are not 0 are '-'.
 *   read strand  over ALL N ops of the read (the walk of csrc/spl_junction_walk.h with the knobs 0, 0, 0): '+' with a '+' code and
 *                no '-' code, '-' for the mirror case, 0 otherwise; 0 for a read that is unmapped (0x4), has POS < 1, no CIGAR or
 *                no N op.  STAR's intronMotif, except that reads of inconsistent motifs stay and count under '?'.
 * spl_genome_open maps the file and sends it up through the staging ring in windows of whole lines of about window_bytes (0 = the
 * SAM text's SPL_SAM_WINDOW_BYTES, 256 MiB; a test cuts them at 64 KiB), the window before being packed meanwhile: only the file
 * crosses the link.  STORED FORM: two codes a byte, base p (1-based) of a sequence in nibble p - 1 from the sequence's first byte,
 * the low nibble first; every sequence starts on a 16-byte boundary.  spl_genome_name: the pointer is good while the handle is.
 * spl_genome_bases: bases first + 1 .. first + n of sequence i, a code a byte (test hook).  spl_genome_stats: the file's bytes, the
 * store's bytes, the device time of the copies and of the kernels.  spl_genome_free: while nothing uses the handle.
 * spl_genome_pack_host: the same rule on the host, no GPU -- the three counts are always written; name_off[n_seq + 1] / names (end
 * to end) / length[n_seq] / codes (a code a byte, end to end) where given and cap_seq, cap_names, cap_codes are enough.
 * spl_reads_motif_strand OVERWRITES the strand byte of every read of a FUSED set whose arrays have the bytes
 * (spl_reads_has_strand; anything else is SPL_ERR_ARG, as spl_junctions' stranded = 3) by the rule, against sequence `seq`, the
 * reads' POS moved by their segment's shift; the set stays fused.  tally_out[12]: junction walks by code 0 .. 6, then reads given
 * '+', '-', conflicting, spliced without a canonical junction, with a pair outside the sequence.  The call synchronises.
 * spl_motif_read_strand_host: the rule over host arrays and a sequence with a code a byte (test hook; offsets beyond n_ops_total
 * are an empty CIGAR).  spl_junction_motifs: code_out[i] for row i of a junction table; _host the same without a GPU. */
typedef struct spl_genome spl_genome;
int spl_genome_open(spl_ctx *ctx, const char *fasta_path, int64_t window_bytes, spl_genome **out);
int spl_genome_n(const spl_genome *g);
int spl_genome_name(const spl_genome *g, int i, const char **name_out, int64_t *length_out);
int spl_genome_bases(const spl_ctx *ctx, const spl_genome *g, int i, int64_t first, int64_t n, uint8_t *codes_out);
int spl_genome_stats(const spl_genome *g, int64_t *text_bytes, int64_t *device_bytes, float *upload_ms, float *pack_ms);
void spl_genome_free(spl_ctx *ctx, spl_genome *g);
int spl_genome_pack_host(const uint8_t *text, int64_t len, int64_t *n_seq_out, int64_t *name_bytes_out, int64_t *n_codes_out, int64_t cap_seq,
                         int64_t cap_names, int64_t cap_codes, int64_t *name_off, uint8_t *names, int64_t *length, uint8_t *codes);
int spl_reads_motif_strand(spl_ctx *ctx, spl_dreads *dr, const spl_genome *g, int seq, int64_t *tally_out);
int spl_motif_read_strand_host(int64_t n_reads, const int32_t *pos, const uint16_t *flag, const uint32_t *cig_off, const uint32_t *cigar,
                               int64_t n_ops_total, int32_t shift, const uint8_t *codes, int64_t length, uint8_t *strand_out, int64_t *tally_out);
int spl_junction_motifs(spl_ctx *ctx, const spl_genome *g, int seq, int64_t n, const int32_t *left, const int32_t *right, uint8_t *code_out);
int spl_junction_motifs_host(const uint8_t *codes, int64_t length, int64_t n, const int32_t *left, const int32_t *right, uint8_t *code_out);

/* ---- host helper of Step 1 ---------------------------------------------------------------------------
 * binary_gene_search (SpliSER_v0_1_8.py:118-173) for a batch of query positions against one chromosome's gene list
 * (in list order), probe for probe like the reference.  Strand bytes are '+', '-' or 0 for anything else;
 * out[q] = index of the gene found or -1.  No GPU involved. */
int spl_gene_search(const int64_t *left, const int64_t *right, const uint8_t *gene_strand, int64_t n_genes,
                    const int64_t *q_pos, const uint8_t *q_strand, int64_t n_queries, int is_stranded, int32_t *out);

/* ---- host helpers of Steps 0-1: the text inputs as columns ----------------------------------------------------------------
 * spl_bed_open: every line of exactly 12 tab-separated columns of a BED12 junction file as findAlphaCounts reads it
 * (SpliSER_v0_1_8.py:257-277): chromosome (index into the file's chromosome names, first-appearance order), left = chromStart +
 * blockSizes[0], right = chromEnd - blockSizes[1], alpha = score, strand byte (0 = empty column).  spl_gff_open: every `gene`
 * line of a GFF / GTF file as createGenes keeps it (:81-87, HTSeq conventions): chromosome, left = column 4 - 1, right = column 5,
 * strand byte, name = value of the first attribute.  Both fail with SPL_ERR_FORMAT on anything they are not sure to read the way
 * the reference's Python would (the caller then reads line by line).  No GPU involved. */
typedef struct spl_textfile spl_textfile;
int spl_bed_open(const char *path, spl_textfile **out);
int spl_gff_open(const char *path, spl_textfile **out);
void spl_text_close(spl_textfile *t);
int64_t spl_text_rows(const spl_textfile *t);
int32_t spl_text_n_chrom(const spl_textfile *t);
const char *spl_text_chrom_name(const spl_textfile *t, int32_t k);
const int32_t *spl_text_chrom(const spl_textfile *t);                 /* [rows] */
const int64_t *spl_text_i64(const spl_textfile *t, int which);        /* [rows] which: 0 left, 1 right, 2 alpha (BED) */
const uint8_t *spl_text_strand(const spl_textfile *t);                /* [rows] */
const char *spl_text_names(const spl_textfile *t, const uint32_t **off_out); /* GFF: gene names, one blob + rows + 1 offsets */

/* ---- output (outputBedFile, SpliSER_v0_1_8.py:641-664) -------------------------------------------------------
 * Appends the rows of one chromosome to a .SpliSER.tsv file (the caller writes the header line): 12 tab-separated
 * columns, SSE as "%.3f", the two cryptic columns as an integer and "%.5f" or "NA NA" when cryptic == 0, Partners as
 * Python's str(dict) "{pos: count, ...}" in partner order, Competitors as str(list).  Strand and gene texts come as one
 * blob each with n_sites + 1 offsets.  No GPU involved.  spl_tsv_append_many: the same for several chromosomes at once, in the
 * order given (their rows are formatted side by side). */
typedef struct spl_tsv_rows {
    const char *chrom;
    int64_t n_sites;
    const int64_t *pos;
    const char *strand_blob; const uint32_t *strand_off;
    const char *gene_blob; const uint32_t *gene_off;
    const double *sse;
    const int64_t *alpha;
    const uint32_t *beta1;
    const int64_t *beta2_simple, *beta2_cryptic; /* beta2_cryptic, beta2_weighted: read when cryptic != 0 */
    const double *beta2_weighted;
    const uint32_t *part_off; const int64_t *part_pos, *edge_cnt;
    const uint32_t *comp_off; const int64_t *comp_pos;
} spl_tsv_rows;
int spl_tsv_append_many(const char *path, int32_t n_chrom, const spl_tsv_rows *rows, int cryptic);
int spl_tsv_append(const char *path, const char *chrom, int64_t n_sites, const int64_t *pos, const char *strand_blob,
                   const uint32_t *strand_off, const char *gene_blob, const uint32_t *gene_off, const double *sse,
                   const int64_t *alpha, const uint32_t *beta1, const int64_t *beta2_simple, int cryptic,
                   const int64_t *beta2_cryptic, const double *beta2_weighted, const uint32_t *part_off,
                   const int64_t *part_pos, const int64_t *edge_cnt, const uint32_t *comp_off, const int64_t *comp_pos);

/* The writer's "%.3f" / "%.5f": x >= 0 with `digits` (0..6) decimals into out64 (NUL-terminated), correctly rounded from the
 * double's exact value, ties to even -- what Python's "{0:.3f}".format gives (SpliSER_v0_1_8.py:655-660).  Exported so that the
 * tests can hold it against Python over many values. */
int spl_fmt_fixed(double x, int digits, char *out64);

/* ---- `combine` / `combineShallow`: the host walk on columns (csrc/spl_combine.cpp) --------------------------------------------
 * Replaces the lock-step loop of SpliSER_v0_1_8.py:820-915 (combine) and :1007-1166 (combineShallow) around the calls of
 * checkBam (:903): spl_combine_open parses the per-sample .SpliSER.tsv files into columns (SPL_ERR_FORMAT on anything it is
 * not sure to read the way Python's str.split / int / float / literal_eval would: the caller then walks the files in Python);
 * spl_combine_region_runs gives what the region order (:761-790) is deduced from; spl_combine_merge is the walk -- merged
 * sites in output order, and for every sample the gap-fill queries as tables (rows by position per region; strand, partners
 * and competitors as the walk had them when it reached that sample); the queries are answered through spl_count in
 * combine mode and handed back with spl_combine_answers; spl_combine_write is outputCombinedLines (:722-740).  No GPU. */
typedef struct spl_combine spl_combine;
typedef struct spl_query_table {
    const char *chrom;            /* region name */
    int64_t n;                    /* rows */
    const int64_t *pos;           /* [n] site positions, ascending */
    const int64_t *site;          /* [n] index of the merged site a row answers */
    const uint8_t *strand;        /* [n] first byte of the site's strand text at that moment, 0 if it had none */
    const uint32_t *part_off;     /* [n + 1] */
    const int64_t *part_pos;      /* partner positions (one-way lists) */
    const uint32_t *comp_off;     /* [n + 1] */
    const int64_t *comp_pos;      /* competitor positions */
} spl_query_table;
int spl_combine_open(const char *const *tsv_paths, int32_t n_samples, spl_combine **out);
void spl_combine_close(spl_combine *c);
int64_t spl_combine_rows(const spl_combine *c, int32_t idx);
int32_t spl_combine_n_texts(const spl_combine *c);
const char *spl_combine_text(const spl_combine *c, int32_t id);
int64_t spl_combine_region_runs(const spl_combine *c, int32_t idx, int32_t *ids, int64_t cap);
int spl_combine_keep_gene(spl_combine *c, const char *gene);
int spl_combine_merge(spl_combine *c, const char *const *chroms, int32_t n_chroms, int is_stranded, const char *q_gene, int shallow,
                      int64_t min_samples, int64_t min_reads, double min_sse);
int64_t spl_combine_n_sites(const spl_combine *c);
int64_t spl_combine_n_gap_sites(const spl_combine *c);
int64_t spl_combine_skipped(const spl_combine *c, const int64_t **pairs);
int32_t spl_combine_n_tables(const spl_combine *c, int32_t idx);
int spl_combine_table(const spl_combine *c, int32_t idx, int32_t k, spl_query_table *out);
int spl_combine_answers(spl_combine *c, int32_t idx, int64_t n, const int64_t *site, const uint32_t *beta1, const uint32_t *beta2_simple);
int spl_combine_write(const spl_combine *c, const char *path, const char *const *titles, int cryptic);

/* str(x) of a Python float (the beta2_weighted column of .combined.tsv, :735) into out64, NUL-terminated.  Test hook. */
int spl_fmt_repr(double x, char *out64);

#ifdef __cplusplus
}
#endif
#endif /* SPLISER_H */
