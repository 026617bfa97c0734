"""ctypes binding of libspliser_hip.so (C ABI: include/spliser.h).

This is the only door to the compute path.  There is no Python/numpy fallback: if the shared library
is missing or no MI355X is visible, every entry point raises -- loudly -- instead of computing on the
host.
"""
import ctypes
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
# SPLISER_HIP_LIB: load another build of the same library (A/B runs of two builds on one box)
LIB_PATH = os.environ.get("SPLISER_HIP_LIB") or os.path.join(HERE, "libspliser_hip.so")
CSRC = os.path.join(HERE, "csrc")

STRANDED_CODE = {None: 0, False: 0, "": 0, "fr": 1, "rf": 2}
COORD_MAX = 2147483581   # csrc/spl_pack.h's SPL_COORD_MAX: read ends and site positions stay at or below it (``shard.COORD_MAX`` is this)
STRAND_FROM_XS = 3   # spl_junctions' fourth mode: a junction's strand is its read's strand byte (the aligner's XS:A tag)


class SpliserNativeError(RuntimeError):
    def __init__(self, code, message):
        RuntimeError.__init__(self, "libspliser_hip error %d: %s" % (code, message))
        self.code = code


class spl_sites(ctypes.Structure):
    _fields_ = [("n_sites", ctypes.c_int64), ("pos", ctypes.c_void_p), ("strand", ctypes.c_void_p),
                ("part_off", ctypes.c_void_p), ("part_pos", ctypes.c_void_p), ("part_site", ctypes.c_void_p),
                ("comp_off", ctypes.c_void_p), ("comp_pos", ctypes.c_void_p), ("alpha", ctypes.c_void_p),
                ("edge_cnt", ctypes.c_void_p)]


class spl_reads(ctypes.Structure):
    _fields_ = [("n_reads", ctypes.c_int64), ("pos", ctypes.c_void_p), ("flag", ctypes.c_void_p),
                ("cig_off", ctypes.c_void_p), ("cigar", ctypes.c_void_p)]


class spl_opts(ctypes.Structure):
    _fields_ = [("stranded", ctypes.c_int32), ("combine_mode", ctypes.c_int32), ("flags", ctypes.c_int32)]


OPT_PAIR_KERNEL = 1
OPT_WAVE_AGGREGATION = 2   # (selects nothing: such a pass is the default one; kept for callers of ABI v1)


EXPORTS = [
    "spl_abi_version", "spl_last_error", "spl_device_count", "spl_trim", "spl_devmem_stats", "spl_devmem_probe", "spl_create", "spl_create_on_stream", "spl_destroy",
    "spl_sync", "spl_pass_barrier", "spl_timer_begin", "spl_timer_end", "spl_kernel_timing_begin", "spl_kernel_timing_collect", "spl_prof_enable", "spl_prof_report", "spl_count", "spl_sse", "spl_sites_upload", "spl_sites_free",
    "spl_reads_upload", "spl_reads_upload_segments", "spl_reads_begin", "spl_reads_begin_sized", "spl_reads_add", "spl_reads_add2", "spl_reads_add_bam", "spl_reads_add_bam_share", "spl_reads_finish",
    "spl_soa_upload", "spl_soa_upload2", "spl_soa_upload3", "spl_soa_upload4", "spl_reads_has_strand", "spl_reads_has_mate_keys", "spl_soa_free", "spl_reads_add_soa", "spl_reads_relayout", "spl_layout_timing_collect", "spl_reads_layout_bytes", "spl_reads_slots_download",
    "spl_pack_host", "spl_reads_free", "spl_count_launch", "spl_sse_launch", "spl_counters_download",
    "spl_sse_download", "spl_count_algorithmic_bytes", "spl_literal_queue_size", "spl_last_launch_info", "spl_bam_open", "spl_bam_open_stream", "spl_bam_open_deferred", "spl_bam_set_filter", "spl_bam_set_aux_strand", "spl_bam_set_mate_keys", "spl_bam_mate_keys", "spl_bam_aux_strand", "spl_bam_aux_strand_host", "spl_bam_filter_counts", "spl_bam_set_flagstat", "spl_bam_flagstat", "spl_flagstat_add_host", "spl_bam_set_any_order", "spl_bam_any_order_sorted", "spl_sort_keys_device", "spl_text_windows_host", "spl_text_line_index", "spl_bam_decode_device", "spl_bam_reserve_device", "spl_bam_share_plan", "spl_bam_share_range", "spl_bam_share_info", "spl_bam_share_count_host", "spl_bam_share_ref", "spl_bam_decode_device_share", "spl_bam_decoded_on_device", "spl_bam_wait_device", "spl_bam_start", "spl_bam_compression_ratio", "spl_bam_sample", "spl_bam_wait_ref", "spl_bam_wait_all", "spl_bam_cancel", "spl_bam_decline_reason", "spl_sam_open", "spl_bam_is_text", "spl_bam_text_compression", "spl_bam_text_blocks", "spl_bam_close",
    "spl_bam_n_ref", "spl_bam_ref_name", "spl_bam_ref_length", "spl_bam_n_records", "spl_bam_reads", "spl_bam_write", "spl_bam_write2",
    "spl_gene_search", "spl_junctions", "spl_junctions_get", "spl_junctions_stats", "spl_junction_walk_host", "spl_junctions_fragments", "spl_junction_fragment_rule_host", "spl_strand_tally", "spl_strand_rule_host", "spl_genome_open", "spl_genome_n", "spl_genome_name", "spl_genome_bases", "spl_genome_stats", "spl_genome_free", "spl_genome_pack_host", "spl_reads_motif_strand", "spl_motif_read_strand_host", "spl_junction_motifs", "spl_junction_motifs_host", "spl_coverage", "spl_coverage_totals", "spl_coverage_download", "spl_coverage_free", "spl_coverage_rule_host", "spl_bedgraph_append", "spl_coverage_fragments", "spl_coverage_fragment_totals", "spl_intron_depth_fragments", "spl_coverage_fragment_rule_host", "spl_coverage_cursor_host", "spl_gene_count", "spl_gene_count_rule_host", "spl_mate_table", "spl_gene_count_fragments", "spl_name_key_host", "spl_reads_subsample", "spl_subsample_keep_host", "spl_subsample_tile", "spl_reads_n_segments", "spl_reads_duplicates", "spl_reads_dedup", "spl_duplicates_host", "spl_lanes_plan_host", "spl_mate_table_host", "spl_gene_fragment_rule_host", "spl_exon_count", "spl_exon_count_rule_host", "spl_exon_count_fragments", "spl_exon_fragment_rule_host", "spl_intron_depth", "spl_intron_depth_runs", "spl_intron_depth_host", "spl_simple_span_host", "spl_sites_index_info", "spl_sites_index_download", "spl_tsv_append", "spl_tsv_append_many", "spl_fmt_fixed",
    "spl_bed_open", "spl_gff_open", "spl_text_close", "spl_text_rows", "spl_text_n_chrom", "spl_text_chrom_name", "spl_text_chrom",
    "spl_text_i64", "spl_text_strand", "spl_text_names",
    "spl_combine_open", "spl_combine_close", "spl_combine_rows", "spl_combine_n_texts", "spl_combine_text", "spl_combine_region_runs",
    "spl_combine_keep_gene", "spl_combine_merge", "spl_combine_n_sites", "spl_combine_n_gap_sites", "spl_combine_skipped",
    "spl_combine_n_tables", "spl_combine_table", "spl_combine_answers", "spl_combine_write", "spl_fmt_repr",
]

_lib = None


def build(force=False):
    """Compile libspliser_hip.so for gfx950 with hipcc (cross-compiles without a GPU)."""
    if force:
        subprocess.check_call(["make", "-s", "-C", CSRC, "clean"])
    subprocess.check_call(["make", "-s", "-C", CSRC])
    return LIB_PATH


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise SpliserNativeError(-2, "%s not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                                         "(hipcc, gfx950). There is no CPU fallback." % LIB_PATH)
        L = ctypes.CDLL(LIB_PATH)
        L.spl_last_error.restype = ctypes.c_char_p
        L.spl_bam_ref_name.restype = ctypes.c_char_p
        L.spl_bam_decline_reason.restype = ctypes.c_char_p
        L.spl_bam_ref_length.restype = ctypes.c_int64
        L.spl_bam_n_records.restype = ctypes.c_int64
        L.spl_bam_text_blocks.restype = ctypes.c_int64
        for name in ("spl_destroy", "spl_sites_free", "spl_reads_free", "spl_soa_free", "spl_bam_close", "spl_text_close", "spl_combine_close", "spl_coverage_free", "spl_genome_free"):
            getattr(L, name).restype = None
        for name in ("spl_combine_rows", "spl_combine_region_runs", "spl_combine_n_sites", "spl_combine_n_gap_sites", "spl_combine_skipped"):
            getattr(L, name).restype = ctypes.c_int64
        L.spl_combine_text.restype = ctypes.c_char_p
        L.spl_text_rows.restype = ctypes.c_int64
        L.spl_text_chrom_name.restype = ctypes.c_char_p
        for name in ("spl_text_chrom", "spl_text_i64", "spl_text_strand", "spl_text_names"):
            getattr(L, name).restype = ctypes.c_void_p
        if L.spl_abi_version() != 1:
            raise SpliserNativeError(-1, "ABI version mismatch")
        _lib = L
    return _lib


def _check(rc):
    if rc != 0:
        raise SpliserNativeError(rc, lib().spl_last_error().decode("utf-8", "replace"))


def _ptr(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _arr(a, dt):
    return np.ascontiguousarray(a, dtype=dt)


def _to_i32(a, what):
    a = np.asarray(a)
    if a.size and (a.max() > COORD_MAX or a.min() < -2147483648):
        raise SpliserNativeError(-6, "%s exceeds the int32 shard coordinate space; split the shard" % what)
    return _arr(a, np.int32)


def device_count():
    n = ctypes.c_int(0)
    _check(lib().spl_device_count(ctypes.byref(n)))
    return n.value


class SiteArrays(object):
    """Keeps the numpy arrays behind a ``spl_sites`` alive."""

    def __init__(self, pos, strand, part_off, part_pos, comp_off, comp_pos, part_site=None, alpha=None, edge_cnt=None):
        self.pos = _to_i32(pos, "site position")
        self.strand = _arr(strand, np.uint8)
        self.part_off = _arr(part_off, np.uint32)
        self.part_pos = _to_i32(part_pos, "partner position")
        self.comp_off = _arr(comp_off, np.uint32)
        self.comp_pos = _to_i32(comp_pos, "competitor position")
        self.part_site = None if part_site is None else _arr(part_site, np.int32)
        self.alpha = None if alpha is None else _arr(alpha, np.int64)
        self.edge_cnt = None if edge_cnt is None else _arr(edge_cnt, np.int64)
        self.n = int(self.pos.shape[0])
        self.n_part = int(self.part_off[-1]) if self.n else 0
        self.c = spl_sites(self.n, _ptr(self.pos), _ptr(self.strand), _ptr(self.part_off), _ptr(self.part_pos),
                           _ptr(self.part_site), _ptr(self.comp_off), _ptr(self.comp_pos), _ptr(self.alpha),
                           _ptr(self.edge_cnt))

    @classmethod
    def from_chrom(cls, arr, offset=0):
        """From sites.ChromArrays, optionally shifted into a shard coordinate space."""
        return cls(arr.pos + offset, arr.strand, arr.part_off, arr.part_pos + offset, arr.comp_off,
                   arr.comp_pos + offset, arr.part_site, arr.alpha, arr.edge_cnt)


class ReadArrays(object):
    """``xs``: None, or a strand byte per read ('+', '-', 0) for ``Context.upload_soa`` (``spl_soa_upload3``); ``name_key``: None, or a
    name key per read (uint64, 0 = no name) for ``Context.upload_soa`` (``spl_soa_upload4``); no other call reads them."""

    def __init__(self, pos, flag, cig_off, cigar, xs=None, name_key=None):
        self.xs = None if xs is None else _arr(xs, np.uint8)
        self.name_key = None if name_key is None else _arr(name_key, np.uint64)
        self.pos = _to_i32(pos, "read position")
        self.flag = _arr(flag, np.uint16)
        self.cig_off = _arr(cig_off, np.uint32)
        self.cigar = _arr(cigar, np.uint32)
        self.n = int(self.pos.shape[0])
        if self.cig_off.shape[0] != self.n + 1:
            raise ValueError("cig_off must have n_reads + 1 entries")
        if self.xs is not None and self.xs.shape[0] != self.n:
            raise ValueError("xs must have n_reads entries")
        if self.name_key is not None and self.name_key.shape[0] != self.n:
            raise ValueError("name_key must have n_reads entries")
        self.c = spl_reads(self.n, _ptr(self.pos), _ptr(self.flag), _ptr(self.cig_off), _ptr(self.cigar))


class Context(object):
    """One GPU + one stream (``spl_ctx``)."""

    def __init__(self, device=0, stream=None):
        self._h = ctypes.c_void_p()
        if stream is None:
            _check(lib().spl_create(ctypes.c_int(device), ctypes.byref(self._h)))
        else:
            _check(lib().spl_create_on_stream(ctypes.c_int(device), ctypes.c_void_p(stream), ctypes.byref(self._h)))
        self.device = device

    def close(self):
        if self._h:
            lib().spl_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- one-shot host-buffer calls ----------------------------------------------------------------
    def count(self, sites, reads, stranded=0, combine_mode=0, flags=0):
        """checkBam for all sites of a shard -> (beta1, beta2s_reads, dbl) uint32."""
        beta1 = np.zeros(max(sites.n, 1), np.uint32)
        b2s = np.zeros(max(sites.n, 1), np.uint32)
        dbl = np.zeros(max(sites.n_part, 1), np.uint32)
        opts = spl_opts(int(stranded), int(combine_mode), int(flags))
        _check(lib().spl_count(self._h, ctypes.byref(sites.c), ctypes.byref(reads.c), ctypes.byref(opts),
                               _ptr(beta1), _ptr(b2s), _ptr(dbl)))
        return beta1[:sites.n], b2s[:sites.n], dbl[:sites.n_part]

    def sse(self, sites, beta1, b2s_reads, dbl, cryptic):
        """findBeta2Counts + calculateSSE -> (beta2_simple, beta2_cryptic, beta2_weighted, sse)."""
        n = sites.n
        beta1, b2s_reads = _arr(beta1, np.uint32), _arr(b2s_reads, np.uint32)
        dbl = _arr(dbl if len(dbl) else np.zeros(1), np.uint32)
        o = [np.zeros(max(n, 1), np.int64), np.zeros(max(n, 1), np.int64), np.zeros(max(n, 1), np.float64),
             np.zeros(max(n, 1), np.float64)]
        _check(lib().spl_sse(self._h, ctypes.byref(sites.c), _ptr(beta1), _ptr(b2s_reads), _ptr(dbl),
                             ctypes.c_int(1 if cryptic else 0), _ptr(o[0]), _ptr(o[1]), _ptr(o[2]), _ptr(o[3])))
        return tuple(a[:n] for a in o)

    # -- device-resident pipeline --------------------------------------------------------------------
    def upload_sites(self, sites):
        h = ctypes.c_void_p()
        _check(lib().spl_sites_upload(self._h, ctypes.byref(sites.c), ctypes.byref(h)))
        return DeviceSites(self, h, sites.n, sites.n_part)

    def upload_reads(self, reads):
        h = ctypes.c_void_p()
        _check(lib().spl_reads_upload(self._h, ctypes.byref(reads.c), ctypes.byref(h)))
        return DeviceReads(self, h, reads.n)

    def begin_reads(self, expected_reads=0):
        """A read set to which segments are added one by one (``DeviceReads.add`` / ``add_bam``), then ``finish()``.
        ``expected_reads``: how many reads are going to be added, when known (sets of 64 M and more get larger chunks)."""
        h = ctypes.c_void_p()
        _check(lib().spl_reads_begin_sized(self._h, ctypes.c_int64(int(expected_reads)), ctypes.byref(h)))
        return DeviceReads(self, h, 0)

    def upload_read_segments(self, segments):
        """segments: [(ReadArrays-like with .c, position shift)] laid end to end as ONE device read set, copied straight
        from where they are (``spl_reads_upload_segments``)."""
        n = len(segments)
        segs = (spl_reads * max(n, 1))()
        shifts = (ctypes.c_int32 * max(n, 1))()
        total = 0
        for k, (reads, shift) in enumerate(segments):
            segs[k] = reads.c
            shifts[k] = int(shift)
            total += reads.n
        h = ctypes.c_void_p()
        _check(lib().spl_reads_upload_segments(self._h, ctypes.c_int(n), segs, shifts, ctypes.byref(h)))
        return DeviceReads(self, h, total)

    def upload_soa(self, segments, max_ends=None, with_strand=False, with_keys=False):
        """segments: [ReadArrays-like with .c] -> the BAM-native arrays as they are, laid end to end in device memory
        (``spl_soa_upload``): what a decode on the device leaves.  Read sets are laid out from them by the layout kernel
        (``DeviceReads.add_soa`` + ``finish``; ``relayout``).  ``max_ends``: per segment the last base its reads cover, if known.
        ``with_strand``: every segment's ``xs`` goes up as a fifth array (``spl_soa_upload3``), for ``junctions(STRAND_FROM_XS)``.
        ``with_keys``: every segment's ``name_key`` goes up beside it (``spl_soa_upload4``), for ``mate_table`` and
        ``gene_counts(fragments=True)``."""
        n = len(segments)
        segs = (spl_reads * max(n, 1))()
        for k, reads in enumerate(segments):
            segs[k] = reads.c
        h = ctypes.c_void_p()
        ends = None if max_ends is None else (ctypes.c_int64 * max(n, 1))(*[int(v) if v is not None else -1 for v in max_ends])
        if with_strand and any(r.xs is None for r in segments):
            raise ValueError("upload_soa(with_strand=True): every segment needs its xs array")
        xs = (ctypes.c_void_p * max(n, 1))(*[r.xs.ctypes.data for r in segments]) if with_strand else None
        if with_keys:
            if any(getattr(r, "name_key", None) is None for r in segments):
                raise ValueError("upload_soa(with_keys=True): every segment needs its name_key array")
            keys = (ctypes.c_void_p * max(n, 1))(*[r.name_key.ctypes.data for r in segments])
            _check(lib().spl_soa_upload4(self._h, ctypes.c_int(n), segs, ends, xs, keys, ctypes.byref(h)))
        elif with_strand:
            _check(lib().spl_soa_upload3(self._h, ctypes.c_int(n), segs, ends, xs, ctypes.byref(h)))
        else:
            _check(lib().spl_soa_upload2(self._h, ctypes.c_int(n), segs, ends, ctypes.byref(h)))
        return DeviceSoA(self, h, [r.n for r in segments])

    def layout_read_segments(self, soa, shifts):
        """One read set from all segments of a ``DeviceSoA``, segment k moved by shifts[k]: the layout kernel's launch is
        queued, nothing is waited for."""
        dr = self.begin_reads(sum(soa.n))
        try:
            for k, shift in enumerate(shifts):
                dr.add_soa(soa, k, shift)
            return dr.finish()
        except Exception:
            dr.free()
            raise

    def layout_timing_collect(self, capacity=4096):
        """Durations (ms) of the layout kernel's launches since ``kernel_timing_begin`` (before ``kernel_timing_collect``)."""
        ms = (ctypes.c_float * capacity)()
        n = ctypes.c_int(0)
        _check(lib().spl_layout_timing_collect(self._h, ms, ctypes.c_int(capacity), ctypes.byref(n)))
        return [ms[i] for i in range(n.value)]

    def count_launch(self, dsites, dreads, stranded=0, combine_mode=0, flags=0):
        opts = spl_opts(int(stranded), int(combine_mode), int(flags))
        _check(lib().spl_count_launch(self._h, dsites._h, dreads._h, ctypes.byref(opts)))

    def sse_launch(self, dsites, cryptic):
        _check(lib().spl_sse_launch(self._h, dsites._h, ctypes.c_int(1 if cryptic else 0)))

    def sync(self):
        _check(lib().spl_sync(self._h))

    def pass_barrier(self):
        """Later launches start after all earlier ones (tails of counting passes included) are done; the host does not wait."""
        _check(lib().spl_pass_barrier(self._h))

    def timer_begin(self):
        _check(lib().spl_timer_begin(self._h))

    def timer_end(self):
        ms = ctypes.c_float(0)
        _check(lib().spl_timer_end(self._h, ctypes.byref(ms)))
        return ms.value

    def kernel_timing_begin(self, max_records):
        _check(lib().spl_kernel_timing_begin(self._h, ctypes.c_int(max_records)))

    def kernel_timing_collect(self, capacity=4096):
        ms = (ctypes.c_float * capacity)()
        n = ctypes.c_int(0)
        _check(lib().spl_kernel_timing_collect(self._h, ms, ctypes.c_int(capacity), ctypes.byref(n)))
        return [ms[i] for i in range(n.value)]

    def launch_info(self):
        g, b, l = ctypes.c_int32(0), ctypes.c_int32(0), ctypes.c_int32(0)
        _check(lib().spl_last_launch_info(self._h, ctypes.byref(g), ctypes.byref(b), ctypes.byref(l)))
        return dict(grid=g.value, block=b.value, lds_bytes=l.value)


class DeviceSites(object):
    def __init__(self, ctx, h, n, n_part):
        self.ctx, self._h, self.n, self.n_part = ctx, h, n, n_part

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.free()

    def counters(self):
        beta1 = np.zeros(max(self.n, 1), np.uint32)
        b2s = np.zeros(max(self.n, 1), np.uint32)
        dbl = np.zeros(max(self.n_part, 1), np.uint32)
        _check(lib().spl_counters_download(self.ctx._h, self._h, _ptr(beta1), _ptr(b2s), _ptr(dbl)))
        return beta1[:self.n], b2s[:self.n], dbl[:self.n_part]

    def sse_results(self):
        n = self.n
        o = [np.zeros(max(n, 1), np.int64), np.zeros(max(n, 1), np.int64), np.zeros(max(n, 1), np.float64),
             np.zeros(max(n, 1), np.float64)]
        _check(lib().spl_sse_download(self.ctx._h, self._h, _ptr(o[0]), _ptr(o[1]), _ptr(o[2]), _ptr(o[3])))
        return tuple(a[:n] for a in o)

    def position_index(self, first=0, count=None):
        """The table's position index as the device holds it (test hook: ``spl_sites_index_info`` / ``spl_sites_index_download``)
        -> (dbase, n_dbuckets, n_dpos, uint32[count, 3]: first, occ, rival of buckets [first, first + count)); ``count`` None: all
        buckets from ``first`` on."""
        dbase, n_dbuckets, n_dpos = ctypes.c_int32(0), ctypes.c_uint32(0), ctypes.c_int32(0)
        _check(lib().spl_sites_index_info(self._h, ctypes.byref(dbase), ctypes.byref(n_dbuckets), ctypes.byref(n_dpos)))
        first = int(first)
        count = max(n_dbuckets.value - first, 0) if count is None else int(count)
        if first < 0 or count < 0 or first >= 1 << 32 or count >= 1 << 32:
            raise ValueError("position_index: first and count must fit uint32")
        out = np.zeros((max(count, 1), 3), np.uint32)
        _check(lib().spl_sites_index_download(self.ctx._h, self._h, ctypes.c_uint32(first), ctypes.c_uint32(count), _ptr(out)))
        return dbase.value, n_dbuckets.value, n_dpos.value, out[:count]

    def free(self):
        if self._h:
            lib().spl_sites_free(self.ctx._h, self._h)
            self._h = ctypes.c_void_p()


class DeviceReads(object):
    def __init__(self, ctx, h, n):
        self.ctx, self._h, self.n = ctx, h, n

    def add(self, reads, shift=0, max_end=None):
        """One more segment from host arrays (``ReadArrays``), moved by ``shift`` into the shard's coordinate space.  ``max_end``:
        the last base the reads cover, if known (a decoder's arrays, a kept file's)."""
        _check(lib().spl_reads_add2(self.ctx._h, self._h, ctypes.byref(reads.c), ctypes.c_int32(int(shift)),
                                    ctypes.c_int64(-1 if max_end is None else int(max_end))))
        self.n += reads.n

    def add_bam(self, bam, chrom, shift=0):
        """One more segment: the reads of reference ``chrom`` straight from the decoder's buffers (waits for that reference
        to be complete; the rest of the file may still be decoding).  -> number of reads added."""
        tid = bam._tid[chrom]
        n_reads, _ = bam.wait_ref(chrom)
        _check(lib().spl_reads_add_bam(self.ctx._h, self._h, bam._h, ctypes.c_int(tid), ctypes.c_int32(int(shift))))
        self.n += n_reads
        return n_reads

    def add_bam_share(self, bam, share, chrom, shift=0):
        """One more segment: what share ``share`` of a decode in shares holds of reference ``chrom``, from that share's arrays on
        this device (``BamFile.decode_on_devices_async``; the decoders must be done: ``join_decoders``).  -> number of reads added."""
        n_reads, _ = bam.share_ref(share, chrom)
        if n_reads:
            _check(lib().spl_reads_add_bam_share(self.ctx._h, self._h, bam._h, ctypes.c_int(int(share)), ctypes.c_int(bam._tid[chrom]), ctypes.c_int32(int(shift))))
            self.n += n_reads
        return n_reads

    def add_soa(self, soa, seg, shift=0):
        """One more segment: segment ``seg`` of BAM-native arrays resident on the device (``Context.upload_soa``)."""
        _check(lib().spl_reads_add_soa(self.ctx._h, self._h, soa._h, ctypes.c_int(int(seg)), ctypes.c_int32(int(shift))))
        self.n += soa.n[seg]

    def finish(self):
        _check(lib().spl_reads_finish(self.ctx._h, self._h))
        return self

    def has_strand(self):
        """True when the (finished) set is fused and its device arrays include the reads' strand bytes: what
        ``junctions(STRAND_FROM_XS)`` needs (a decode after ``BamFile.set_aux_strand``, ``upload_soa(with_strand=True)``)."""
        out = ctypes.c_int(0)
        _check(lib().spl_reads_has_strand(self._h, ctypes.byref(out)))
        return bool(out.value)

    def has_mate_keys(self):
        """True when the (finished) set is fused and its device arrays include the reads' name keys: what ``mate_table`` and
        ``gene_counts(fragments=True)`` need (a decode with ``mate_keys``, ``upload_soa(with_keys=True)``)."""
        out = ctypes.c_int(0)
        _check(lib().spl_reads_has_mate_keys(self._h, ctypes.byref(out)))
        return bool(out.value)

    def mate_table(self, seg, n_reads=None):
        """The mate table of segment ``seg`` of this (finished, fused) set with name keys, made on the device (``spl_mate_table``) ->
        (mate uint32[reads of the segment]: the mate's index within the segment or 0xFFFFFFFF, counts: dict of pairable, paired,
        unpaired_mate_mapped).  ``seg`` counts the segments that have reads, in the order they were added.  ``n_reads``: the
        segment's reads (asked of nobody: the caller added it); None: counts only."""
        counts = np.zeros(3, np.int64)
        mate = None if n_reads is None else np.empty(max(int(n_reads), 1), np.uint32)
        _check(lib().spl_mate_table(self.ctx._h, self._h, ctypes.c_int(int(seg)), _ptr(mate), _ptr(counts)))
        return (None if mate is None else mate[:int(n_reads)]), dict(zip(MATE_COUNTS, counts.tolist()))

    def subsample(self, seed, threshold, with_index=False):
        """The read set of the reads of this (finished, fused) set with name keys that the subsampling rule keeps under ``seed`` and
        ``threshold`` (0 .. 2^32: 2^32 keeps every read), made on the device (``spl_reads_subsample``) -> ``(DeviceReads,
        kept_per_seg)``: a finished, fused set on arrays of its own -- this one is untouched, and either may be freed first -- and
        the reads kept per segment of this set that has reads (int64).  ``with_index``: a third value, the number within this set of
        every kept read (uint32)."""
        h = ctypes.c_void_p()
        n_seg = self.n_segments()          # (asked of the library: the entries it writes)
        kept = np.zeros(max(n_seg, 1), np.int64)
        index = np.empty(max(self.n, 1), np.uint32) if with_index else None
        seed, threshold = int(seed), int(threshold)
        if not (0 <= seed < 1 << 64 and 0 <= threshold < 1 << 64):
            raise ValueError("seed and threshold are unsigned 64-bit numbers")
        _check(lib().spl_reads_subsample(self.ctx._h, self._h, ctypes.c_uint64(seed), ctypes.c_uint64(threshold), ctypes.byref(h), _ptr(kept), _ptr(index)))
        kept = kept[:n_seg]
        total = int(kept.sum())
        out = DeviceReads(self.ctx, h, total)
        return (out, kept, index[:total]) if with_index else (out, kept)

    def duplicates(self, seg, n_reads=None):
        """The duplicate marks of segment ``seg`` of this (finished, fused) set with name keys, made on the device at the first call
        and kept with the set (``spl_reads_duplicates``; the rule is ``csrc/spl_dup_rule.h``) -> (dup bool[reads of the segment],
        counts: dict of ``DUP_COUNTS``, hist int64[257]: groups of size 1 .. 255 and 256+, then the fragments of the last bin's
        groups).  ``seg`` and ``n_reads`` as for ``mate_table``; ``n_reads`` None: no marks come down."""
        counts, hist = np.zeros(len(DUP_COUNTS), np.int64), np.zeros(DUP_HIST, np.int64)
        dup = None if n_reads is None else np.zeros(max(int(n_reads), 1), np.uint8)
        _check(lib().spl_reads_duplicates(self.ctx._h, self._h, ctypes.c_int(int(seg)), _ptr(dup), _ptr(counts), _ptr(hist)))
        return (None if dup is None else dup[:int(n_reads)].astype(bool)), dict(zip(DUP_COUNTS, counts.tolist())), hist

    def dedup(self, with_index=False):
        """The read set of the reads of this (finished, fused) set with name keys that are no duplicates, made on the device
        (``spl_reads_dedup``) -> what ``subsample`` returns: a finished, fused set on arrays of its own and the reads kept per
        segment; ``with_index``: the number within this set of every kept read too."""
        h = ctypes.c_void_p()
        n_seg = self.n_segments()
        kept = np.zeros(max(n_seg, 1), np.int64)
        index = np.empty(max(self.n, 1), np.uint32) if with_index else None
        _check(lib().spl_reads_dedup(self.ctx._h, self._h, ctypes.byref(h), _ptr(kept), _ptr(index)))
        kept = kept[:n_seg]
        total = int(kept.sum())
        out = DeviceReads(self.ctx, h, total)
        return (out, kept, index[:total]) if with_index else (out, kept)

    def n_segments(self):
        """The segments of this set that have reads, in the order they were added (``spl_reads_n_segments``): ``mate_table``'s numbers,
        ``subsample``'s ``kept_per_seg``."""
        out = ctypes.c_int64(0)
        _check(lib().spl_reads_n_segments(self._h, ctypes.byref(out)))
        return out.value

    def junctions_stats(self):
        """-> (bytes of the device table the last ``junctions`` call on this context allocated, device ms of its launches or -1)."""
        b, ms = ctypes.c_int64(0), ctypes.c_float(-1.0)
        _check(lib().spl_junctions_stats(self.ctx._h, ctypes.byref(b), ctypes.byref(ms)))
        return b.value, ms.value

    def layout_bytes(self):
        """-> (bytes of BAM-native arrays the layout kernel reads, bytes of records it writes) for this read set."""
        a, b = ctypes.c_int64(0), ctypes.c_int64(0)
        _check(lib().spl_reads_layout_bytes(self.ctx._h, self._h, ctypes.byref(a), ctypes.byref(b)))
        return a.value, b.value

    def slots(self):
        """The range kernel's slots of this (finished) set as the last layout left them (test hook: ``spl_reads_slots_download``) ->
        dict: ``fused``; ``order`` uint32[8, per], the chunk of every slot of every XCD share (0xffffffff: none); for a fused set
        also ``slots`` uint8[8, per, 64] and ``chunks`` uint8[n_chunks, 32], the descriptors as bytes (``spl_devpack.h``)."""
        n, ns, fused = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int(0)
        _check(lib().spl_reads_slots_download(self.ctx._h, self._h, ctypes.byref(n), ctypes.byref(ns), ctypes.byref(fused), None, None, None))
        n, ns, fused = n.value, ns.value, bool(fused.value)
        order = np.zeros(max(ns, 1), np.uint32)
        slots = np.zeros((max(ns, 1), 64), np.uint8) if fused else None
        chunks = np.zeros((max(n, 1), 32), np.uint8) if fused else None
        _check(lib().spl_reads_slots_download(self.ctx._h, self._h, None, None, None, _ptr(order), _ptr(slots), _ptr(chunks)))
        out = dict(fused=fused, order=order[:ns].reshape(8, ns // 8))
        if fused:
            out.update(slots=slots[:ns].reshape(8, ns // 8, 64), chunks=chunks[:n])
        return out

    def relayout(self):
        """The layout kernel once more, into the same records (segments that were laid out on the device)."""
        _check(lib().spl_reads_relayout(self.ctx._h, self._h))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.free()

    def literal_queue_size(self):
        out = ctypes.c_int64(0)
        _check(lib().spl_literal_queue_size(self.ctx._h, self._h, ctypes.byref(out)))
        return out.value

    def junctions(self, stranded=0, min_anchor=0, min_intron=0, max_intron=0, fragments=False):
        """Junction table of this read set, computed on the device (``spl_junctions``): dict of arrays left, right,
        strand (bytes '+', '-' or '?'), count, anchor_left, anchor_right, sorted by (left, right, strand).  ``stranded``: 0, 1
        (fr), 2 (rf) or ``STRAND_FROM_XS``: the reads' strand bytes, up to three rows a junction (``has_strand`` sets only).
        ``fragments``: a junction whose read has an earlier mate (``mate_table``) that supports the same row adds nothing
        (``spl_junctions_fragments``; a fused set with name keys)."""
        n = ctypes.c_int64(0)
        entry = lib().spl_junctions_fragments if fragments else lib().spl_junctions
        _check(entry(self.ctx._h, self._h, ctypes.c_int(int(stranded)), ctypes.c_int32(int(min_anchor)),
                                   ctypes.c_int32(int(min_intron)), ctypes.c_int32(int(max_intron)), ctypes.byref(n)))
        n = n.value
        out = dict(left=np.empty(n, np.int32), right=np.empty(n, np.int32), strand=np.empty(n, np.uint8),
                   count=np.empty(n, np.uint32), anchor_left=np.empty(n, np.uint32), anchor_right=np.empty(n, np.uint32))
        _check(lib().spl_junctions_get(self.ctx._h, _ptr(out["left"]), _ptr(out["right"]), _ptr(out["strand"]), _ptr(out["count"]),
                                       _ptr(out["anchor_left"]), _ptr(out["anchor_right"])))
        return out

    def motif_strand(self, genome, seq):
        """OVERWRITES the strand byte of every read of this (finished, fused, ``has_strand``) set by the splice motifs of sequence
        ``seq`` (an index or a name) of ``genome`` (``spl_reads_motif_strand``) -> int64[12], ``MOTIF_TALLY``'s counters."""
        out = np.zeros(12, np.int64)
        _check(lib().spl_reads_motif_strand(self.ctx._h, self._h, genome._h, ctypes.c_int(genome.index(seq)), _ptr(out)))
        return out

    def strand_tally(self, cover=None):
        """Read strand against evidence strand over this (finished, fused) set, on the device (``spl_strand_tally``): -> int64[14]
        -- reads seen, eligible reads, then per mate class (unpaired, first, second) the reads whose fr strand agrees / disagrees
        with their strand byte (``has_strand`` sets) and, from index 8, with the strand cover map.  ``cover``: ``(start, code)`` in the
        set's coordinates (``strandedness.cover_map``) or None."""
        start, code = _cover_arrays(cover)
        out = np.zeros(14, np.int64)
        _check(lib().spl_strand_tally(self.ctx._h, self._h, ctypes.c_int64(start.shape[0]), _ptr(start) if start.shape[0] else None,
                                      _ptr(code) if code.shape[0] else None, _ptr(out)))
        return out

    def coverage(self, length, stranded=0, strand=0, fragments=False):
        """Per-base read depth of this (finished, fused) set, taken as the reads of one reference of ``length`` bases, on the device
        (``spl_coverage``): -> (start int32, end int32, depth uint32, totals) -- the runs, 0-based and half-open, ascending, maximal,
        depth > 0 only; ``totals``: dict of runs, reads_seen, contributed, past_end, covered_bases.  ``stranded``: 0, 1 (fr) or 2
        (rf); ``strand``: 0 with ``stranded=0``, else ``'+'`` or ``'-'`` (a character or its code): the track.  ``fragments``: a pair
        of mates (``mate_table``) on the track covers the union of both reads' blocks once (``spl_coverage_fragments``; the set needs
        name keys); ``totals`` then has ``pairs`` too, the pairs whose union was taken."""
        strand = ord(strand) if isinstance(strand, (str, bytes)) else int(strand)
        h = ctypes.c_void_p()
        entry = lib().spl_coverage_fragments if fragments else lib().spl_coverage
        _check(entry(self.ctx._h, self._h, ctypes.c_int64(int(length)), ctypes.c_int(int(stranded)), ctypes.c_int(strand), ctypes.byref(h)))
        try:
            t = np.zeros(6 if fragments else 5, np.int64)
            _check((lib().spl_coverage_fragment_totals if fragments else lib().spl_coverage_totals)(h, _ptr(t)))
            n = int(t[0])
            start, end, depth = np.empty(n, np.int32), np.empty(n, np.int32), np.empty(n, np.uint32)
            _check(lib().spl_coverage_download(self.ctx._h, h, _ptr(start), _ptr(end), _ptr(depth)))
        finally:
            lib().spl_coverage_free(self.ctx._h, h)
        return start, end, depth, dict(zip(COVERAGE_FRAGMENT_TOTALS if fragments else COVERAGE_TOTALS, t.tolist()))

    def gene_counts(self, n_genes, map_a, map_b=None, stranded=0, out=None, fragments=False):
        """Per-gene read counts of this (finished, fused) set, on the device (``spl_gene_count``): ADDS to ``out`` (int64[n_genes + 3];
        made when None) and returns it -- the genes' reads, then no feature, ambiguous, not counted.  ``map_a`` / ``map_b``: gene maps
        ``(start int32, code uint32)`` in the set's coordinates (``genecounts.gene_maps``) or None; ``stranded``: 0 (``map_a`` serves
        every read), 1 (fr) or 2 (rf): ``map_a`` serves the ``+`` reads, ``map_b`` the ``-`` reads.  ``fragments``: a pair of mates
        (``mate_table``) counts once, by both mates' blocks (``spl_gene_count_fragments``; the set needs name keys)."""
        n_genes = int(n_genes)
        if out is None:
            out = np.zeros(max(n_genes, 0) + 3, np.int64)
        if not (isinstance(out, np.ndarray) and out.dtype == np.int64 and out.shape == (n_genes + 3,) and out.flags.c_contiguous):
            raise ValueError("gene counts are a contiguous int64 array of n_genes + 3 entries")
        (a_start, a_code), (b_start, b_code) = _gene_map_arrays(map_a), _gene_map_arrays(map_b)
        entry = lib().spl_gene_count_fragments if fragments else lib().spl_gene_count
        _check(entry(self.ctx._h, self._h, ctypes.c_int(int(stranded)), ctypes.c_int64(a_start.shape[0]), _ptr(a_start) if a_start.shape[0] else None,
                    _ptr(a_code) if a_code.shape[0] else None, ctypes.c_int64(b_start.shape[0]), _ptr(b_start) if b_start.shape[0] else None,
                    _ptr(b_code) if b_code.shape[0] else None, ctypes.c_int64(n_genes), _ptr(out)))
        return out

    def exon_counts(self, bin_gene, map_a, map_b=None, stranded=0, out=None, fragments=False):
        """Per-exon-bin read counts of this (finished, fused) set, on the device (``spl_exon_count``): ADDS to ``out``
        (int64[n_bins + 4]; made when None) and returns it -- the bins' reads, then the reads counted, without a feature, ambiguous,
        not counted.  ``bin_gene``: every bin's gene (uint32[n_bins]); ``map_a`` / ``map_b``: bin maps ``(start int32, code uint32)``
        in the set's coordinates (``exoncounts.exon_maps``) or None; ``stranded`` as for ``gene_counts``.  ``fragments``: a pair of
        mates (``mate_table``) adds one to every distinct bin of both reads (``spl_exon_count_fragments``; the set needs name keys)."""
        bin_gene = _arr(bin_gene, np.uint32)
        n_bins = int(bin_gene.shape[0])
        if out is None:
            out = np.zeros(n_bins + 4, np.int64)
        if not (isinstance(out, np.ndarray) and out.dtype == np.int64 and out.shape == (n_bins + 4,) and out.flags.c_contiguous):
            raise ValueError("exon counts are a contiguous int64 array of n_bins + 4 entries")
        (a_start, a_code), (b_start, b_code) = _gene_map_arrays(map_a), _gene_map_arrays(map_b)
        entry = lib().spl_exon_count_fragments if fragments else lib().spl_exon_count
        _check(entry(self.ctx._h, self._h, ctypes.c_int(int(stranded)), ctypes.c_int64(a_start.shape[0]), _ptr(a_start) if a_start.shape[0] else None,
                     _ptr(a_code) if a_code.shape[0] else None, ctypes.c_int64(b_start.shape[0]), _ptr(b_start) if b_start.shape[0] else None,
                     _ptr(b_code) if b_code.shape[0] else None, ctypes.c_int64(n_bins), _ptr(bin_gene) if n_bins else None, _ptr(out)))
        return out

    def intron_depth(self, length, piece_off, piece_start, piece_end, trim_percent=30, stranded=0, strand=0, fragments=False):
        """The trimmed depth of introns over this (finished, fused) set, taken as the reads of one reference of ``length`` bases, on
        the device (``spl_intron_depth``): -> int64[n_introns, 4] -- measurable bases L, covered bases, depth_n, depth_sum.  Intron i
        has the pieces ``piece_off[i] .. piece_off[i + 1]`` of ``(piece_start, piece_end)``, 0-based and half-open, disjoint and
        ascending within an intron; ``stranded`` / ``strand``: the track, as for ``coverage``.  ``fragments``: the depth is
        ``coverage(fragments=True)``'s (``spl_intron_depth_fragments``; the set needs name keys)."""
        strand = ord(strand) if isinstance(strand, (str, bytes)) else int(strand)
        off, start, end = _arr(piece_off, np.int64), _arr(piece_start, np.int32), _arr(piece_end, np.int32)
        n = max(int(off.shape[0]) - 1, 0)
        out = np.zeros((n, 4), np.int64)
        entry = lib().spl_intron_depth_fragments if fragments else lib().spl_intron_depth
        _check(entry(self.ctx._h, self._h, ctypes.c_int64(int(length)), ctypes.c_int(int(stranded)), ctypes.c_int(strand), ctypes.c_int64(n),
                     _ptr(off) if off.shape[0] else None, _ptr(start) if start.shape[0] else None, _ptr(end) if end.shape[0] else None,
                     ctypes.c_int(int(trim_percent)), _ptr(out) if n else None))
        return out

    def free(self):
        if self._h:
            lib().spl_reads_free(self.ctx._h, self._h)
            self._h = ctypes.c_void_p()


class DeviceSoA(object):
    """BAM-native reads (pos, flag, cig_off, cigar) resident in HBM; ``n`` = reads per segment."""
    def __init__(self, ctx, h, n):
        self.ctx, self._h, self.n = ctx, h, list(n)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.free()

    def free(self):
        if self._h:
            lib().spl_soa_free(self.ctx._h, self._h)
            self._h = ctypes.c_void_p()


def algorithmic_bytes(dsites, dreads):
    out = ctypes.c_int64(0)
    _check(lib().spl_count_algorithmic_bytes(dsites._h, dreads._h, ctypes.byref(out)))
    return out.value


def gene_search(g_left, g_right, g_strand, q_pos, q_strand, is_stranded):
    """binary_gene_search for a batch (``spl_gene_search``): -> int32 gene index per query, -1 = none."""
    g_left = np.ascontiguousarray(g_left, np.int64)
    g_right = np.ascontiguousarray(g_right, np.int64)
    g_strand = np.ascontiguousarray(g_strand, np.uint8)
    q_pos = np.ascontiguousarray(q_pos, np.int64)
    q_strand = np.ascontiguousarray(q_strand, np.uint8)
    out = np.empty(q_pos.shape[0], np.int32)
    _check(lib().spl_gene_search(_ptr(g_left), _ptr(g_right), _ptr(g_strand), ctypes.c_int64(g_left.shape[0]), _ptr(q_pos),
                                 _ptr(q_strand), ctypes.c_int64(q_pos.shape[0]), ctypes.c_int(1 if is_stranded else 0), _ptr(out)))
    return out


def _blob(texts):
    """list of str -> (bytes, uint32 offsets[n + 1])."""
    enc = [t.encode("utf-8") for t in texts]
    off = np.zeros(len(enc) + 1, np.uint32)
    if enc:
        np.cumsum(np.fromiter((len(e) for e in enc), dtype=np.int64, count=len(enc)), out=off[1:])
    return b"".join(enc), off


def tsv_prepare(arr):
    """What ``spl_tsv_append`` wants of a chromosome's rows that no count changes -- the strand and gene texts as blobs, the
    table's columns as the integers it reads -- made once and kept on ``arr``: ``process`` has this done while the alignment
    file is still being decoded, so that only the formatting itself is left when the counts arrive."""
    st = getattr(arr, "_tsv_static", None)
    if st is not None:
        return st
    if getattr(arr, "_strand_text", 0) is None:      # (a table built from arrays: the texts follow from the arrays, no list of str)
        codes = np.ascontiguousarray(arr.strand, np.uint8)
        there = codes != 0
        strand_blob = codes[there].tobytes()
        strand_off = np.zeros(arr.n + 1, np.uint32)
        np.cumsum(there, out=strand_off[1:])
    else:
        strand_blob, strand_off = _blob(arr.strand_text)
    if getattr(arr, "_genes", 0) is None and arr.gene_idx is not None:
        names_blob, names_off = _blob(list(arr.gene_names) + ["NA"])
        gi = np.where(arr.gene_idx >= 0, arr.gene_idx, len(arr.gene_names)).astype(np.int64)
        first = names_off[:-1].astype(np.int64)[gi]
        length = np.diff(names_off.astype(np.int64))[gi]
        gene_off = np.zeros(arr.n + 1, np.uint32)
        np.cumsum(length, out=gene_off[1:])
        take = np.repeat(first - gene_off[:-1].astype(np.int64), length) + np.arange(int(gene_off[-1]), dtype=np.int64)
        gene_blob = np.frombuffer(names_blob, np.uint8)[take].tobytes() if arr.n else b""
    else:
        gene_blob, gene_off = _blob(arr.genes)
    c64 = lambda a: np.ascontiguousarray(a, np.int64)   # noqa: E731
    st = dict(strand_blob=strand_blob, strand_off=strand_off, gene_blob=gene_blob, gene_off=gene_off, pos=c64(arr.pos), alpha=c64(arr.alpha),
              part_off=np.ascontiguousarray(arr.part_off, np.uint32), comp_off=np.ascontiguousarray(arr.comp_off, np.uint32),
              part_pos=c64(arr.part_pos), edge_cnt=c64(arr.edge_cnt), comp_pos=c64(arr.comp_pos), chrom=arr.chrom.encode("utf-8"))
    arr._tsv_static = st
    return st


class spl_tsv_rows(ctypes.Structure):
    _fields_ = [("chrom", ctypes.c_char_p), ("n_sites", ctypes.c_int64), ("pos", ctypes.c_void_p), ("strand_blob", ctypes.c_char_p),
                ("strand_off", ctypes.c_void_p), ("gene_blob", ctypes.c_char_p), ("gene_off", ctypes.c_void_p), ("sse", ctypes.c_void_p),
                ("alpha", ctypes.c_void_p), ("beta1", ctypes.c_void_p), ("beta2_simple", ctypes.c_void_p), ("beta2_cryptic", ctypes.c_void_p),
                ("beta2_weighted", ctypes.c_void_p), ("part_off", ctypes.c_void_p), ("part_pos", ctypes.c_void_p), ("edge_cnt", ctypes.c_void_p),
                ("comp_off", ctypes.c_void_p), ("comp_pos", ctypes.c_void_p)]


def tsv_append_many(path, items, cryptic):
    """Rows of several chromosomes, [(ChromArrays, results)], appended to ``path`` in that order by ``spl_tsv_append_many`` (same
    bytes as tsv.format_chrom for each)."""
    n = len(items)
    if n == 0:
        return
    rows = (spl_tsv_rows * n)()
    keep = []
    addr = lambda a: None if a is None else a.ctypes.data   # noqa: E731
    c64 = lambda a: np.ascontiguousarray(a, np.int64)       # noqa: E731
    for k, (arr, res) in enumerate(items):
        st = tsv_prepare(arr)
        beta1 = np.ascontiguousarray(res["beta1"], np.uint32)
        b2s = c64(res["beta2_simple"])
        sse = np.ascontiguousarray(res["sse"], np.float64)
        b2c = c64(res["beta2_cryptic"]) if cryptic else None
        b2w = np.ascontiguousarray(res["beta2_weighted"], np.float64) if cryptic else None
        keep.append((st, beta1, b2s, sse, b2c, b2w))
        r = rows[k]
        r.chrom, r.n_sites = st["chrom"], arr.n
        r.pos, r.strand_blob, r.strand_off = addr(st["pos"]), st["strand_blob"], addr(st["strand_off"])
        r.gene_blob, r.gene_off = st["gene_blob"], addr(st["gene_off"])
        r.sse, r.alpha, r.beta1, r.beta2_simple = addr(sse), addr(st["alpha"]), addr(beta1), addr(b2s)
        r.beta2_cryptic, r.beta2_weighted = addr(b2c), addr(b2w)
        r.part_off, r.part_pos, r.edge_cnt = addr(st["part_off"]), addr(st["part_pos"]), addr(st["edge_cnt"])
        r.comp_off, r.comp_pos = addr(st["comp_off"]), addr(st["comp_pos"])
    _check(lib().spl_tsv_append_many(os.fsencode(path), ctypes.c_int32(n), rows, ctypes.c_int(1 if cryptic else 0)))
    del keep


def tsv_append(path, arr, res, cryptic):
    """Rows of one chromosome appended to ``path`` (``spl_tsv_append_many`` with one; same bytes as tsv.format_chrom)."""
    tsv_append_many(path, [(arr, res)], cryptic)


def write_bam(path, ref_names, ref_lengths, read_sets, level=1, threads=0, seq_mode=0):
    """Fast native BAM writer for synthetic workloads: read_sets[i] = samio.ReadSet of reference i.  ``seq_mode`` 0: constant
    SEQ / QUAL bytes (deflates to a few bytes per record); 1: pseudo-random bases, binned qualities (deflates ~4x)."""
    n = len(ref_names)
    names = (ctypes.c_char_p * n)(*[s.encode("ascii") for s in ref_names])
    lens = (ctypes.c_int64 * n)(*[int(v) for v in ref_lengths])
    arr = (spl_reads * n)()
    keep = []
    for i, rs in enumerate(read_sets):
        ra = ReadArrays(rs.pos, rs.flag, rs.cig_off, rs.cigar)
        keep.append(ra)
        arr[i] = ra.c
    _check(lib().spl_bam_write2(os.fsencode(path), ctypes.c_int(n), names, lens, arr, ctypes.c_int(level), ctypes.c_int(threads),
                                ctypes.c_int(seq_mode)))


def trim(device=-1):
    """Device memory the library keeps for its next call goes back to the driver (``spl_trim``)."""
    _check(lib().spl_trim(ctypes.c_int(device)))


DEVMEM_STATS = ("handed_out", "from_pool", "poisoned", "held_bytes")


def devmem_stats():
    """The device memory pool since the process began (``spl_devmem_stats``, a test hook) -> dict of handed_out, from_pool, poisoned
    (buffers) and held_bytes (what the pool holds now)."""
    out = np.zeros(4, np.int64)
    _check(lib().spl_devmem_stats(_ptr(out)))
    return dict(zip(DEVMEM_STATS, out.tolist()))


def devmem_probe(ctx, n_bytes, tag="x", room=None):
    """A buffer of ``n_bytes`` taken from the pool under ``tag`` as the library takes its own, and given back
    (``spl_devmem_probe``, a test hook) -> (its bytes as it was handed over: uint8[min(capacity, room)], its capacity)."""
    room = int(n_bytes) + (4 << 20) if room is None else int(room)
    host = np.zeros(max(room, 1), np.uint8)
    cap = ctypes.c_int64(0)
    _check(lib().spl_devmem_probe(ctx._h, ctypes.c_int64(int(n_bytes)), ctypes.c_int(ord(tag)), _ptr(host), ctypes.c_int64(room), ctypes.byref(cap)))
    return host[:min(cap.value, room)], cap.value


def prof_enable(on=True):
    """The library's own stopwatch over all its kernels, process-wide (``spl_prof_enable``): clears what was recorded."""
    _check(lib().spl_prof_enable(ctypes.c_int(1 if on else 0)))


def prof_report():
    """-> [{"kernel", "calls", "ms", "bytes"}, ...] of the launches since ``prof_enable`` (waits for the devices)."""
    import json
    need = lib().spl_prof_report(None, ctypes.c_int(0))
    buf = ctypes.create_string_buffer(need + 16)
    lib().spl_prof_report(buf, ctypes.c_int(need + 16))
    return json.loads(buf.value.decode("ascii"))


class BamFile(object):
    """BAM decode on host threads (``spl_bam_*``); replaces ``samtools view`` per site.

    ``stream=True``: the constructor returns once the header is read and the decode goes on in the background; ``wait_ref``
    blocks until one reference is complete, ``DeviceReads.add_bam`` sends its reads to the GPU from the decoder's own buffers,
    ``wait_all`` ends the decode and tells whether the file was sorted by reference (if not, references taken early were
    incomplete).

    ``min_mapq``, ``require_flags``, ``exclude_flags``: samtools view's -q / -f / -F (``spl_bam_set_filter``); a record that fails
    them is never extracted, whoever decodes the file.  ``filter_counts`` says how many did.

    ``flagstat``: whoever decodes the file also counts samtools flagstat's categories over all its records
    (``spl_bam_set_flagstat``); ``flagstat()`` has them.

    ``any_order``: the file's records may come in any order, e.g. as the aligner wrote them -- whoever decodes the file hands
    every reference's reads out sorted by (POS, place in the file) (``spl_bam_set_any_order``), ``wait_all`` says True and
    ``wait_ref`` returns at the end of the decode; ``any_order_sorted()`` says what that took."""

    def __init__(self, path, threads=0, stream=False, defer=False, min_mapq=0, require_flags=0, exclude_flags=0, aux_strand=False, flagstat=False,
                 any_order=False, mate_keys=False):
        self._h = ctypes.c_void_p()
        self.filter, self.aux_strand, self.counts_flagstat, self.any_order, self.mate_keys = (0, 0, 0), False, False, False, False
        # what was asked for must be there before the decode starts: such a file is opened deferred, set up and started below
        options = [(self.set_filter, (int(min_mapq), int(require_flags), int(exclude_flags)), (0, 0, 0)),
                   (self.set_aux_strand, (bool(aux_strand),), (False,)),
                   (self.set_flagstat, (bool(flagstat),), (False,)),
                   (self.set_any_order, (bool(any_order),), (False,)),
                   (self.set_mate_keys, (bool(mate_keys),), (False,))]
        asked = [(setter, args) for setter, args, default in options if args != default]
        opener = self._opener(defer or bool(asked), stream)
        _check(opener(os.fsencode(path), ctypes.c_int(threads), ctypes.byref(self._h)))
        if asked:
            try:
                for setter, args in asked:
                    setter(*args)
                if not defer:
                    _check(lib().spl_bam_start(self._h))
                    if not stream:
                        _check(lib().spl_bam_wait_all(self._h, None))
            except Exception:
                lib().spl_bam_close(self._h)
                self._h = ctypes.c_void_p()
                raise
        self.on_device = None    # (defer=True: set by decode_on_device)
        self.ref_names = [lib().spl_bam_ref_name(self._h, i).decode("ascii") for i in range(lib().spl_bam_n_ref(self._h))]
        self.ref_lengths = [lib().spl_bam_ref_length(self._h, i) for i in range(len(self.ref_names))]
        self._tid = {n: i for i, n in enumerate(self.ref_names)}
        self._views = {}

    @staticmethod
    def _opener(deferred, stream):
        return lib().spl_bam_open_deferred if deferred else (lib().spl_bam_open_stream if stream else lib().spl_bam_open)

    def set_filter(self, min_mapq=0, require_flags=0, exclude_flags=0):
        """The read filter of a ``defer=True`` file nobody decodes yet (``spl_bam_set_filter``; an error afterwards)."""
        _check(lib().spl_bam_set_filter(self._h, ctypes.c_int(int(min_mapq)), ctypes.c_int(int(require_flags)), ctypes.c_int(int(exclude_flags))))
        self.filter = (int(min_mapq), int(require_flags), int(exclude_flags))

    def set_aux_strand(self, on=True):
        """A ``defer=True`` file nobody decodes yet: the decode -- whoever does it -- also leaves a strand byte per placed read, the
        aligner's XS:A tag of the spliced ones (``spl_bam_set_aux_strand``; an error afterwards).  ``reads(chrom).xs`` has them,
        a read set of the device decode ``has_strand()``."""
        _check(lib().spl_bam_set_aux_strand(self._h, ctypes.c_int(1 if on else 0)))
        self.aux_strand = bool(on)

    def set_mate_keys(self, on=True):
        """A ``defer=True`` file nobody decodes yet: the decode -- whoever does it -- also leaves a name key per placed read
        (``spl_bam_set_mate_keys``; an error afterwards): which two records are mates.  ``reads(chrom).name_key`` has them, a read
        set of the device decode ``has_mate_keys()``."""
        _check(lib().spl_bam_set_mate_keys(self._h, ctypes.c_int(1 if on else 0)))
        self.mate_keys = bool(on)

    def set_flagstat(self, on=True):
        """A ``defer=True`` file nobody decodes yet: the decode -- whoever does it -- also counts the flagstat categories
        (``spl_bam_set_flagstat``; an error afterwards)."""
        _check(lib().spl_bam_set_flagstat(self._h, ctypes.c_int(1 if on else 0)))
        self.counts_flagstat = bool(on)

    def set_any_order(self, on=True):
        """A ``defer=True`` file nobody decodes yet: its records may come in any order, and the decode -- whoever does it -- hands
        every reference's reads out sorted by (POS, place in the file) (``spl_bam_set_any_order``; an error afterwards)."""
        _check(lib().spl_bam_set_any_order(self._h, ctypes.c_int(1 if on else 0)))
        self.any_order = bool(on)

    def any_order_sorted(self):
        """-> (reads that were put in order -- 0 when the file was in order already --, True when the GPU's sort did it and False
        when the host threads did); waits for the end of the decode (``spl_bam_any_order_sorted``)."""
        n, dev = ctypes.c_int64(0), ctypes.c_int(0)
        _check(lib().spl_bam_any_order_sorted(self._h, ctypes.byref(n), ctypes.byref(dev)))
        return int(n.value), bool(dev.value)

    def flagstat(self):
        """-> int64 array (16, 2): per category of samtools flagstat (``FLAGSTAT_LABELS``) the QC-passed and the QC-failed records
        of the file -- of those the read filter keeps, when one is set; waits for the end of the decode.  An error for a file
        opened without ``flagstat=True``."""
        out = (ctypes.c_int64 * 32)()
        _check(lib().spl_bam_flagstat(self._h, out))
        return np.array(out[:], np.int64).reshape(16, 2)

    def filter_counts(self):
        """-> (records dropped by their flags, records dropped by their MAPQ alone); waits for the end of the decode."""
        out = (ctypes.c_int64 * 2)()
        _check(lib().spl_bam_filter_counts(self._h, out))
        return int(out[0]), int(out[1])

    def start_host_decode(self):
        """A file opened with ``defer=True``: decode on the host's threads, from now on in the background."""
        _check(lib().spl_bam_start(self._h))
        self.on_device = False

    def compression_ratio(self):
        """Inflated bytes per file byte over the first record blocks (0.0 = cannot tell); ``defer=True`` files only."""
        r = ctypes.c_double(0.0)
        _check(lib().spl_bam_compression_ratio(self._h, ctypes.byref(r)))
        return r.value

    def decode_on_device_async(self, device=0):
        """``decode_on_device`` on a thread and a context of its own, started now: the caller goes on (Steps 0-2), anybody who
        waits for a reference meanwhile waits for this decode.  -> the thread (join it before closing the file)."""
        import threading
        _check(lib().spl_bam_reserve_device(self._h))
        self.on_device = False

        def run():
            try:
                with Context(device) as ctx:
                    self.decode_on_device(ctx)
            except BaseException as exc:   # (the C side never leaves the file without a decoder; keep the reason)
                self.device_error = exc
                try:                       # (... and if it never got as far as the C side -- no context -- the reservation must
                    lib().spl_bam_start(self._h)   #  not outlive this thread: the host threads take the file)
                except Exception:
                    pass
        t = threading.Thread(target=run)
        t.start()
        self._device_thread = t
        return t

    def decode_on_devices_async(self, devices):
        """The decode in SHARES, one per entry of ``devices`` (a device may appear more than once: a context each): the file is
        cut into stretches of EQUAL size in file bytes, at any BGZF block (``spl_bam_share_plan``), and every device inflates and
        extracts its own stretch over its own PCIe link.  A reference may lie in several shares: each device counts its stretch
        against the reference's whole site table and the partial counters are added (``process.process_sites``).  -> [(device,
        [names of the references the share can hold records of])], the plan (``shares``; ``share_bytes``: the file bytes of each;
        ``share_ref`` says what a share really holds once the decoders are done).  Threads in ``_device_threads``."""
        import threading
        n = ctypes.c_int(0)
        _check(lib().spl_bam_share_plan(self._h, ctypes.c_int(len(devices)), ctypes.byref(n)))
        _check(lib().spl_bam_reserve_device(self._h))
        self.on_device = False
        plan, sizes = [], []
        for k in range(n.value):
            lo, hi = ctypes.c_int(0), ctypes.c_int(0)
            _check(lib().spl_bam_share_range(self._h, ctypes.c_int(k), ctypes.byref(lo), ctypes.byref(hi)))
            plan.append((devices[k], [self.ref_names[t] for t in range(lo.value, min(hi.value, len(self.ref_names)))]))
            sizes.append(self.share_info(k)["file_bytes"])
        self.shares = plan
        self.share_bytes = sizes
        self._share_errors = []

        def run(k, device):
            flag = ctypes.c_int(0)
            try:
                with Context(device) as ctx:
                    _check(lib().spl_bam_decode_device_share(ctx._h, self._h, ctypes.c_int(k), ctypes.byref(flag)))
            except BaseException as exc:   # (no context, or the call itself failed: the share must still be reported, or the
                self._share_errors.append(exc)   # file waits for ever -- the host threads take all of it then)
                try:
                    lib().spl_bam_start(self._h)
                except Exception:
                    pass
        self._device_threads = [threading.Thread(target=run, args=(k, dev)) for k, (dev, _) in enumerate(plan)]
        for t in self._device_threads:
            t.start()
        self._device_thread = self._device_threads[0]
        return plan

    def sample(self):
        """-> (records, CIGAR ops, inflated bytes) of what the host sampled at three places of the file (``spl_bam_sample``)."""
        out = (ctypes.c_int64 * 3)()
        _check(lib().spl_bam_sample(self._h, out))
        return int(out[0]), int(out[1]), int(out[2])

    def share_info(self, k):
        """-> {file_bytes, u_lo, u_hi, tail_blocks} of share ``k`` of the plan (``spl_bam_share_info``)."""
        v = [ctypes.c_int64(0) for _ in range(4)]
        _check(lib().spl_bam_share_info(self._h, ctypes.c_int(int(k)), *[ctypes.byref(x) for x in v]))
        return dict(file_bytes=v[0].value, u_lo=v[1].value, u_hi=v[2].value, tail_blocks=v[3].value)

    def share_ref(self, k, chrom):
        """-> (reads, largest end coordinate) of what share ``k`` holds of reference ``chrom`` (after ``join_decoders`` said True)."""
        n, me = ctypes.c_int64(0), ctypes.c_int64(0)
        _check(lib().spl_bam_share_ref(self._h, ctypes.c_int(int(k)), ctypes.c_int(self._tid[chrom]), ctypes.byref(n), ctypes.byref(me)))
        return n.value, me.value

    def share_count_host(self, k):
        """-> records of share ``k`` per reference by the host's inflate and a plain walk (the last entry: records without a
        reference); raises when the walk from the share's first record does not arrive at the next share's.  No GPU."""
        out = (ctypes.c_int64 * (len(self.ref_names) + 1))()
        _check(lib().spl_bam_share_count_host(self._h, ctypes.c_int(int(k)), out))
        return list(out)

    def decline_reason(self):
        """Why the device decoder left the file to the host threads ('' if it did not)."""
        return lib().spl_bam_decline_reason(self._h).decode("utf-8", "replace")

    def device_decode_started(self):
        """Somebody has started a decode on the device(s) (``decode_on_device_async`` / ``decode_on_devices_async``): its outcome
        is what ``join_decoders`` waits for."""
        return getattr(self, "_device_thread", None) is not None or bool(getattr(self, "_device_threads", None))

    def join_decoders(self):
        """Waits for the OUTCOME of the device decoders started by ``decode_on_device_async`` / ``decode_on_devices_async``; ->
        True when the reads are on the device(s) and every reference is complete, False when the host threads have the file (they
        may still be decoding it).  The decoders' threads themselves are joined by ``close``: what they give back on their way
        out (buffers, streams, events, their context: 10-13 ms for a large file) nobody has to wait for."""
        threads = getattr(self, "_device_threads", None) or ([self._device_thread] if getattr(self, "_device_thread", None) is not None else [])
        if not threads:
            return bool(getattr(self, "on_device", False))
        flag = ctypes.c_int(0)
        _check(lib().spl_bam_wait_device(self._h, ctypes.byref(flag)))
        self.on_device = bool(flag.value)
        return self.on_device

    def decode_on_device(self, ctx):
        """A file opened with ``defer=True``: inflate it and extract its records on the GPU of ``ctx`` (every reference is
        complete on return).  -> True; False when the file is not one for the device path (unsorted, CG-tag CIGARs, malformed)
        and the host threads have been started on it instead.  Without this call the first wait starts the host decode."""
        flag = ctypes.c_int(0)
        _check(lib().spl_bam_decode_device(ctx._h, self._h, ctypes.byref(flag)))
        self.on_device = bool(flag.value)
        return self.on_device

    @property
    def n_records(self):
        return lib().spl_bam_n_records(self._h)     # (waits for the end of the decode)

    def wait_ref(self, chrom):
        """-> (reads on that reference, largest end coordinate) once the reference is complete."""
        n, me = ctypes.c_int64(0), ctypes.c_int64(0)
        _check(lib().spl_bam_wait_ref(self._h, ctypes.c_int(self._tid[chrom]), ctypes.byref(n), ctypes.byref(me)))
        return n.value, me.value

    def wait_all(self):
        """Waits for the end of the decode (raises its error, if any).  -> True when the file was sorted by reference."""
        ok = ctypes.c_int(0)
        _check(lib().spl_bam_wait_all(self._h, ctypes.byref(ok)))
        return bool(ok.value)

    def reads(self, chrom):
        """-> samio.ReadSet-compatible views of the BAM-native arrays (borrowed from the native object, which every view
        keeps alive) or None when the file has no such reference (the reference's samtools call would print an error and
        yield nothing).  Waits for the whole file."""
        from .samio import ReadSet
        tid = self._tid.get(chrom)
        if tid is None:
            return None
        if chrom in self._views:
            return self._views[chrom]
        r = spl_reads()
        me = ctypes.c_int64(0)
        _check(lib().spl_bam_reads(self._h, ctypes.c_int(tid), ctypes.byref(r), ctypes.byref(me)))
        n = r.n_reads
        if n == 0:
            return ReadSet.empty()
        owner = _BamHandle(self)

        def view(ptr, count, dt):
            buf = (ctypes.c_char * (count * np.dtype(dt).itemsize)).from_address(ptr)
            buf._owner = owner      # the array's base object keeps the native decoder alive
            return np.frombuffer(buf, dtype=dt, count=count)
        cig_off = view(r.cig_off, n + 1, np.uint32)
        n_cig = int(cig_off[-1])
        rs = ReadSet.__new__(ReadSet)
        rs.pos = view(r.pos, n, np.int32)
        rs.flag = view(r.flag, n, np.uint16)
        rs.cig_off = cig_off
        rs.cigar = view(r.cigar, n_cig, np.uint32) if n_cig else np.zeros(0, np.uint32)
        rs.max_end = me.value
        rs.xs = None
        if self.aux_strand:
            xp = ctypes.c_void_p()
            _check(lib().spl_bam_aux_strand(self._h, ctypes.c_int(tid), ctypes.byref(xp)))
            rs.xs = view(xp.value, n, np.uint8) if xp.value else None
        rs.name_key = None
        if self.mate_keys:
            kp = ctypes.c_void_p()
            _check(lib().spl_bam_mate_keys(self._h, ctypes.c_int(tid), ctypes.byref(kp)))
            rs.name_key = view(kp.value, n, np.uint64) if kp.value else None
        self._views[chrom] = rs
        return rs

    def close(self):
        """Closes the native decoder -- unless views of its arrays are still alive: then their owner closes it.  A decode that is
        still running is told to stop first (``spl_bam_cancel``): nobody who closes the file wants the rest of it."""
        if self._h:
            lib().spl_bam_cancel.restype = None
            lib().spl_bam_cancel(self._h)
        for t in (getattr(self, "_device_threads", None) or []) + ([self._device_thread] if getattr(self, "_device_thread", None) is not None else []):
            t.join()                 # (the device decoders work on the native object: not under their feet)
        self._device_thread = None
        self._device_threads = None
        h, self._h = self._h, ctypes.c_void_p()
        views, self._views = self._views, {}
        if h and not views:
            lib().spl_bam_close(h)
        elif h:
            _BamHandle.release(h, views)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class SamFile(BamFile):
    """SAM text as the aligner wrote it, behind the same native object (``spl_sam_open``): every method of ``BamFile`` applies,
    except the ones about BGZF blocks (``compression_ratio``, ``sample``, a decode in shares: errors).  The file is opened
    deferred whatever ``stream`` / ``defer`` say: ``decode_on_device`` parses it on the GPU, and without that call the first
    wait parses it on a host thread -- by the same strict rule (csrc/spl_sam_line.h), always as ``any_order``.  A file with a
    line the rule does not take is DECLINED: waiting for it raises (code -5) and ``decline_reason()`` says ``line N <why>``;
    ``samio.read_sam`` reads such a file as before (``process.open_and_decode`` does that).  The text may be compressed, as BGZF
    (``bgzip``, ``samtools view -O sam,level=6``) or as plain gzip (``gzip``, several members too): ``compression`` says which."""

    def __init__(self, path, threads=0, stream=False, defer=True, min_mapq=0, require_flags=0, exclude_flags=0, aux_strand=False, flagstat=False,
                 any_order=True, mate_keys=False):
        BamFile.__init__(self, path, threads=threads, stream=True, defer=True, min_mapq=min_mapq, require_flags=require_flags, exclude_flags=exclude_flags,
                         aux_strand=aux_strand, flagstat=flagstat, mate_keys=mate_keys)
        self.any_order = True     # (the native side's default for text, whatever was passed)

    @staticmethod
    def _opener(deferred, stream):
        return lib().spl_sam_open

    COMPRESSION = ("", "BGZF", "gzip")

    @property
    def compression(self):
        """'' for plain text, 'BGZF' or 'gzip' for compressed text (``spl_bam_text_compression``): BGZF is inflated on the GPU, block
        by block, plain gzip by one host thread -- parsed on the GPU either way (``decode_on_device``)."""
        return self.COMPRESSION[lib().spl_bam_text_compression(self._h)]

    @property
    def blocks_inflated(self):
        """The BGZF blocks a device decode of this file inflated (0: none did, or the file is not BGZF)."""
        return int(lib().spl_bam_text_blocks(self._h))

    def declined(self):
        """Waits for the end of the decode; -> '' when the rule took every line, else ``line N <why>``.  Other failures raise."""
        try:
            self.wait_all()
        except SpliserNativeError as exc:
            if exc.code != -5 or not self.decline_reason().startswith("line "):
                raise
            return self.decline_reason()
        return ""


class _BamHandle(object):
    """Shared ownership of a native decoder between a BamFile and the numpy views handed out from it."""
    _parked = {}

    def __init__(self, bam):
        self._bam = bam          # a view keeps its BamFile (and so the native object) alive

    @classmethod
    def release(cls, handle, views):
        # BamFile.close() with live views: the native object is closed when the last view is gone
        import weakref
        key = handle.value
        cls._parked[key] = handle
        # (every array of every read set, not one of them: a caller that keeps the flags, the strand bytes or the name keys and
        # lets POS go still reads the native object's memory)
        live = [a for rs in views.values() for a in (rs.pos, rs.flag, rs.cig_off, rs.cigar, getattr(rs, "xs", None), getattr(rs, "name_key", None))
                if a is not None]
        left = [len(live)]

        def gone(_):
            left[0] -= 1
            if left[0] == 0:
                lib().spl_bam_close(cls._parked.pop(key))
        for a in live:
            weakref.finalize(a, gone, None)


FLAGSTAT_LABELS = ("in total (QC-passed reads + QC-failed reads)", "primary", "secondary", "supplementary", "duplicates", "primary duplicates", "mapped",
                   "primary mapped", "paired in sequencing", "read1", "read2", "properly paired", "with itself and mate mapped", "singletons",
                   "with mate mapped to a different chr", "with mate mapped to a different chr (mapQ>=5)")


def sort_keys_device(ctx, keys, key_bits):
    """The device's stable radix sort on ``keys`` (uint64) -- exactly the passes the decode of an ``any_order`` file runs for keys of
    ``key_bits`` bits (``spl_sort_keys_device``) -> the permutation, uint32: entry i = index of the key that comes i-th, equal keys
    in the order they came in."""
    keys = np.ascontiguousarray(keys, np.uint64)
    perm = np.zeros(len(keys), np.uint32)
    _check(lib().spl_sort_keys_device(ctx._h, _ptr(keys) if len(keys) else None, ctypes.c_int64(len(keys)), ctypes.c_int(int(key_bits)), _ptr(perm) if len(keys) else None))
    return perm


TEXT_WINDOWS_STOP, TEXT_WINDOWS_OWN = 0, 1     # what becomes of a line that fits no window: SAM text's rule, FASTA's


def text_windows_host(text, begin, win_bytes, rule):
    """How the device's text sources cut bytes [begin, len(text)) into windows of whole lines (``spl_text_windows_host``, no GPU)
    -> ([(lo, hi)], whether a line that fits no window ended the plan)."""
    buf = np.frombuffer(bytes(text), np.uint8)
    n, long_line = ctypes.c_int64(0), ctypes.c_int(0)
    cuts = np.zeros(2 * (buf.size + 1), np.int64)          # (a window holds a byte at least)
    _check(lib().spl_text_windows_host(_ptr(buf) if buf.size else None, ctypes.c_int64(buf.size), ctypes.c_int64(int(begin)), ctypes.c_int64(int(win_bytes)), ctypes.c_int(int(rule)),
                                       ctypes.c_int64(buf.size + 1), _ptr(cuts), ctypes.byref(n), ctypes.byref(long_line)))
    return [(int(cuts[2 * k]), int(cuts[2 * k + 1])) for k in range(n.value)], bool(long_line.value)


def text_line_index(ctx, text, windows):
    """The line starts of ``windows`` [(lo, hi)] of ``text`` by ONE of the decoders' line-index objects, in that order
    (``spl_text_line_index``) -> per window (line starts as offsets from lo & ~15, uint32; the lines the index then had room for)."""
    buf = np.frombuffer(bytes(text), np.uint8)
    lo, hi = _arr([w[0] for w in windows], np.int64), _arr([w[1] for w in windows], np.int64)
    cap = max(int(sum(h - l for l, h in windows)), 0)              # (a line holds a byte at least, except a window's last)
    n_lines, room, starts = np.zeros(max(len(windows), 1), np.int64), np.zeros(max(len(windows), 1), np.int64), np.zeros(cap + len(windows) + 1, np.uint32)
    _check(lib().spl_text_line_index(ctx._h, _ptr(buf) if buf.size else None, ctypes.c_int64(buf.size), ctypes.c_int64(len(windows)), _ptr(lo), _ptr(hi),
                                     ctypes.c_int64(starts.size), _ptr(n_lines), _ptr(room), _ptr(starts)))
    ends = np.cumsum(n_lines[:len(windows)])
    return [(starts[int(e - n):int(e)].copy(), int(r)) for e, n, r in zip(ends, n_lines, room)]


def flagstat_add_host(flag, tid, next_tid, mapq, counters=None):
    """The decoders' counting of one record on the host (``spl_flagstat_add_host``): adds to ``counters`` (int64, (16, 2); made when
    None) and returns them."""
    if counters is None:
        counters = np.zeros((16, 2), np.int64)
    assert counters.dtype == np.int64 and counters.shape == (16, 2) and counters.flags.c_contiguous
    _check(lib().spl_flagstat_add_host(ctypes.c_uint32(int(flag)), ctypes.c_int32(int(tid)), ctypes.c_int32(int(next_tid)), ctypes.c_uint32(int(mapq)), _ptr(counters)))
    return counters


MOTIF_TALLY = ("walks_none", "walks_GT_AG", "walks_CT_AC", "walks_GC_AG", "walks_CT_GC", "walks_AT_AC", "walks_GT_AT",
               "reads_plus", "reads_minus", "reads_conflicting", "reads_no_canonical", "reads_outside")


class Genome(object):
    """A FASTA's sequences as base codes in device memory (``spl_genome_open``): ``names``, ``lengths``; ``window_bytes``: 0 = the
    default windows.  ``free()`` while nothing uses it.  The store belongs to the device, not to the context that loaded it:
    ``detach()`` lets go of that context, after which every context of the device may use the handle (``junction_motifs(ctx=...)``,
    ``DeviceReads.motif_strand``) and ``free()`` waits for the whole device instead of for one stream."""

    def __init__(self, ctx, path, window_bytes=0):
        self.ctx, self._h = ctx, ctypes.c_void_p()
        _check(lib().spl_genome_open(ctx._h, os.fsencode(path), ctypes.c_int64(int(window_bytes)), ctypes.byref(self._h)))
        self.names, self.lengths = [], []
        for i in range(lib().spl_genome_n(self._h)):
            name, length = ctypes.c_char_p(), ctypes.c_int64(0)
            _check(lib().spl_genome_name(self._h, ctypes.c_int(i), ctypes.byref(name), ctypes.byref(length)))
            self.names.append(name.value.decode("utf-8", "surrogateescape"))
            self.lengths.append(length.value)
        self._index = {n: i for i, n in enumerate(self.names)}

    def index(self, seq):
        if isinstance(seq, str):
            if seq not in self._index:
                raise KeyError("%s is not in the FASTA" % seq)
            return self._index[seq]
        return int(seq)

    def __contains__(self, name):
        return name in self._index

    def length(self, seq):
        return self.lengths[self.index(seq)]

    def bases(self, seq, first=0, n=None):
        """Test hook: bases first + 1 .. first + n of a sequence, a code a byte (``spl_genome_bases``)."""
        i = self.index(seq)
        n = self.lengths[i] - first if n is None else n
        out = np.zeros(max(n, 1), np.uint8)
        _check(lib().spl_genome_bases(self.ctx._h, self._h, ctypes.c_int(i), ctypes.c_int64(int(first)), ctypes.c_int64(int(n)), _ptr(out)))
        return out[:n]

    def stats(self):
        """-> dict: text_bytes, device_bytes, upload_ms, pack_ms (device time of the copies / of the kernels)."""
        t, d, u, k = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_float(0), ctypes.c_float(0)
        _check(lib().spl_genome_stats(self._h, ctypes.byref(t), ctypes.byref(d), ctypes.byref(u), ctypes.byref(k)))
        return dict(text_bytes=t.value, device_bytes=d.value, upload_ms=u.value, pack_ms=k.value)

    def junction_motifs(self, seq, left, right, ctx=None):
        """The motif codes of the rows (left, right) of a junction table of sequence ``seq`` (``spl_junction_motifs``) -> uint8[n].
        ``ctx``: another context of the genome's device than the one that loaded it."""
        left, right = _arr(left, np.int32), _arr(right, np.int32)
        out = np.zeros(max(left.shape[0], 1), np.uint8)
        _check(lib().spl_junction_motifs((ctx or self.ctx)._h, self._h, ctypes.c_int(self.index(seq)), ctypes.c_int64(left.shape[0]), _ptr(left), _ptr(right), _ptr(out)))
        return out[:left.shape[0]]

    def detach(self):
        self.ctx = None
        return self

    def free(self):
        if self._h:
            lib().spl_genome_free(self.ctx._h if self.ctx is not None else None, self._h)
            self._h = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.free()


def genome_pack_host(text):
    """The FASTA rule on the host (``spl_genome_pack_host``): bytes -> [(name bytes, codes uint8[length])]."""
    buf = np.frombuffer(bytes(text), np.uint8)
    n, nb, nc = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0)
    args = (_ptr(buf) if buf.size else None, ctypes.c_int64(buf.size), ctypes.byref(n), ctypes.byref(nb), ctypes.byref(nc))
    _check(lib().spl_genome_pack_host(*args, ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0), None, None, None, None))
    off, names = np.zeros(n.value + 1, np.int64), np.zeros(max(nb.value, 1), np.uint8)
    length, codes = np.zeros(max(n.value, 1), np.int64), np.zeros(max(nc.value, 1), np.uint8)
    _check(lib().spl_genome_pack_host(*args, ctypes.c_int64(n.value), ctypes.c_int64(nb.value), ctypes.c_int64(nc.value), _ptr(off), _ptr(names), _ptr(length), _ptr(codes)))
    out, at = [], 0
    for k in range(n.value):
        out.append((names[off[k]:off[k + 1]].tobytes(), codes[at:at + length[k]].copy()))
        at += int(length[k])
    return out


def motif_read_strand_host(reads, codes, shift=0):
    """The motif rule over host arrays (``spl_motif_read_strand_host``): ``reads`` with pos, flag, cig_off, cigar; ``codes``: the
    sequence, a code a byte -> (strand uint8[n], tally int64[12])."""
    pos, flag = _arr(reads.pos, np.int32), _arr(reads.flag, np.uint16)
    cig_off, cigar, codes = _arr(reads.cig_off, np.uint32), _arr(reads.cigar, np.uint32), _arr(codes, np.uint8)
    n = pos.shape[0]
    strand, tally = np.zeros(max(n, 1), np.uint8), np.zeros(12, np.int64)
    _check(lib().spl_motif_read_strand_host(ctypes.c_int64(n), _ptr(pos), _ptr(flag), _ptr(cig_off), _ptr(cigar) if cigar.size else None, ctypes.c_int64(cigar.shape[0]),
                                            ctypes.c_int32(int(shift)), _ptr(codes) if codes.size else None, ctypes.c_int64(codes.shape[0]), _ptr(strand), _ptr(tally)))
    return strand[:n], tally


def junction_motifs_host(codes, left, right):
    """The motif codes of junctions (left, right) over a sequence with a code a byte (``spl_junction_motifs_host``) -> uint8[n]."""
    codes, left, right = _arr(codes, np.uint8), _arr(left, np.int32), _arr(right, np.int32)
    out = np.zeros(max(left.shape[0], 1), np.uint8)
    _check(lib().spl_junction_motifs_host(_ptr(codes) if codes.size else None, ctypes.c_int64(codes.shape[0]), ctypes.c_int64(left.shape[0]), _ptr(left), _ptr(right), _ptr(out)))
    return out[:left.shape[0]]


def aux_strand_host(aux):
    """The decoders' walk over one record's aux area on the host (``spl_bam_aux_strand_host``): bytes -> ``'+'``, ``'-'`` or 0 as
    an int."""
    buf = np.frombuffer(bytes(aux), np.uint8)
    out = ctypes.c_uint8(0)
    _check(lib().spl_bam_aux_strand_host(_ptr(buf) if buf.size else None, ctypes.c_uint32(int(buf.size)), ctypes.byref(out)))
    return out.value


def _cover_arrays(cover):
    if cover is None:
        return np.zeros(0, np.int32), np.zeros(0, np.uint8)
    start, code = _arr(cover[0], np.int32), _arr(cover[1], np.uint8)
    if start.ndim != 1 or start.shape != code.shape:
        raise ValueError("a cover map is two arrays of one length: start (int32) and code (uint8)")
    return start, code


def strand_rule_host(flag, pos, ops, xs=0, cover=None, counters=None):
    """The strandedness rule for one read on the host (``spl_strand_rule_host``): adds to ``counters`` (int64[14]; made when None)
    and returns them."""
    if counters is None:
        counters = np.zeros(14, np.int64)
    assert counters.dtype == np.int64 and counters.shape == (14,) and counters.flags.c_contiguous
    ops = np.ascontiguousarray(ops, np.uint32)
    start, code = _cover_arrays(cover)
    _check(lib().spl_strand_rule_host(ctypes.c_uint32(int(flag)), ctypes.c_int32(int(pos)), _ptr(ops) if ops.shape[0] else None, ctypes.c_uint32(ops.shape[0]),
                                      ctypes.c_uint8(int(xs)), ctypes.c_int64(start.shape[0]), _ptr(start) if start.shape[0] else None,
                                      _ptr(code) if code.shape[0] else None, _ptr(counters)))
    return counters


GENE_MANY = 0xFFFFFFFF                 # a gene map's code where two or more genes cover a position
GENE_SPECIALS = ("__no_feature", "__ambiguous", "__not_counted")      # the three counters behind the genes'


def _gene_map_arrays(gene_map):
    if gene_map is None:
        return np.zeros(0, np.int32), np.zeros(0, np.uint32)
    start, code = _arr(gene_map[0], np.int32), _arr(gene_map[1], np.uint32)
    if start.ndim != 1 or start.shape != code.shape:
        raise ValueError("a gene map is two arrays of one length: start (int32) and code (uint32)")
    return start, code


def gene_count_rule_host(flag, pos, ops, n_genes, map_a, map_b=None, stranded=0, shift=0):
    """The gene-count rule for one read on the host (``spl_gene_count_rule_host``): -> the gene's index, -1 no feature, -2 ambiguous,
    -3 not counted."""
    ops = np.ascontiguousarray(ops, np.uint32)
    (a_start, a_code), (b_start, b_code) = _gene_map_arrays(map_a), _gene_map_arrays(map_b)
    out = ctypes.c_int64(0)
    _check(lib().spl_gene_count_rule_host(ctypes.c_uint32(int(flag)), ctypes.c_int32(int(pos)), _ptr(ops) if ops.shape[0] else None, ctypes.c_uint32(ops.shape[0]),
                                          ctypes.c_int32(int(shift)), ctypes.c_int(int(stranded)), ctypes.c_int64(a_start.shape[0]), _ptr(a_start) if a_start.shape[0] else None,
                                          _ptr(a_code) if a_code.shape[0] else None, ctypes.c_int64(b_start.shape[0]), _ptr(b_start) if b_start.shape[0] else None,
                                          _ptr(b_code) if b_code.shape[0] else None, ctypes.c_int64(int(n_genes)), ctypes.byref(out)))
    return out.value


MATE_NONE = 0xFFFFFFFF                 # a mate table's word for a read without a mate
MATE_COUNTS = ("pairable", "paired", "unpaired_mate_mapped")          # spl_mate_table's three counters (paired: twice the pairs)


def name_key_host(name):
    """The name key of ``name`` (bytes) by the library's rule header (``spl_name_key_host``): 0 = no name."""
    name = bytes(name)
    buf = (ctypes.c_uint8 * max(len(name), 1)).from_buffer_copy(name.ljust(1, b"\0"))
    out = ctypes.c_uint64(0)
    _check(lib().spl_name_key_host(buf, ctypes.c_int64(len(name)), ctypes.byref(out)))
    return out.value


SUBSAMPLE_ALL = 1 << 32   # spl_reads_subsample's threshold that keeps every read


def subsample_keep_host(name_key, pos, flag, cig_off, seed, threshold):
    """The subsampling rule over one segment's host arrays by the library's rule header (``spl_subsample_keep_host``, no GPU) ->
    bool[n]: the reads kept."""
    name_key, pos, flag, cig_off = _arr(name_key, np.uint64), _arr(pos, np.int32), _arr(flag, np.uint16), _arr(cig_off, np.uint32)
    n = int(name_key.shape[0])
    if pos.shape[0] != n or flag.shape[0] != n or cig_off.shape[0] != n + 1:
        raise ValueError("name_key, pos and flag have n entries, cig_off n + 1")
    keep = np.zeros(max(n, 1), np.uint8)
    _check(lib().spl_subsample_keep_host(ctypes.c_int64(n), _ptr(name_key), _ptr(pos), _ptr(flag), _ptr(cig_off), ctypes.c_uint64(int(seed)), ctypes.c_uint64(int(threshold)),
                                         _ptr(keep)))
    return keep[:n].astype(bool)


def subsample_tile():
    """The reads of a tile of ``spl_reads_subsample``'s kernels (``spl_subsample_tile``): the tests' shapes hang on it."""
    return int(lib().spl_subsample_tile())


# spl_reads_duplicates' seven counters; its histogram has DUP_HIST sums (sizes 1 .. 255, 256+, the fragments of the 256+ groups)
DUP_COUNTS = ("reads", "examined", "pair_fragments", "single_fragments", "duplicate_pairs", "duplicate_singles", "flagged_in_file")
DUP_HIST = 257


def duplicates_host(reads, name_key, mate):
    """The duplicate rule over one segment's host arrays (``ReadArrays``-like) and its mate table by the rule header behind a
    stable sort on the host (``spl_duplicates_host``, no GPU) -> (dup bool[n], counts dict, hist int64[257])."""
    name_key, mate = _arr(name_key, np.uint64), _arr(mate, np.uint32)
    if name_key.shape[0] != reads.n or mate.shape[0] != reads.n:
        raise ValueError("name_key and mate must have n_reads entries")
    dup, counts, hist = np.zeros(max(reads.n, 1), np.uint8), np.zeros(len(DUP_COUNTS), np.int64), np.zeros(DUP_HIST, np.int64)
    _check(lib().spl_duplicates_host(ctypes.c_int64(reads.n), _ptr(reads.pos), _ptr(reads.flag), _ptr(reads.cig_off), _ptr(reads.cigar) if len(reads.cigar) else None,
                                     _ptr(name_key), _ptr(mate), _ptr(dup), _ptr(counts), _ptr(hist)))
    return dup[:reads.n].astype(bool), dict(zip(DUP_COUNTS, counts.tolist())), hist


LANE_PLAN_STRIDE = 6 + 4 * 12


def lanes_plan_host(calls, n_tables, n_sets, two_lanes=True, tail_stream=True, callers_stream=False):
    """The lane rule (``csrc/spl_lanes.h``) over a sequence of calls ``(kind, a, b, c)`` (``spl_lanes_plan_host``) -> per call a dict:
    lane, piped, n_after, n_mid, tail_stream, ops [(op, stream, kind, seq)]."""
    calls = _arr(np.asarray(calls, np.int32).reshape(-1, 4), np.int32)
    out = np.zeros((max(len(calls), 1), LANE_PLAN_STRIDE), np.int64)
    _check(lib().spl_lanes_plan_host(ctypes.c_int(int(two_lanes)), ctypes.c_int(int(tail_stream)), ctypes.c_int(int(callers_stream)), ctypes.c_int(n_tables),
                                     ctypes.c_int(n_sets), ctypes.c_int64(len(calls)), _ptr(calls), _ptr(out)))
    return [dict(lane=int(r[0]), piped=int(r[1]), n_after=int(r[3]), n_mid=int(r[4]), tail_stream=int(r[5]), ops=[tuple(int(v) for v in r[6 + 4 * k:10 + 4 * k]) for k in range(int(r[2]))])
            for r in out[:len(calls)]]


def mate_table_host(reads, name_key):
    """The mate table of one segment's host arrays (``ReadArrays``-like) by the rule header on the host (``spl_mate_table_host``) ->
    (mate uint32[n], counts dict)."""
    name_key = _arr(name_key, np.uint64)
    if name_key.shape[0] != reads.n:
        raise ValueError("name_key must have n_reads entries")
    mate, counts = np.empty(max(reads.n, 1), np.uint32), np.zeros(3, np.int64)
    _check(lib().spl_mate_table_host(ctypes.c_int64(reads.n), _ptr(reads.pos), _ptr(reads.flag), _ptr(reads.cig_off), _ptr(name_key), _ptr(mate), _ptr(counts)))
    return mate[:reads.n], dict(zip(MATE_COUNTS, counts.tolist()))


def gene_fragment_rule_host(reads, mate, n_genes, map_a, map_b=None, stranded=0, shift=0):
    """The fragment rule for every read of one segment's host arrays with its mate table (``spl_gene_fragment_rule_host``) ->
    int64[n]: the gene's index, -1 no feature, -2 ambiguous, -3 not counted, -4 nothing (the read's leader counts the fragment)."""
    mate = _arr(mate, np.uint32)
    if mate.shape[0] != reads.n:
        raise ValueError("mate must have n_reads entries")
    (a_start, a_code), (b_start, b_code) = _gene_map_arrays(map_a), _gene_map_arrays(map_b)
    out = np.zeros(max(reads.n, 1), np.int64)
    _check(lib().spl_gene_fragment_rule_host(ctypes.c_int64(reads.n), _ptr(reads.pos), _ptr(reads.flag), _ptr(reads.cig_off), _ptr(reads.cigar) if reads.cigar.shape[0] else None,
                                             _ptr(mate), ctypes.c_int32(int(shift)), ctypes.c_int(int(stranded)), ctypes.c_int64(a_start.shape[0]),
                                             _ptr(a_start) if a_start.shape[0] else None, _ptr(a_code) if a_code.shape[0] else None, ctypes.c_int64(b_start.shape[0]),
                                             _ptr(b_start) if b_start.shape[0] else None, _ptr(b_code) if b_code.shape[0] else None, ctypes.c_int64(int(n_genes)), _ptr(out)))
    return out[:reads.n]


EXON_SPECIALS = ("__no_feature", "__ambiguous", "__not_counted")      # the rows behind the bins' (the counted reads are no row)


def exon_count_rule_host(flag, pos, ops, bin_gene, map_a, map_b=None, stranded=0, shift=0, cap=64):
    """The exon-bin rule for one read on the host (``spl_exon_count_rule_host``): -> (verdict, bins, n_hits) -- 0 counted, -1 no
    feature, -2 ambiguous, -3 not counted; a counted read's first ``cap`` bins; the number of its bins, also beyond ``cap``."""
    ops, bin_gene = np.ascontiguousarray(ops, np.uint32), _arr(bin_gene, np.uint32)
    (a_start, a_code), (b_start, b_code) = _gene_map_arrays(map_a), _gene_map_arrays(map_b)
    verdict, n_hits, bins = ctypes.c_int64(0), ctypes.c_int64(0), np.zeros(max(int(cap), 1), np.int64)
    _check(lib().spl_exon_count_rule_host(ctypes.c_uint32(int(flag)), ctypes.c_int32(int(pos)), _ptr(ops) if ops.shape[0] else None, ctypes.c_uint32(ops.shape[0]),
                                          ctypes.c_int32(int(shift)), ctypes.c_int(int(stranded)), ctypes.c_int64(a_start.shape[0]), _ptr(a_start) if a_start.shape[0] else None,
                                          _ptr(a_code) if a_code.shape[0] else None, ctypes.c_int64(b_start.shape[0]), _ptr(b_start) if b_start.shape[0] else None,
                                          _ptr(b_code) if b_code.shape[0] else None, ctypes.c_int64(bin_gene.shape[0]), _ptr(bin_gene) if bin_gene.shape[0] else None,
                                          ctypes.byref(verdict), _ptr(bins), ctypes.c_int64(int(cap)), ctypes.byref(n_hits)))
    return verdict.value, bins[:min(int(cap), n_hits.value)].tolist(), n_hits.value


def exon_fragment_rule_host(reads, mate, bin_gene, map_a, map_b=None, stranded=0, shift=0, cap=4096):
    """The exon-bin fragment rule for every read of one segment's host arrays with its mate table (``spl_exon_fragment_rule_host``)
    -> (verdict int64[n], n_hits int64[n], bins int64[min(cap, sum of n_hits)]): 0 counted, -1 no feature, -2 ambiguous, -3 not
    counted, -4 silent (the read's leader counts the fragment); a counted leader's number of distinct bins, also beyond ``cap``; the
    counted leaders' merged bins, one fragment after the other in read order, as far as ``cap`` reaches."""
    mate, bin_gene = _arr(mate, np.uint32), _arr(bin_gene, np.uint32)
    if mate.shape[0] != reads.n:
        raise ValueError("mate must have n_reads entries")
    (a_start, a_code), (b_start, b_code) = _gene_map_arrays(map_a), _gene_map_arrays(map_b)
    verdict, n_hits, bins = np.zeros(max(reads.n, 1), np.int64), np.zeros(max(reads.n, 1), np.int64), np.zeros(max(int(cap), 1), np.int64)
    _check(lib().spl_exon_fragment_rule_host(ctypes.c_int64(reads.n), _ptr(reads.pos), _ptr(reads.flag), _ptr(reads.cig_off), _ptr(reads.cigar) if reads.cigar.shape[0] else None,
                                             _ptr(mate), ctypes.c_int32(int(shift)), ctypes.c_int(int(stranded)), ctypes.c_int64(a_start.shape[0]),
                                             _ptr(a_start) if a_start.shape[0] else None, _ptr(a_code) if a_code.shape[0] else None, ctypes.c_int64(b_start.shape[0]),
                                             _ptr(b_start) if b_start.shape[0] else None, _ptr(b_code) if b_code.shape[0] else None, ctypes.c_int64(bin_gene.shape[0]),
                                             _ptr(bin_gene) if bin_gene.shape[0] else None, _ptr(verdict), _ptr(n_hits), _ptr(bins), ctypes.c_int64(int(cap))))
    verdict, n_hits = verdict[:reads.n], n_hits[:reads.n]
    return verdict, n_hits, bins[:min(int(cap), int(n_hits.sum()))]


INTRON_LONG_BASES = 16384   # csrc/spl_intron.h's SPL_INTRON_LONG_BASES: an intron of this many measurable bases or more has a team of its own


def intron_depth_runs(ctx, bound_pos, bound_depth, length, piece_off, piece_start, piece_end, trim_percent=30):
    """``spl_intron_depth``'s kernel over a caller's boundaries (``spl_intron_depth_runs``: test hook) -> int64[n_introns, 4].
    ``bound_pos`` strictly ascending; ``bound_depth[k]`` holds from ``bound_pos[k]`` to the next one, 0 before the first."""
    pos, depth = _arr(bound_pos, np.int32), _arr(bound_depth, np.uint32)
    off, start, end = _arr(piece_off, np.int64), _arr(piece_start, np.int32), _arr(piece_end, np.int32)
    n = max(int(off.shape[0]) - 1, 0)
    out = np.zeros((n, 4), np.int64)
    _check(lib().spl_intron_depth_runs(ctx._h, ctypes.c_int64(pos.shape[0]), _ptr(pos) if pos.shape[0] else None, _ptr(depth) if depth.shape[0] else None,
                                       ctypes.c_int64(int(length)), ctypes.c_int64(n), _ptr(off) if off.shape[0] else None, _ptr(start) if start.shape[0] else None,
                                       _ptr(end) if end.shape[0] else None, ctypes.c_int(int(trim_percent)), _ptr(out) if n else None))
    return out


def intron_depth_host(bound_pos, bound_depth, piece_start, piece_end, trim_percent=30):
    """The intron rule for ONE intron on the host, by sorting (``spl_intron_depth_host``: test hook, no GPU) -> [L, covered, depth_n,
    depth_sum]."""
    pos, depth = _arr(bound_pos, np.int32), _arr(bound_depth, np.uint32)
    start, end = _arr(piece_start, np.int32), _arr(piece_end, np.int32)
    out = np.zeros(4, np.int64)
    _check(lib().spl_intron_depth_host(ctypes.c_int64(pos.shape[0]), _ptr(pos) if pos.shape[0] else None, _ptr(depth) if depth.shape[0] else None, ctypes.c_int64(start.shape[0]),
                                       _ptr(start) if start.shape[0] else None, _ptr(end) if end.shape[0] else None, ctypes.c_int(int(trim_percent)), _ptr(out)))
    return out.tolist()


COVERAGE_TOTALS = ("runs", "reads_seen", "contributed", "past_end", "covered_bases")
COVERAGE_FRAGMENT_TOTALS = COVERAGE_TOTALS + ("pairs",)          # spl_coverage_fragment_totals' six
COVF_CONTRIBUTED, COVF_NOTHING, COVF_NOT_PARTICIPATING, COVF_SILENT = 1, 0, -3, -4          # spl_coverage_fragment_rule_host's status of a read


def coverage_rule_host(flag, pos, ops, length, shift=0, stranded=0, strand=0):
    """The coverage rule for one read on the host (``spl_coverage_rule_host``): -> ([(start, end)] its clipped blocks on the track,
    whether it lost a base to the clipping)."""
    ops = np.ascontiguousarray(ops, np.uint32)
    strand = ord(strand) if isinstance(strand, (str, bytes)) else int(strand)
    cap = max(1, ops.shape[0])
    s, e = np.empty(cap, np.int64), np.empty(cap, np.int64)
    n, past = ctypes.c_int(0), ctypes.c_int(0)
    _check(lib().spl_coverage_rule_host(ctypes.c_uint32(int(flag)), ctypes.c_int32(int(pos)), _ptr(ops) if ops.shape[0] else None, ctypes.c_uint32(ops.shape[0]),
                                        ctypes.c_int32(int(shift)), ctypes.c_int64(int(length)), ctypes.c_int(int(stranded)), ctypes.c_int(strand), ctypes.c_int(cap),
                                        _ptr(s), _ptr(e), ctypes.byref(n), ctypes.byref(past)))
    return list(zip(s[:n.value].tolist(), e[:n.value].tolist())), bool(past.value)


def junction_fragment_rule_host(reads, mate, stranded=0, min_anchor=0, min_intron=0, max_intron=0, shift=0, xs=None, cap=1 << 16):
    """The junction fragment rule for every read of one segment's host arrays with its mate table
    (``spl_junction_fragment_rule_host``) -> (counted int64[n], duplicate int64[n], rows int64[min(cap, all), 6]: left, right, strand
    byte, anchor_left, anchor_right, duplicate -- every supported junction in read and walk order)."""
    mate = _arr(mate, np.uint32)
    if mate.shape[0] != reads.n:
        raise ValueError("mate must have n_reads entries")
    xs = None if xs is None else _arr(xs, np.uint8)
    counted, dup = np.zeros(max(reads.n, 1), np.int64), np.zeros(max(reads.n, 1), np.int64)
    rows, n_rows = np.zeros((max(int(cap), 1), 6), np.int64), ctypes.c_int64(0)
    _check(lib().spl_junction_fragment_rule_host(ctypes.c_int64(reads.n), _ptr(reads.pos), _ptr(reads.flag), _ptr(reads.cig_off), _ptr(reads.cigar) if reads.cigar.shape[0] else None,
                                                 _ptr(xs), _ptr(mate), ctypes.c_int32(int(shift)), ctypes.c_int(int(stranded)), ctypes.c_int32(int(min_anchor)),
                                                 ctypes.c_int32(int(min_intron)), ctypes.c_int32(int(max_intron)), _ptr(counted), _ptr(dup), _ptr(rows), ctypes.c_int64(int(cap)),
                                                 ctypes.byref(n_rows)))
    return counted[:reads.n], dup[:reads.n], rows[:min(int(cap), n_rows.value)]


def coverage_cursor_host(flag, pos, ops, length, shift=0, stranded=0, strand=0):
    """``coverage_rule_host``'s arguments and results by the fragment rule's resumable block cursor (``spl_coverage_cursor_host``)."""
    ops = np.ascontiguousarray(ops, np.uint32)
    strand = ord(strand) if isinstance(strand, (str, bytes)) else int(strand)
    cap = max(1, ops.shape[0])
    s, e = np.empty(cap, np.int64), np.empty(cap, np.int64)
    n, past = ctypes.c_int(0), ctypes.c_int(0)
    _check(lib().spl_coverage_cursor_host(ctypes.c_uint32(int(flag)), ctypes.c_int32(int(pos)), _ptr(ops) if ops.shape[0] else None, ctypes.c_uint32(ops.shape[0]),
                                          ctypes.c_int32(int(shift)), ctypes.c_int64(int(length)), ctypes.c_int(int(stranded)), ctypes.c_int(strand), ctypes.c_int(cap),
                                          _ptr(s), _ptr(e), ctypes.byref(n), ctypes.byref(past)))
    return list(zip(s[:n.value].tolist(), e[:n.value].tolist())), bool(past.value)


def coverage_fragment_rule_host(reads, mate, length, shift=0, stranded=0, strand=0, cap=1 << 16):
    """The fragment coverage rule for every read of one segment's host arrays with its mate table
    (``spl_coverage_fragment_rule_host``) -> (status int64[n]: ``COVF_*``, n_iv int64[n]: the intervals of a read's union, also beyond
    ``cap``, past bool[n], intervals [(start, end)]: the reads' unions one after the other in read order as far as ``cap`` reaches,
    totals: dict of ``COVERAGE_FRAGMENT_TOTALS``, ``runs`` being the intervals)."""
    mate = _arr(mate, np.uint32)
    if mate.shape[0] != reads.n:
        raise ValueError("mate must have n_reads entries")
    strand = ord(strand) if isinstance(strand, (str, bytes)) else int(strand)
    status, n_iv, past = np.zeros(max(reads.n, 1), np.int64), np.zeros(max(reads.n, 1), np.int64), np.zeros(max(reads.n, 1), np.uint8)
    s, e, totals = np.zeros(max(int(cap), 1), np.int64), np.zeros(max(int(cap), 1), np.int64), np.zeros(6, np.int64)
    _check(lib().spl_coverage_fragment_rule_host(ctypes.c_int64(reads.n), _ptr(reads.pos), _ptr(reads.flag), _ptr(reads.cig_off), _ptr(reads.cigar) if reads.cigar.shape[0] else None,
                                                 _ptr(mate), ctypes.c_int32(int(shift)), ctypes.c_int64(int(length)), ctypes.c_int(int(stranded)), ctypes.c_int(strand), _ptr(status),
                                                 _ptr(n_iv), _ptr(past), _ptr(s), _ptr(e), ctypes.c_int64(int(cap)), _ptr(totals)))
    used = min(int(cap), int(n_iv[:reads.n].sum()))
    return status[:reads.n], n_iv[:reads.n], past[:reads.n].astype(bool), list(zip(s[:used].tolist(), e[:used].tolist())), dict(zip(COVERAGE_FRAGMENT_TOTALS, totals.tolist()))


def bedgraph_append(path, chrom, start, end, depth, per_million_of=0):
    """Runs of one chromosome appended to a bedGraph file (``spl_bedgraph_append``): ``chrom\tstart\tend\tvalue`` lines, the value
    the depth or, with ``per_million_of=N``, what ``repr(depth * 1000000 / N)`` gives."""
    start, end, depth = _arr(start, np.int32), _arr(end, np.int32), _arr(depth, np.uint32)
    n = start.shape[0]
    if end.shape[0] != n or depth.shape[0] != n:
        raise ValueError("start, end and depth are three arrays of one length")
    _check(lib().spl_bedgraph_append(os.fsencode(path), chrom.encode("utf-8"), ctypes.c_int64(n), _ptr(start) if n else None, _ptr(end) if n else None,
                                     _ptr(depth) if n else None, ctypes.c_int64(int(per_million_of))))


def simple_span_host(site_pos, pos, length, is_simple, shift=0, reads_per_thread=4):
    """The fused range kernel's rule for a thread's simple reads on the host (``spl_simple_span_host``).  ``pos``, ``length``
    (1 .. 65535) and ``is_simple`` hold ``reads_per_thread`` reads a thread.  -> (flagged[threads], emits, lo, ub [reads]): whether
    the span of a thread's simple reads holds a site, and for a flagged thread's simple reads their ranges of distinct positions
    (0 for every other read)."""
    site_pos = _arr(site_pos, np.int32)
    pos, length, is_simple = _arr(pos, np.int32), _arr(length, np.uint16), _arr(is_simple, np.uint8)
    n = pos.shape[0]
    if n % reads_per_thread or length.shape[0] != n or is_simple.shape[0] != n:
        raise ValueError("pos, length and is_simple hold reads_per_thread reads a thread")
    n_threads = n // reads_per_thread
    flagged, emits = np.zeros(n_threads, np.uint8), np.zeros(n, np.uint8)
    lo, ub = np.zeros(n, np.int32), np.zeros(n, np.int32)
    _check(lib().spl_simple_span_host(_ptr(site_pos), ctypes.c_int64(site_pos.shape[0]), ctypes.c_int64(n_threads), ctypes.c_int(reads_per_thread),
                                      _ptr(pos), _ptr(length), _ptr(is_simple), ctypes.c_int32(int(shift)), _ptr(flagged), _ptr(emits), _ptr(lo), _ptr(ub)))
    return flagged.astype(bool), emits.astype(bool), lo, ub


def junction_walk_host(ops, pos, min_anchor=0, min_intron=0, max_intron=0):
    """The junction kernels' per-read walk on the host (``spl_junction_walk_host``): -> ([(left, right, anchor_left,
    anchor_right, passes)], range_error)."""
    ops = np.ascontiguousarray(ops, np.uint32)
    cap = max(1, ops.shape[0])
    left, right = np.empty(cap, np.int32), np.empty(cap, np.int32)
    al, ar, ok = np.empty(cap, np.uint32), np.empty(cap, np.uint32), np.empty(cap, np.uint8)
    n, bad = ctypes.c_int(0), ctypes.c_int(0)
    _check(lib().spl_junction_walk_host(_ptr(ops), ctypes.c_uint32(ops.shape[0]), ctypes.c_int32(int(pos)), ctypes.c_int32(int(min_anchor)),
                                        ctypes.c_int32(int(min_intron)), ctypes.c_int32(int(max_intron)), ctypes.c_int(cap), _ptr(left), _ptr(right),
                                        _ptr(al), _ptr(ar), _ptr(ok), ctypes.byref(n), ctypes.byref(bad)))
    k = n.value
    return list(zip(left[:k].tolist(), right[:k].tolist(), al[:k].tolist(), ar[:k].tolist(), [bool(x) for x in ok[:k].tolist()])), bool(bad.value)


def pack_host(reads, threads=1):
    """The host packer alone (``spl_pack_host``): -> (chunk descriptors as a structured array, record blob uint8, wide ops)."""
    nc, rb, nw = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0)
    _check(lib().spl_pack_host(ctypes.byref(reads.c), ctypes.c_int(threads), ctypes.byref(nc), ctypes.byref(rb), ctypes.byref(nw),
                               None, None, None))
    desc = np.zeros(max(nc.value, 1), np.dtype([("rec_off", "<u8"), ("wide_off", "<u8"), ("first_pos", "<i4"), ("cost", "<u4"),
                                                 ("n", "<u2", (4,))]))
    rec = np.zeros(max(rb.value, 1), np.uint8)
    wide = np.zeros(max(nw.value, 1), np.uint32)
    _check(lib().spl_pack_host(ctypes.byref(reads.c), ctypes.c_int(threads), ctypes.byref(nc), ctypes.byref(rb), ctypes.byref(nw),
                               _ptr(desc), _ptr(rec), _ptr(wide)))
    return desc[:nc.value], rec[:rb.value], wide[:nw.value]


class TextColumns(object):
    """A BED12 junction file or the gene lines of an annotation as columns (``spl_bed_open`` / ``spl_gff_open``)."""
    __slots__ = ("chrom_names", "chrom", "left", "right", "alpha", "strand", "names")


def _text_columns(opener, path, with_alpha, with_names):
    h = ctypes.c_void_p()
    rc = opener(os.fsencode(path), ctypes.byref(h))
    if rc == -5:
        return None           # something the native reader will not vouch for: the caller reads line by line
    _check(rc)
    try:
        L = lib()
        rows = L.spl_text_rows(h)

        def col(ptr, dt):
            if not rows:
                return np.zeros(0, dt)
            return np.ctypeslib.as_array(ctypes.cast(ptr, ctypes.POINTER(np.ctypeslib.as_ctypes_type(dt))), shape=(rows,)).copy()
        out = TextColumns()
        out.chrom_names = [L.spl_text_chrom_name(h, k).decode("utf-8") for k in range(L.spl_text_n_chrom(h))]
        out.chrom = col(L.spl_text_chrom(h), np.int32)
        out.left = col(L.spl_text_i64(h, 0), np.int64)
        out.right = col(L.spl_text_i64(h, 1), np.int64)
        out.alpha = col(L.spl_text_i64(h, 2), np.int64) if with_alpha else None
        out.strand = col(L.spl_text_strand(h), np.uint8)
        out.names = None
        if with_names:
            off_p = ctypes.c_void_p()
            blob_p = L.spl_text_names(h, ctypes.byref(off_p))
            off = np.ctypeslib.as_array(ctypes.cast(off_p, ctypes.POINTER(ctypes.c_uint32)), shape=(rows + 1,)).tolist()
            blob = ctypes.string_at(blob_p, off[-1]) if rows and off[-1] else b""
            out.names = [blob[off[i]:off[i + 1]].decode("ascii") for i in range(rows)]
        return out
    except UnicodeDecodeError:
        return None
    finally:
        lib().spl_text_close(h)


def read_bed_columns(path):
    """-> TextColumns of the 12-column lines of a BED file, or None when the file must be read line by line."""
    return _text_columns(lib().spl_bed_open, path, True, False)


def read_gff_genes(path):
    """-> TextColumns of the ``gene`` lines of a GFF / GTF file, or None when the file must be read line by line."""
    return _text_columns(lib().spl_gff_open, path, False, True)


class spl_query_table(ctypes.Structure):
    _fields_ = [("chrom", ctypes.c_char_p), ("n", ctypes.c_int64), ("pos", ctypes.c_void_p), ("site", ctypes.c_void_p),
                ("strand", ctypes.c_void_p), ("part_off", ctypes.c_void_p), ("part_pos", ctypes.c_void_p),
                ("comp_off", ctypes.c_void_p), ("comp_pos", ctypes.c_void_p)]


def _view(addr, n, dt):
    """n items of dtype dt at address addr, copied out (the library owns the memory)."""
    if n == 0 or not addr:
        return np.zeros(0, dt)
    return np.ctypeslib.as_array(ctypes.cast(addr, ctypes.POINTER(np.ctypeslib.as_ctypes_type(dt))), shape=(n,)).copy()


def _ascii_gene(gene):
    """The native walk compares gene names as bytes of files it has checked to be ASCII: a name outside ASCII can match nothing there,
    and must not be turned into '?' (a gene may be called that) -- the Python walk takes it."""
    try:
        return str(gene).encode("ascii")
    except UnicodeEncodeError:
        raise SpliserNativeError(-5, "gene name %r is not ASCII: the Python walk of combine takes it" % (gene,))


class Combine(object):
    """The host walk of ``combine`` / ``combineShallow`` on columns (``spl_combine_*``, csrc/spl_combine.cpp): the per-sample
    .SpliSER.tsv files parsed and merged natively, the gap-fill queries as tables, the answers handed back, the .combined.tsv
    written.  Raises SpliserNativeError with code -5 for files the native parser does not take (spliser_amd/combine.py then
    walks them in Python)."""

    def __init__(self, tsv_paths):
        self._h = None
        self.n = len(tsv_paths)
        paths = (ctypes.c_char_p * self.n)(*[os.fsencode(p) for p in tsv_paths])
        h = ctypes.c_void_p()
        _check(lib().spl_combine_open(paths, ctypes.c_int32(self.n), ctypes.byref(h)))
        self._h = h

    def close(self):
        if self._h:
            lib().spl_combine_close(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        self.close()

    def rows(self, idx):
        return int(lib().spl_combine_rows(self._h, ctypes.c_int32(idx)))

    def region_runs(self):
        """-> per sample the regions of its file in order, one entry per run of lines."""
        L = lib()
        out = []
        for idx in range(self.n):
            n = int(L.spl_combine_region_runs(self._h, ctypes.c_int32(idx), None, ctypes.c_int64(0)))
            ids = np.zeros(max(n, 1), np.int32)
            L.spl_combine_region_runs(self._h, ctypes.c_int32(idx), _ptr(ids), ctypes.c_int64(n))
            out.append([L.spl_combine_text(self._h, ctypes.c_int32(int(i))).decode("ascii") for i in ids[:n]])
        return out

    def keep_gene(self, gene):
        _check(lib().spl_combine_keep_gene(self._h, _ascii_gene(gene)))

    def merge(self, chroms, is_stranded, q_gene, shallow=None):
        """The lock-step walk.  -> [(position, samples with evidence)] of the sites combineShallow dropped."""
        names = (ctypes.c_char_p * max(len(chroms), 1))(*[c.encode("ascii", "replace") for c in chroms])
        ms, mr, me = (0, 0, 0.0) if shallow is None else shallow
        _check(lib().spl_combine_merge(self._h, names, ctypes.c_int32(len(chroms)), ctypes.c_int(1 if is_stranded else 0),
                                       _ascii_gene(q_gene), ctypes.c_int(0 if shallow is None else 1),
                                       ctypes.c_int64(int(ms)), ctypes.c_int64(int(mr)), ctypes.c_double(float(me))))
        p = ctypes.c_void_p()
        n = int(lib().spl_combine_skipped(self._h, ctypes.byref(p)))
        sk = _view(p.value, 2 * n, np.int64)
        return [(int(sk[2 * k]), int(sk[2 * k + 1])) for k in range(n)]

    @property
    def n_sites(self):
        return int(lib().spl_combine_n_sites(self._h))

    @property
    def n_gap_sites(self):
        return int(lib().spl_combine_n_gap_sites(self._h))

    def tables(self, idx):
        """The gap-fill queries of sample idx: [(region, dict of arrays: pos, site, strand, part_off, part_pos, comp_off, comp_pos)]
        in the order the walk met the regions, rows by position."""
        L = lib()
        out = []
        for k in range(int(L.spl_combine_n_tables(self._h, ctypes.c_int32(idx)))):
            t = spl_query_table()
            _check(L.spl_combine_table(self._h, ctypes.c_int32(idx), ctypes.c_int32(k), ctypes.byref(t)))
            n = int(t.n)
            part_off = _view(t.part_off, n + 1, np.uint32)
            comp_off = _view(t.comp_off, n + 1, np.uint32)
            out.append((t.chrom.decode("ascii"), dict(
                pos=_view(t.pos, n, np.int64), site=_view(t.site, n, np.int64), strand=_view(t.strand, n, np.uint8),
                part_off=part_off, part_pos=_view(t.part_pos, int(part_off[-1]), np.int64),
                comp_off=comp_off, comp_pos=_view(t.comp_pos, int(comp_off[-1]), np.int64))))
        return out

    def answers(self, idx, site, beta1, beta2_simple):
        site, beta1, b2 = _arr(site, np.int64), _arr(beta1, np.uint32), _arr(beta2_simple, np.uint32)
        _check(lib().spl_combine_answers(self._h, ctypes.c_int32(idx), ctypes.c_int64(site.shape[0]), _ptr(site), _ptr(beta1), _ptr(b2)))

    def write(self, path, titles, cryptic):
        t = (ctypes.c_char_p * self.n)(*[s.encode("utf-8") for s in titles])
        _check(lib().spl_combine_write(self._h, os.fsencode(path), t, ctypes.c_int(1 if cryptic else 0)))
