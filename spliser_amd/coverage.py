"""``coverage`` -- per-base read depth as a bedGraph, from the decode of the alignment file: no sorted, indexed BAM needed to look at
the data.

Not part of SpliSER v0.1.8: its README sends the user to IGV whenever something looks wrong, and to validate a diffSpliSER hit.  IGV
wants a coordinate-sorted, indexed BAM -- the very file ``--anyOrder`` and the SAM-text inputs spare the user -- or a coverage track
from a second tool (``bedtools genomecov -bg -split``, deepTools ``bamCoverage``) run over the file this build has just decoded.
``junctions`` writes the arcs of such a view; this writes the other half.  The decode leaves POS, FLAG and CIGAR of every reference
on the device, and ``spl_coverage`` reduces them to runs of equal depth there (the rule: include/spliser.h,
csrc/spl_coverage_rule.h): a read counts when it is mapped (FLAG 0x4 clear), secondary, supplementary, duplicate and QC-failed
reads included, as in bedtools genomecov -- ``--excludeFlags 0x704`` gives samtools depth's default set --; M, = and X cover, D and
N are gaps (``-split``); blocks are clipped to the reference's length.  Parity with bedtools / deepTools is intended and unpinned
(neither tool is on the build machine): the yardstick is that statement of the rule.

``--perMillion`` divides every depth by the library size ``--flagstat`` logs (mapped reads, under the filters) and multiplies by
10^6: the value column is ``repr(depth * 1000000 / N)``.
"""
import sys

import numpy as np

from . import native, process as _process

SUFFIX, SUFFIX_PLUS, SUFFIX_MINUS = ".bedgraph", ".plus.bedgraph", ".minus.bedgraph"
STRANDED = {"fr": 1, "rf": 2}


def tracks_of(stranded):
    """-> [(file suffix, strand argument)] of a run: one track, or the '+' and the '-' one."""
    return [(SUFFIX_PLUS, "+"), (SUFFIX_MINUS, "-")] if stranded else [(SUFFIX, 0)]


def sets_of_source(source, device, chroms):
    """A finished, fused read set per chromosome of ``chroms`` that has a read, each in turn: yields (chrom, length, dr).  On the
    plan of ``strandedness.tally_of_source``, one device: a file decoded on the device is visited per chromosome where it lies (one
    fused set a chromosome, shift 0); host-decoded reads and the Python reader's go up as four arrays, a fused set of their own.
    ``length``: the header's LN; a source without lengths uses the reads' ``max_end``."""
    is_bam = isinstance(source, native.BamFile)
    on_device = is_bam and source.join_decoders()      # (False: the host threads have the file)
    lengths = dict(zip(source.ref_names, source.ref_lengths)) if getattr(source, "ref_lengths", None) else {}
    with native.Context(device) as ctx:
        for chrom in chroms:
            length = int(lengths.get(chrom, 0))
            if on_device:
                with ctx.begin_reads() as dr:
                    if not dr.add_bam(source, chrom):
                        continue
                    dr.finish()
                    yield chrom, length, dr
                continue
            rs = source.reads(chrom)
            if rs is None or not rs.n:
                continue
            if length < 1:
                length = int(rs.max_end)       # (the last base a read covers, 1-based: as many bases as the reads can tell of)
            if length < 1:
                continue                        # (no read covers a base: nothing to write, and no length to clip to)
            with ctx.upload_soa([native.ReadArrays(rs.pos, rs.flag, rs.cig_off, rs.cigar)], [getattr(rs, "max_end", None)]) as soa:
                with ctx.begin_reads() as dr:
                    dr.add_soa(soa, 0)
                    dr.finish()
                    yield chrom, length, dr


def runs_of_source(source, device, chroms, stranded=0):
    """``spl_coverage`` over every chromosome of ``chroms`` in turn (``sets_of_source``), every track of it: yields (chrom, length,
    [(start, end, depth, totals) per track])."""
    for chrom, length, dr in sets_of_source(source, device, chroms):
        yield chrom, length, [dr.coverage(length, stranded, strand) for _, strand in tracks_of(stranded)]


def coverage(inBAM, outputPath, qChrom="All", isStranded=False, strandedType=None, perMillion=False, devices=(0,), threads=0, log=None, gpuDecode=None,
             minMapQ=0, requireFlags=0, excludeFlags=0, anyOrder=False):
    """The ``coverage`` command: one decode, ``<outputPath>.bedgraph`` -- or, ``isStranded`` with ``strandedType`` ``fr`` / ``rf``,
    ``<outputPath>.plus.bedgraph`` and ``<outputPath>.minus.bedgraph`` -- with the chromosomes in header order (``qChrom``: that one)
    and no track line.  ``perMillion``: values per million mapped reads (the decode counts them: ``DecodeOptions(flagstat=True)``; a
    source without those counters is an error).  With several devices the file is decoded and covered on the first: there are no
    shares.  -> {file path: number of runs written}."""
    log = log or (lambda msg: (print(msg), sys.stdout.flush()))
    if isStranded and strandedType not in STRANDED:
        raise ValueError("coverage: --isStranded needs -s fr or -s rf (the `strandedness` command tells which)")
    stranded = STRANDED[strandedType] if isStranded else 0
    devices = tuple(devices)
    if len(devices) > 1:
        log("  (coverage: the alignment file is decoded and covered on device %d alone, not in shares over %d devices)" % (devices[0], len(devices)))
        devices = devices[:1]
    options = _process.DecodeOptions(_process.read_filter(minMapQ, requireFlags, excludeFlags), flagstat=bool(perMillion), any_order=bool(anyOrder))
    source = _process.open_and_decode(inBAM, devices, gpuDecode, threads, options, log=log)
    tracks = tracks_of(stranded)
    paths = [outputPath + suffix for suffix, _ in tracks]
    written = dict.fromkeys(paths, 0)
    held = []          # --perMillion: (chrom, runs per track) until the library size is known
    sums = np.zeros((len(tracks), 5), np.int64)
    try:
        if isinstance(source, native.BamFile):
            source.wait_all()      # (every reference is complete at the end of the file, whatever its order)
        if anyOrder:
            _process.log_any_order(source, log)
        for path in paths:
            open(path, "w").close()
        chroms = [c for c in source.ref_names if qChrom == c or qChrom == "All"]
        for chrom, length, per_track in runs_of_source(source, devices[0], chroms, stranded):
            for k, (start, end, depth, totals) in enumerate(per_track):
                name = "%s (%s)" % (chrom, tracks[k][1]) if stranded else chrom
                log("  %s: %d runs, %d covered bases" % (name, totals["runs"], totals["covered_bases"]))
                if totals["past_end"]:
                    log("  %d reads ran past the end of %s (%d bases)" % (totals["past_end"], name, length))
                sums[k] += [totals[key] for key in native.COVERAGE_TOTALS]
                if not perMillion:
                    native.bedgraph_append(paths[k], chrom, start, end, depth)
                    written[paths[k]] += int(start.shape[0])
            if perMillion:
                held.append((chrom, [t[:3] for t in per_track]))
        if perMillion:
            from . import flagstat as _flagstat
            counts = source.flagstat()
            size = int(counts[_flagstat.MAPPED][0])
            log("Library size: %d mapped reads (%d primary)" % (size, int(counts[_flagstat.PRIMARY_MAPPED][0])))
            if size < 1 and any(r[0].shape[0] for _, per_track in held for r in per_track):
                raise native.SpliserNativeError(-1, "coverage --perMillion: the library size is 0 mapped reads")
            for chrom, per_track in held:
                for k, (start, end, depth) in enumerate(per_track):
                    native.bedgraph_append(paths[k], chrom, start, end, depth, per_million_of=size)
                    written[paths[k]] += int(start.shape[0])
        _process.log_filter(source, options.read_filter, log)
    finally:
        if hasattr(source, "close"):
            source.close()
    for k, path in enumerate(paths):
        log("%s: %d runs, %d covered bases, %d of %d reads contributed%s" % (path, sums[k][0], sums[k][4], sums[k][2], sums[k][1],
                                                                          ", %d ran past the end of their reference" % sums[k][3] if sums[k][3] else ""))
    return written
