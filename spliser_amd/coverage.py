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

``--fragments`` covers a paired-end library per FRAGMENT, as deepTools ``bamCoverage`` does by default and ``bedtools genomecov -pc``:
where the mates of a pair overlap one molecule was sequenced, and the depth there is one.  The decode then keeps a 64-bit key of
every read's name (``mate_keys``), the mate table is built on the GPU per chromosome (``spl_mate_table``) and
``spl_coverage_fragments`` marks, for a pair whose mates both cover on the track, the UNION of both reads' blocks once (the rule:
include/spliser.h, csrc/spl_covfragment_rule.h).  The gap between two mates is not filled.  A pair split over two chromosomes, by
the read filter or -- stranded -- over the two tracks is two single fragments; names are compared by a 63-bit hash.  The files have
the same names and format.  ``--perMillion --fragments`` is refused: no fragment library size is counted, and fragment depth divided
by mapped reads would mislead.  Parity with deepTools / bedtools -pc is intended and unpinned: the yardstick is
tests/covfragcases.py.
"""
import numpy as np

from . import native, process as _process, readsets

SUFFIX, SUFFIX_PLUS, SUFFIX_MINUS = ".bedgraph", ".plus.bedgraph", ".minus.bedgraph"


def tracks_of(stranded):
    """-> [(file suffix, strand argument)] of a run: one track, or the '+' and the '-' one."""
    return [(SUFFIX_PLUS, "+"), (SUFFIX_MINUS, "-")] if stranded else [(SUFFIX, 0)]


def sets_of_source(source, device, chroms, with_keys=False):
    """A finished, fused read set per chromosome of ``chroms`` that has a read, each in turn: yields (chrom, length, dr); the set is
    freed when the next one is asked for.  On the plan of ``readsets``, one device and the calling thread: a file decoded on the
    device is visited per chromosome where it lies (one fused set a chromosome, shift 0); reads on the host go up as four arrays, a
    fused set of their own -- ``with_keys``: with their name keys, which the source must have (``DecodeOptions.mate_keys``).
    ``length``: the header's LN; a source without lengths uses the reads' ``max_end``, and a chromosome of it no read of which covers
    a base is skipped (its set has gone up by then: it holds no covering read, and nothing is written of it)."""
    if with_keys:
        readsets.check_fragment_source(source)
    lengths = dict(zip(source.ref_names, source.ref_lengths)) if getattr(source, "ref_lengths", None) else {}
    plans = readsets.plans_of(source, (device,), chroms)
    if len(plans) != 1:
        raise native.SpliserNativeError(-1, "the read sets are visited on one device in turn: this file was decoded in %d shares" % len(plans))
    entries = plans[0][1]
    with native.Context(device) as ctx:
        for chrom, add in entries:
            with readsets.fused_set(ctx, source, chrom, add, with_keys=with_keys) as dr:
                if dr is None:
                    continue
                length = int(lengths.get(chrom, 0))
                if add is None and length < 1:
                    length = int(source.reads(chrom).max_end)       # (the last base a read covers, 1-based: as many bases as the reads can tell of)
                    if length < 1:
                        continue                                    # (no read covers a base: nothing to write, and no length to clip to)
                yield chrom, length, dr


def union_text(tracks, taken):
    """The log's words for the pairs whose union was taken, per track."""
    if len(tracks) == 1:
        return "%d pairs whose union was taken" % taken[0]
    return "pairs whose union was taken: " + ", ".join("%d (%s)" % (n, strand) for (_, strand), n in zip(tracks, taken))


def runs_of_source(source, device, chroms, stranded=0, fragments=False, mates=None):
    """``spl_coverage`` over every chromosome of ``chroms`` in turn (``sets_of_source``), every track of it: yields (chrom, length,
    [(start, end, depth, totals) per track]).  ``fragments``: ``spl_coverage_fragments`` (the source was decoded with ``mate_keys``);
    ``mates``: a dict that gets every chromosome's mate table counters."""
    for chrom, length, dr in sets_of_source(source, device, chroms, with_keys=bool(fragments)):
        per_track = [dr.coverage(length, stranded, strand, fragments=bool(fragments)) for _, strand in tracks_of(stranded)]
        if fragments and mates is not None:
            mates[chrom] = dr.mate_table(0)[1]
        yield chrom, length, per_track


def coverage(inBAM, outputPath, qChrom="All", isStranded=False, strandedType=None, perMillion=False, devices=(0,), threads=0, log=None, gpuDecode=None,
             minMapQ=0, requireFlags=0, excludeFlags=0, anyOrder=False, fragments=False):
    """The ``coverage`` command: one decode, ``<outputPath>.bedgraph`` -- or, ``isStranded`` with ``strandedType`` ``fr`` / ``rf``,
    ``<outputPath>.plus.bedgraph`` and ``<outputPath>.minus.bedgraph`` -- with the chromosomes in header order (``qChrom``: that one)
    and no track line.  ``perMillion``: values per million mapped reads (the decode counts them: ``DecodeOptions(flagstat=True)``; a
    source without those counters is an error).  With several devices the file is decoded and covered on the first: there are no
    shares.  ``fragments``: a pair of mates covers the union of its reads' blocks once (the module's text); not with ``perMillion``.
    -> {file path: number of runs written}."""
    log = _process.logger(log)
    if fragments and perMillion:
        raise ValueError("coverage: --perMillion --fragments is refused: no fragment library size is counted, and fragment depth per million mapped READS would mislead")
    stranded = _process.stranded_code("coverage", isStranded, strandedType)
    devices = _process.one_device(devices, log, "coverage: the alignment file is decoded and covered")
    options = _process.DecodeOptions(_process.read_filter(minMapQ, requireFlags, excludeFlags), flagstat=bool(perMillion), any_order=bool(anyOrder), mate_keys=bool(fragments))
    tracks = tracks_of(stranded)
    mates = {} if fragments else None
    pair_sums = np.zeros(2 + len(tracks), np.int64)      # --fragments: pairable reads, pairs found, pairs whose union was taken per track
    paths = [outputPath + suffix for suffix, _ in tracks]
    written = dict.fromkeys(paths, 0)
    held = []          # --perMillion: (chrom, runs per track) until the library size is known
    sums = np.zeros((len(tracks), 5), np.int64)
    with _process.decoding(inBAM, devices, gpuDecode, threads, options, log=log) as source:
        _process.wait_decoded(source, anyOrder, log)
        for path in paths:
            open(path, "w").close()
        for chrom, length, per_track in runs_of_source(source, devices[0], _process.chroms_of(source, qChrom), stranded, fragments=bool(fragments), mates=mates):
            if fragments:
                taken = [int(t[3]["pairs"]) for t in per_track]
                log("  %s: %d pairable reads, %d pairs found, %s" % (chrom, mates[chrom]["pairable"], mates[chrom]["paired"] // 2, union_text(tracks, taken)))
                pair_sums += [mates[chrom]["pairable"], mates[chrom]["paired"] // 2] + taken
            for k, (start, end, depth, totals) in enumerate(per_track):
                name = "%s (%s)" % (chrom, tracks[k][1]) if stranded else chrom
                log("  %s: %d runs, %d covered bases" % (name, totals["runs"], totals["covered_bases"]))
                if totals["past_end"]:
                    log("  %d reads ran past the end of %s (%d bases)" % (totals["past_end"], name, length))
                sums[k] += [totals[key] for key in native.COVERAGE_TOTALS]          # (the first five, per read and per fragment)
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
        if fragments:
            log("Mates: %d pairable reads, %d pairs found, %s" % (pair_sums[0], pair_sums[1], union_text(tracks, pair_sums[2:].tolist())))
        _process.log_filter(source, options.read_filter, log)
    for k, path in enumerate(paths):
        log("%s: %d runs, %d covered bases, %d %sof %d reads contributed%s" % (path, sums[k][0], sums[k][4], sums[k][2], "fragments and single reads " if fragments else "", sums[k][1],
                                                                          ", %d ran past the end of their reference" % sums[k][3] if sums[k][3] else ""))
    return written
