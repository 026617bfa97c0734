"""``duplicates`` -- how many of a library's fragments are PCR copies of another, from ONE decode, on the GPU.

Not part of SpliSER v0.1.8.  Every count it and this build report -- alpha, beta1, beta2, junction scores, gene counts -- is a count of
reads, and a low-input or over-amplified library inflates them with copies of one molecule: ``-r minReads`` then sees more evidence
than the library holds.  The usual remedy, Picard ``MarkDuplicates`` or ``samtools fixmate`` + ``samtools markdup`` in front of
``--excludeFlags 0x400``, wants a coordinate-sorted (and a name-sorted) copy of the file and rewrites it.  Here the reads are decoded
once, with their name keys; per chromosome the mates are paired (``spl_mate_table``), every fragment gets a signature of its unclipped
5' ends and orientations, the signatures are sorted and every fragment but one of a group is marked (``spl_reads_duplicates``; the rule
is ``csrc/spl_dup_rule.h``, restated in ``include/spliser.h`` and ``tests/dupcases.py``).  ``--dedup`` on ``junctions``, ``genecounts``
and ``saturation`` runs those commands on the reads that are not marked (``readsets.fused_set``).

Parity with Picard and samtools is intended and unpinned; the yardstick is ``tests/dupcases.py``.  Deliberate differences: the
representative of a group is chosen by name hash, not by base quality (no qualities are decoded); a pair split over two chromosomes
or by a decode filter is two single fragments; singles compete only with singles; secondary, supplementary, QC-failed and unmapped
records are never marked (add ``--excludeFlags 0x900``); no optical duplicates, no UMIs.  The same NAMES are marked whatever the
file's order or container -- for named reads.
"""
import threading

import numpy as np

from . import native, process as _process, readsets

HEADER = "chrom\treads\texamined\tpair_fragments\tsingle_fragments\tduplicate_pairs\tduplicate_singles\tduplicate_reads\tflagged_in_file\tfraction_duplicated\n"
HIST_HEADER = "group_size\tgroups\n"
SUFFIX, HIST_SUFFIX = ".duplicates.tsv", ".duplicates.hist.tsv"
BINS = native.DUP_HIST - 1


def duplicate_reads(counts):
    return 2 * int(counts[4]) + int(counts[5])


def row_text(chrom, counts):
    """One row of the table: ``counts`` int64[7] in ``native.DUP_COUNTS``' order."""
    examined, dup = int(counts[1]), duplicate_reads(counts)
    return "%s\t%s\t%d\t%d\t%s\n" % (chrom, "\t".join("%d" % int(v) for v in counts[:6]), dup, int(counts[6]), repr(dup / examined) if examined else "NA")


def counts_of_source(source, devices, chroms):
    """``spl_reads_duplicates`` over every chromosome of ``chroms`` -> ({chrom: int64[7]} for those with reads, int64[257] the
    histograms' sum).  The source was decoded with ``mate_keys`` and not in shares (an error otherwise)."""
    readsets.check_fragment_source(source)
    per_chrom, hist, lock = {}, np.zeros(native.DUP_HIST, np.int64), threading.Lock()

    def visit(dr, chrom):
        _, counts, h = dr.duplicates(0)
        with lock:
            per_chrom[chrom] = np.array([counts[k] for k in native.DUP_COUNTS], np.int64)
            hist[:] += h

    readsets.over_fused_sets(source, devices, chroms, visit, with_keys=True)
    return per_chrom, hist


def write_tables(outputPath, chroms, per_chrom, hist):
    total = np.zeros(len(native.DUP_COUNTS), np.int64)
    with open(outputPath + SUFFIX, "w") as out:
        out.write(HEADER)
        for chrom in chroms:
            counts = per_chrom.get(chrom, np.zeros(len(native.DUP_COUNTS), np.int64))
            total += counts
            out.write(row_text(chrom, counts))
        out.write(row_text("total", total))
    with open(outputPath + HIST_SUFFIX, "w") as out:
        out.write(HIST_HEADER)
        for k in range(BINS):
            out.write("%s\t%d\n" % ("%d" % (k + 1) if k < BINS - 1 else "%d+" % BINS, int(hist[k])))
    return total


def duplicates(inBAM, outputPath, qChrom="All", anyOrder=False, gpuDecode=None, devices=(0,), threads=0, log=None, minMapQ=0, requireFlags=0, excludeFlags=0):
    """Writes ``<outputPath>.duplicates.tsv`` -- a row per visited chromosome in header order, zeros included, then ``total`` -- and
    ``<outputPath>.duplicates.hist.tsv`` -- the groups of 1 .. 255 and of 256 or more fragments over all visited chromosomes -- and
    returns the total's seven counters (``native.DUP_COUNTS``)."""
    log = _process.logger(log)
    devices = _process.one_device(devices, log, "duplicates: the alignment file is decoded and marked")
    options = _process.DecodeOptions(_process.read_filter(minMapQ, requireFlags, excludeFlags), any_order=bool(anyOrder), mate_keys=True)
    with _process.decoding(inBAM, devices, gpuDecode, threads, options, log=log) as source:
        _process.wait_decoded(source, anyOrder, log)
        if isinstance(source, native.BamFile) and not source.wait_all():
            raise native.SpliserNativeError(-5, "%s is not sorted by reference: sort it (samtools sort) first, or pass --anyOrder" % inBAM)
        chroms = _process.chroms_of(source, qChrom)
        per_chrom, hist = counts_of_source(source, devices, chroms)
        _process.log_filter(source, options.read_filter, log)
    total = write_tables(outputPath, chroms, per_chrom, hist)
    for chrom in chroms:
        if chrom in per_chrom:
            c = per_chrom[chrom]
            log("  %s: %d reads, %d examined, %d pair and %d single fragments, %d duplicate reads" % (chrom, int(c[0]), int(c[1]), int(c[2]), int(c[3]), duplicate_reads(c)))
    if int(hist[BINS]):
        log("  (%d fragments in groups of %d or more)" % (int(hist[BINS]), BINS))
    examined, dup = int(total[1]), duplicate_reads(total)
    log("Duplicates: %d reads examined, %d duplicates (%s %%)" % (examined, dup, "%.2f" % (100.0 * dup / examined) if examined else "-"))
    return dict(zip(native.DUP_COUNTS, (int(v) for v in total)))
