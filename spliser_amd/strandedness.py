"""``strandedness`` / ``-s auto`` -- whether the library is unstranded, ``fr`` or ``rf``, inferred from the BAM itself on the GPU.

Not part of SpliSER v0.1.8: its README has the user open the BAM in IGV, colour the reads by first-in-pair and compare them with a
junction ("a common place to trip up" -- a wrong answer does not fail, it gives no beta1 counts, or half the sites without a gene).
Here the decode leaves what answers the question on the device: FLAG gives the read's strand under ``fr`` (``check_strand``), the
XS:A tag of a spliced read (``spl_bam_set_aux_strand``) and the strand of the genes the read lies in (``-A``) say what strand its
transcript has, and ``spl_strand_tally`` counts the one against the others (the rule: include/spliser.h, csrc/spl_strand_rule.h).

The decision is a stated policy, not a measurement, in integers: per source (tags, annotation), with ``a`` reads agreeing under
``fr``, ``b`` disagreeing and ``n = a + b``: fewer than ``minEvidence`` (default 1000) -> ``none``; ``10 a >= 9 n`` -> ``fr``;
``10 a <= n`` -> ``rf``; ``4 n <= 10 a <= 6 n`` -> ``unstranded``; anything else ``undetermined``.  The verdict is the common
verdict of the sources that are not ``none``.  Parity with RSeQC's ``infer_experiment.py`` is unpinned (it is not on the build
machine): the yardstick is this statement of the rule.
"""
import threading

import numpy as np

from . import native, process as _process, readsets, shard

MIN_EVIDENCE = 1000
SOURCES = (("tags", 2), ("annotation", 8))      # name, first counter
MATES = ("unpaired", "first", "second")
TOO_LITTLE = "undetermined (too little evidence)"
DISAGREE = "undetermined (tags and annotation disagree)"


class Undetermined(RuntimeError):
    """``-s auto`` could not tell; ``report`` is the text of the tally."""

    def __init__(self, message, report):
        RuntimeError.__init__(self, message)
        self.report = report


def cover_map(left, right, strand):
    """The strand cover map of one chromosome from its genes (``GeneBins.gene_arrays``: left = GFF column 4 - 1, right = column 5,
    strand byte): a gene covers the 1-based positions left + 1 .. right; genes whose strand is neither ``+`` nor ``-`` are ignored.
    -> (start int32, code uint8), ascending; code[k] holds from start[k] to start[k + 1] - 1 (the last to the end): 0 no gene,
    1 only ``+`` genes, 2 only ``-`` genes, 3 both; an entry only where the code changes, 0 below start[0]."""
    left, right, strand = np.asarray(left, np.int64), np.asarray(right, np.int64), np.asarray(strand, np.uint8)
    keep = ((strand == 43) | (strand == 45)) & (right > left)
    left, right, minus = left[keep], right[keep], strand[keep] == 45
    if not left.shape[0]:
        return np.zeros(0, np.int32), np.zeros(0, np.uint8)
    at = np.concatenate((left + 1, right + 1))                        # a gene's first position, and the first one behind it
    step = np.concatenate((np.ones(left.shape[0], np.int64), -np.ones(left.shape[0], np.int64)))
    is_minus = np.concatenate((minus, minus))
    points = np.unique(at)
    slot = np.searchsorted(points, at)
    depth = np.zeros((2, points.shape[0]), np.int64)
    np.add.at(depth[0], slot[~is_minus], step[~is_minus])
    np.add.at(depth[1], slot[is_minus], step[is_minus])
    depth = np.cumsum(depth, axis=1)
    code = ((depth[0] > 0).astype(np.uint8) | ((depth[1] > 0).astype(np.uint8) << 1))
    change = np.ones(points.shape[0], bool)
    change[1:] = code[1:] != code[:-1]
    change[0] = code[0] != 0
    if points[change].shape[0] and points[change].max() > shard.COORD_MAX:
        raise native.SpliserNativeError(-6, "a gene ends beyond the int32 coordinate space")
    return points[change].astype(np.int32), code[change]


def covers_of(bins, chroms):
    """{chrom: cover map} of the chromosomes of ``chroms`` that have a gene with a strand."""
    out = {}
    for chrom in chroms:
        left, right, strand, _ = bins.gene_arrays(chrom)
        start, code = cover_map(left, right, strand)
        if start.shape[0]:
            out[chrom] = (start, code)
    return out


def tally_of_source(source, devices, chroms, covers=None, spliced=None):
    """``spl_strand_tally`` over every chromosome of ``chroms``, from an alignment source whose decode has been started with
    ``aux_strand`` (``process.open_and_decode``) -> int64[14], the sums.  On the plan of ``readsets.over_fused_sets``: the tally adds
    over reads, so after a decode in shares every device tallies its piece and the host adds the 14 numbers; reads on the host go
    up with their strand bytes.  ``covers``: {chrom: (start, code)} (``covers_of``) or None.
    ``spliced``: a list whose entry 0 gets the junction-carrying reads of the sets WITHOUT any tag evidence added (what the hint
    about the aligner's options needs)."""
    if not getattr(source, "aux_strand", False):
        raise ValueError("strandedness: the alignment source was opened without aux_strand")
    covers = covers or {}
    total, lock = np.zeros(14, np.int64), threading.Lock()

    def tally(dr, chrom):
        t = dr.strand_tally(covers.get(chrom))
        n_spliced = 0
        if spliced is not None and not t[2:8].any():
            n_spliced = int(dr.junctions(0)["count"].sum())
        with lock:
            total[:] += t
            if spliced is not None:
                spliced[0] += n_spliced

    readsets.over_fused_sets(source, devices, chroms, tally, with_strand=True)
    return total


def source_counts(tally, first):
    """-> (a, b): the reads of one source (``first`` = its first counter) that agree with fr, and that do not."""
    return int(tally[first]) + int(tally[first + 2]) + int(tally[first + 4]), int(tally[first + 1]) + int(tally[first + 3]) + int(tally[first + 5])


def source_verdict(a, b, min_evidence=MIN_EVIDENCE):
    n = a + b
    if n < min_evidence:
        return "none"
    if 10 * a >= 9 * n:
        return "fr"
    if 10 * a <= n:
        return "rf"
    if 4 * n <= 10 * a <= 6 * n:
        return "unstranded"
    return "undetermined"


def decide(tally, min_evidence=MIN_EVIDENCE):
    """-> (verdict, {source: its verdict}): ``fr``, ``rf``, ``unstranded``, ``undetermined`` or one of the two longer texts."""
    per = {name: source_verdict(*source_counts(tally, first), min_evidence=min_evidence) for name, first in SOURCES}
    said = [v for v in per.values() if v != "none"]
    if not said:
        return TOO_LITTLE, per
    if len(set(said)) > 1:
        return DISAGREE, per
    return said[0], per


XS_HINT = "no spliced read carries XS:A:+/-: was the file aligned with STAR --outSAMstrandField intronMotif, HISAT2 or TopHat?"


def report(tally, min_evidence=MIN_EVIDENCE, spliced_untagged=0):
    """The tab-separated text of a tally: reads seen, reads eligible, per source four lines source / mate / agree_fr / agree_rf
    (the ``all`` line with the fraction and the source's verdict), a note when no spliced read carries the tag, the verdict last."""
    verdict, per = decide(tally, min_evidence)
    lines = ["reads seen\t%d" % int(tally[0]), "reads eligible\t%d" % int(tally[1])]
    for name, first in SOURCES:
        for m, mate in enumerate(MATES):
            lines.append("%s\t%s\t%d\t%d" % (name, mate, int(tally[first + 2 * m]), int(tally[first + 2 * m + 1])))
        a, b = source_counts(tally, first)
        lines.append("%s\tall\t%d\t%d\t%s\t%s" % (name, a, b, "%.4f" % (a / float(a + b)) if a + b else "NA", per[name]))
    if source_counts(tally, 2) == (0, 0) and spliced_untagged > 0:
        lines.append("note\t%s" % XS_HINT)
    lines.append("verdict\t%s" % verdict)
    return "\n".join(lines) + "\n"


def infer(source, devices, bins=None, qChrom="All", minEvidence=MIN_EVIDENCE, log=None):
    """The whole inference on a source whose decode was started with ``aux_strand``: waits for the decode, tallies every chromosome
    (``qChrom``: that one) with the cover maps of ``bins`` when there are any -> (verdict, report text, tally).  Logs the report."""
    if isinstance(source, native.BamFile):
        source.wait_all()      # (every reference is complete at the end of the file, whatever its order)
    chroms = _process.chroms_of(source, qChrom)
    covers = covers_of(bins, chroms) if bins is not None else {}
    spliced = [0]
    tally = tally_of_source(source, tuple(devices), chroms, covers, spliced=spliced)
    text = report(tally, minEvidence, spliced[0])
    if log is not None:
        log("Strandedness of the library (%s):" % ("tags and annotation" if covers else "tags only"))
        for line in text.splitlines():
            log("  " + line)
    return decide(tally, minEvidence)[0], text, tally


def resolve_auto(source, devices, isStranded, bins, minEvidence, log, report_path=None):
    """``-s auto`` of ``process`` / ``junctions``: -> (isStranded, strandedType) as if the user had typed the verdict.  The report
    is logged, and written to ``report_path`` when given.  ``Undetermined``: no verdict, or ``unstranded`` where the user said
    ``--isStranded``."""
    verdict, text, _ = infer(source, devices, bins, "All", minEvidence, log)
    if report_path is not None:
        with open(report_path, "w") as fh:
            fh.write(text)
    if verdict in ("fr", "rf"):
        return True, verdict
    if verdict == "unstranded":
        if isStranded:
            raise Undetermined("--isStranded -s auto: the library looks unstranded\n" + text, text)
        return False, None
    raise Undetermined("-s auto: the strandedness of the library is %s; pass -s fr / -s rf, or neither for an unstranded library\n%s" % (verdict, text), text)


def strandedness(inBAM, annotationFile=None, aType="gene", qChrom="All", outputPath=None, minEvidence=MIN_EVIDENCE, devices=(0,), threads=0, log=None,
                 gpuDecode=None, minMapQ=0, requireFlags=0, excludeFlags=0, anyOrder=False):
    """The ``strandedness`` command: one decode with ``aux_strand``, the tally, the report -- logged, and written to ``outputPath``
    when given.  -> (verdict, tally).  Whatever the verdict, it is a result, not an error."""
    from . import sites
    log = _process.logger(log)
    if int(minEvidence) < 0:
        raise ValueError("minEvidence must not be negative")
    options = _process.DecodeOptions(_process.read_filter(minMapQ, requireFlags, excludeFlags), aux_strand=True, any_order=bool(anyOrder))
    with _process.decoding(inBAM, devices, gpuDecode, threads, options, log=log) as source:
        bins = sites.GeneBins.from_annotation(annotationFile, aType, "All", log=log) if annotationFile is not None else None
        if anyOrder:
            _process.log_any_order(source, log)
        verdict, text, tally = infer(source, devices, bins, qChrom, int(minEvidence), log)
        _process.log_filter(source, options.read_filter, log)
    if outputPath is not None:
        with open(outputPath, "w") as fh:
            fh.write(text)
    return verdict, tally
