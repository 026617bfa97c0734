"""``exoncounts`` -- reads per exon counting bin, from the decode of the alignment file: what ``edgeR::diffSpliceDGE`` and DEXSeq
need, without a second pass over the BAM by another program.

Not part of SpliSER v0.1.8.  Whoever looks at a change in splice-site strength also asks the standard question about exon usage,
from the same edgeR session; that has meant ``featureCounts -f -O`` or ``dexseq_count.py`` over the file this build has just
decoded -- the second an HTSeq loop in Python that takes hours on a human sample and wants the sorted file ``--anyOrder`` exists
to spare.  The decode leaves POS, FLAG and CIGAR of every read on the device, and ``spl_exon_count`` counts every read there (the
rule: include/spliser.h, csrc/spl_exoncount_rule.h).  ``<out>.exonbins.tsv`` names the bins, ``<out>.exoncounts.tsv`` holds their
reads, rows in the same order; in R: ``diffSpliceDGE(fit, geneid = bins$gene, exonid = bins$id)``.

The rule.  Features, genes and selections are ``genecounts``' (``-t``, ``--idAttr``, ``--isStranded -s fr|rf``).  A chromosome is
cut at every start and end of its features; a piece covered by features of exactly one gene is a BIN of that gene, a piece covered
by features of two genes or more is shared and no bin.  Two abutting exons of one gene are two bins, the same exon in two
transcripts is one.  A read that ``genecounts`` gives to a gene adds one to EVERY bin one of its aligned blocks overlaps (each bin
once, however many of its blocks lie in it); a read it calls ambiguous adds to no bin.  This is DEXSeq's counting
(``dexseq_count.py``) and ``featureCounts -f -O`` restricted to reads of one gene, applied per READ: a paired fragment adds up to
two per bin.  Parity with DEXSeq and featureCounts is intended and unpinned (neither is on the build machine): the yardstick is
this statement of the rule, restated in tests/exoncases.py.

``--countReadPairs`` (featureCounts' word; ``--fragments`` is ``genecounts``' spelling and is refused here) counts a paired-end
library as DEXSeq and ``featureCounts -f -O -p --countReadPairs`` do, a FRAGMENT once per bin.  Mates are ``genecounts
--fragments``': the decode keeps a 64-bit key of every read's name, the mate table is built on the GPU per chromosome
(``spl_mate_table``), and ``spl_exon_count_fragments`` holds both mates against the bins, each mate on the map of its own strand.
A read that is not eligible is not counted; an eligible read whose mate lies before it in the chromosome's reads is silent; every
other eligible read leads its fragment (or has no mate).  The verdict is taken over both mates' hit stretches together: a shared
piece under either, or bins of two genes, is ambiguous and NO bin moves; no bin at all is no feature; otherwise every DISTINCT bin
under either mate gets one -- a bin both mates overlap counts once, also when a stranded run showed it to them through different
maps (a ``.`` feature).  One read's bins ascend in bin number, so the kernel merges the two mates' walks and gives equal heads once;
nothing is stored per read.  The rows then sum to reads minus pairs, and a fragment's verdict is ``genecounts --fragments``' on the
same features.  The deliberate differences from the tools are that command's: a pair split over two chromosomes or by a filter
counts as two single-end fragments, and names are compared by a 63-bit hash.  Parity is intended and unpinned; the yardstick is
tests/exonfragcases.py.  With several devices the file is decoded and counted on the first one.
"""
import threading
import timeit

import numpy as np

from . import genecounts as _gc, native, process as _process, readsets, shard

BINS_SUFFIX, COUNTS_SUFFIX = ".exonbins.tsv", ".exoncounts.tsv"
SHARED = native.GENE_MANY
SPECIALS = native.EXON_SPECIALS


def _pieces(left, right, gene):
    """One selection's pieces: -> (cuts int64[m], kind int64[m - 1]) -- piece i is [cuts[i], cuts[i + 1]), its kind 0 (no feature),
    g + 1 (features of gene g only) or -1 (two genes or more).  Cuts are the features' own starts and ends; what covers a piece is
    read off each gene's MERGED features (``genecounts.merged_per_gene``): their depth is the number of genes."""
    keep = right > left
    left, right, gene = left[keep], right[keep], gene[keep]
    if not left.shape[0]:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    if int(right.max()) + 1 > shard.COORD_MAX:
        raise native.SpliserNativeError(-6, "a gene ends beyond the int32 coordinate space")
    cuts = np.unique(np.concatenate((left, right)))
    m_left, m_right, m_gene = _gc.merged_per_gene(left, right, gene)
    slot = np.searchsorted(cuts, np.concatenate((m_left, m_right)))      # (merged ends are features' ends: every one is a cut)
    step = np.concatenate((np.ones(m_left.shape[0], np.int64), -np.ones(m_left.shape[0], np.int64)))
    depth, total = np.zeros(cuts.shape[0], np.int64), np.zeros(cuts.shape[0], np.int64)
    np.add.at(depth, slot, step)
    np.add.at(total, slot, step * (np.concatenate((m_gene, m_gene)) + 1))
    depth, total = np.cumsum(depth)[:-1], np.cumsum(total)[:-1]
    return cuts, np.where(depth == 0, 0, np.where(depth == 1, total, -1))


def exon_maps(left, right, strand, gene, stranded=False):
    """The bin maps and the bins of one chromosome's features: -> (map a, map b or None, (bin gene, bin start, bin end)).  A map is
    ``(start int32, code uint32)`` in the shape of ``genecounts.gene_map``: 0 none, b + 1 bin b, ``SHARED``; an entry only where the
    code changes.  Unstranded: map a of all features.  Stranded: map a (the ``+`` reads') of the features whose strand is not ``-``,
    map b of those whose strand is not ``+``; a ``.`` is in both.  The bins -- int64 arrays, 0-based half-open -- are numbered in the
    order (start, end, gene) over the distinct triples of both maps."""
    left, right, strand, gene = np.asarray(left, np.int64), np.asarray(right, np.int64), np.asarray(strand, np.uint8), np.asarray(gene, np.int64)
    picks = [np.ones(left.shape[0], bool)] if not stranded else [strand != 45, strand != 43]
    pieces = [_pieces(left[w], right[w], gene[w]) for w in picks]
    triples = [np.stack((cuts[:-1][kind > 0], cuts[1:][kind > 0], kind[kind > 0] - 1), axis=1) for cuts, kind in pieces if cuts.shape[0]]
    triples = np.concatenate(triples) if triples else np.zeros((0, 3), np.int64)
    bins, number = np.unique(triples, axis=0, return_inverse=True) if triples.shape[0] else (triples, np.zeros(0, np.int64))
    number = np.asarray(number, np.int64).ravel()
    maps, used = [], 0
    for cuts, kind in pieces:
        if not cuts.shape[0]:
            maps.append((np.zeros(0, np.int32), np.zeros(0, np.uint32)))
            continue
        code = np.zeros(cuts.shape[0], np.int64)                    # (the last cut: nothing from there on)
        own = np.flatnonzero(kind > 0)
        code[own] = number[used:used + own.shape[0]] + 1
        used += own.shape[0]
        code[:-1][kind < 0] = SHARED
        change = np.ones(cuts.shape[0], bool)
        change[1:] = code[1:] != code[:-1]
        change[0] = code[0] != 0
        maps.append((cuts[change].astype(np.int32), code[change].astype(np.uint32)))
    return maps[0], (maps[1] if stranded else None), (bins[:, 2].copy(), bins[:, 0].copy(), bins[:, 1].copy())


class Bins(object):
    """The bins of an annotation.  ``by_chrom``: {chrom: (map a, map b, bin gene uint32[n_bins])} for ``spl_exon_count``; and the
    ROWS of both files, in their order -- gene ids sorted, then the bin's rank within its gene (over chromosomes in the annotation's
    order of first appearance, then start, end): ``gene`` (index into ``ids``), ``chrom`` (index into ``chroms``), ``start`` / ``end``
    (0-based half-open), ``local`` (the bin's number on its chromosome), ``rank`` (1-based)."""

    def __init__(self, features, stranded=False):
        self.ids, self.chroms, self.by_chrom = features.ids, features.chroms, {}
        cols = [[], [], [], [], []]
        for k, chrom in enumerate(features.chroms):
            a, b, (gene, start, end) = exon_maps(*features.arrays(chrom), stranded=bool(stranded))
            self.by_chrom[chrom] = (a, b, gene.astype(np.uint32))
            for col, v in zip(cols, (gene, np.full(gene.shape[0], k, np.int64), start, end, np.arange(gene.shape[0], dtype=np.int64))):
                col.append(v)
        gene, chrom, start, end, local = (np.concatenate(c) if c else np.zeros(0, np.int64) for c in cols)
        order = np.argsort(gene, kind="stable")      # (within a gene: chromosomes in turn, and a chromosome's bins ascend by start, end)
        self.gene, self.chrom, self.start, self.end, self.local = gene[order], chrom[order], start[order], end[order], local[order]
        first = np.searchsorted(self.gene, self.gene, side="left")
        self.rank = np.arange(self.gene.shape[0], dtype=np.int64) - first + 1

    @property
    def n(self):
        return int(self.gene.shape[0])

    def row_id(self, k):
        return "%s:%03d" % (self.ids[int(self.gene[k])], int(self.rank[k]))

    def rows_on(self, chrom):
        """The rows of the bins on ``chrom`` (None: every row), in the files' order."""
        if chrom is None:
            return np.arange(self.n)
        return np.flatnonzero(self.chrom == self.chroms.index(chrom)) if chrom in self.chroms else np.zeros(0, np.int64)


def counts_of_source(source, devices, chroms, bins, stranded=0, per_chrom=None, fragments=False, mates=None):
    """``spl_exon_count`` over every chromosome of ``chroms`` -> ({chrom: int64[n_bins] the bins' reads}, int64[4] the reads counted,
    without a feature, ambiguous, not counted), on the plan of ``readsets.over_fused_sets``.  A chromosome without a feature has
    no bin, and every eligible read on it is without a feature.  ``per_chrom``: a dict that gets, per chromosome with reads, its
    int64[4].  ``fragments``: ``spl_exon_count_fragments`` -- a pair of mates counts once per bin; the source was decoded with
    ``mate_keys`` and not in shares (an error otherwise).  ``mates``: a dict that then gets, per chromosome with reads, int64[4] as
    ``genecounts.counts_of_source`` fills it."""
    per_bin, total, lock = {}, np.zeros(4, np.int64), threading.Lock()
    nothing = (None, None, np.zeros(0, np.uint32))
    if fragments:
        readsets.check_fragment_source(source)

    def count(dr, chrom):
        a, b, bin_gene = bins.by_chrom.get(chrom, nothing)
        t = dr.exon_counts(bin_gene, a, b, stranded, fragments=fragments)
        row = _gc.mate_row(dr) if fragments and mates is not None else None
        n = bin_gene.shape[0]
        with lock:
            _gc.add_row(mates, chrom, row)
            if chrom in per_bin:
                per_bin[chrom] += t[:n]
            else:
                per_bin[chrom] = t[:n].copy()
            total[:] += t[n:]
            _gc.add_row(per_chrom, chrom, t[n:])

    readsets.over_fused_sets(source, devices, chroms, count, with_keys=bool(fragments))
    return per_bin, total


def row_counts(bins, per_bin, rows):
    """The reads of the rows ``rows``: a bin on a chromosome without a read has none."""
    out = np.zeros(len(rows), np.int64)
    for k, r in enumerate(rows):
        got = per_bin.get(bins.chroms[int(bins.chrom[r])])
        if got is not None:
            out[k] = got[int(bins.local[r])]
    return out


def write_bins(path, bins, rows):
    """``id gene chrom start end`` under a header, a row a bin; start and end 1-based inclusive, as the annotation's columns 4 and 5."""
    with open(path, "w") as fh:
        fh.write("id\tgene\tchrom\tstart\tend\n")
        for r in rows:
            fh.write("%s\t%s\t%s\t%d\t%d\n" % (bins.row_id(r), bins.ids[int(bins.gene[r])], bins.chroms[int(bins.chrom[r])], int(bins.start[r]) + 1, int(bins.end[r])))
    return len(rows)


def write_counts(path, bins, rows, counts, verdicts):
    """``id\\tcount\\n`` for the rows, zeros included, then the three ``__`` rows (``verdicts``: counted, no feature, ambiguous, not
    counted).  No header, as in ``genecounts``."""
    with open(path, "w") as fh:
        for r, c in zip(rows, counts):
            fh.write("%s\t%d\n" % (bins.row_id(r), int(c)))
        for k, name in enumerate(SPECIALS):
            fh.write("%s\t%d\n" % (name, int(verdicts[k + 1])))
    return len(rows)


def exoncounts(inBAM, annotationFile, outputPath, aType="exon", idAttr="gene_id", qChrom="All", isStranded=False, strandedType=None, devices=(0,), threads=0, log=None,
               gpuDecode=None, minMapQ=0, requireFlags=0, excludeFlags=0, anyOrder=False, countReadPairs=False):
    """The ``exoncounts`` command: one decode, the annotation read and cut into bins meanwhile, ``<outputPath>.exonbins.tsv`` and
    ``<outputPath>.exoncounts.tsv``.  ``qChrom``: the reads of that chromosome, and the bins on it, under the ids they have in the
    whole annotation.  ``countReadPairs``: a pair of mates counts once per bin (the module's text); the files' format is the same.
    -> (the rows' counts, int64[4]: counted, no feature, ambiguous, not counted)."""
    log = _process.logger(log)
    if annotationFile is None:
        raise ValueError("exoncounts: an annotation file (-A) is required")
    stranded = _process.stranded_code("exoncounts", isStranded, strandedType)
    devices = _process.one_device(devices, log, "--countReadPairs: the alignment file is decoded and counted") if countReadPairs else tuple(devices)
    options = _process.DecodeOptions(_process.read_filter(minMapQ, requireFlags, excludeFlags), any_order=bool(anyOrder), mate_keys=bool(countReadPairs))
    with _process.decoding(inBAM, devices, gpuDecode, threads, options, log=log) as source:
        t0 = timeit.default_timer()
        features = _gc.read_features(annotationFile, aType, idAttr)
        bins = Bins(features, stranded)
        _gc.log_annotation(features, aType, t0, log)
        log("Bins: %d exon counting bins" % bins.n)
        _process.wait_decoded(source, anyOrder, log)
        chroms = _process.chroms_of(source, qChrom)
        per_chrom, mates = {}, ({} if countReadPairs else None)
        per_bin, verdicts = counts_of_source(source, devices, chroms, bins, stranded, per_chrom, fragments=bool(countReadPairs), mates=mates)
        _gc.log_verdicts(chroms, per_chrom, mates, log)
        _process.log_filter(source, options.read_filter, log)
    rows = bins.rows_on(None if qChrom == "All" else qChrom)
    counts = row_counts(bins, per_bin, rows)
    write_bins(outputPath + BINS_SUFFIX, bins, rows)
    write_counts(outputPath + COUNTS_SUFFIX, bins, rows, counts, verdicts)
    log("%s: %d bins, %d %s counted, %d without a feature, %d ambiguous, %d not counted" % ((outputPath + COUNTS_SUFFIX, len(rows), int(verdicts[0]), "fragments" if countReadPairs else "reads")
                                                                                           + tuple(int(v) for v in verdicts[1:])))
    return counts, verdicts
