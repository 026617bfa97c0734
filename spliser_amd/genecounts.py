"""``genecounts`` -- reads per gene, from the decode of the alignment file: the expression beside a change in SSE, without a second
pass over the BAM by another program.

Not part of SpliSER v0.1.8.  The diffSpliSER analysis is an edgeR analysis, and whoever reads a change in SSE wants the gene's
expression beside it, from the same session; that has meant ``htseq-count`` or ``featureCounts`` over the file this build has just
decoded -- minutes to hours of CPU, and ``htseq-count`` wants the sorted file ``--anyOrder`` exists to spare.  The decode leaves POS,
FLAG and CIGAR of every read on the device, and ``spl_gene_count`` assigns every read there (the rule: include/spliser.h,
csrc/spl_genecount_rule.h).  ``<out>.genecounts.tsv`` is htseq-count's two-column file, which ``edgeR::readDGE`` reads (it drops the
``__`` rows).

The rule.  A feature is a line of the GFF / GTF whose column 3 is ``-t`` (default ``exon``); its gene is the value of ``--idAttr``
(default ``gene_id``); a gene is all features with one id, wherever they lie.  A read counts when it is mapped, primary, QC-passed
and not supplementary, duplicates included; its aligned blocks (M, = and X; D and N are gaps) are held against the features: no
gene under any base -> ``__no_feature``, one gene -> that gene, more -> ``__ambiguous``; every other read -> ``__not_counted``.
With ``--isStranded -s fr|rf`` a read sees only the features of its strand (and those without one).  This is htseq-count's
``--mode union --nonunique none``, and featureCounts' default, applied per READ: a paired fragment adds up to two.  Parity with
htseq-count and featureCounts is intended and unpinned (neither is on the build machine): the yardstick is this statement of the rule,
restated in tests/genecases.py.

``--fragments`` counts a paired-end library as htseq-count and ``featureCounts -p --countReadPairs`` do, a FRAGMENT once.  The decode
then keeps a 64-bit key of every read's name (``mate_keys``), the mate table is built on the GPU per chromosome (``spl_mate_table``:
the pairable reads sorted by key, mates found by binary search) and ``spl_gene_count_fragments`` holds both mates' blocks against the
features, each mate on the map of its own strand: no gene -> ``__no_feature``, one -> that gene, more -> ``__ambiguous``.  A read is
pairable when it counts at all, is paired (0x1), is first or second in its pair (one of 0x40 / 0x80) and has a name; among the pairable
reads of one chromosome with one name the j-th first and the j-th second read are mates.  The rows then sum to reads minus pairs.
Deliberate differences from the tools: a pair split over two chromosomes, or with one mate filtered out (``--minMapQ``, the flag
filters), counts as two single-end fragments; names are compared by a 63-bit hash (two fragments of a chromosome may swap mates
where two names collide: about n^2 / 2^64 pairs for n names, 5e-6 for 10 M).  Parity with htseq-count and ``featureCounts -p`` is
intended and unpinned: the yardstick is tests/matecases.py.  With several devices the file is decoded and counted on the first
one: mates can lie either side of a share's cut.
"""
import threading
import timeit

import numpy as np

from . import native, process as _process, readsets
from .shard import COORD_MAX        # (the bound ``strandedness.cover_map`` enforces on a map's 1-based positions)

SUFFIX = ".genecounts.tsv"
MANY = native.GENE_MANY
SPECIALS = native.GENE_SPECIALS


class Features(object):
    """The features of an annotation: ``ids`` -- the gene ids, sorted, a gene's index is its place there --, ``chroms`` -- the
    chromosomes in the order they first appear --, and per chromosome four arrays ``(left int64, right int64, strand uint8, gene
    int64)``: 0-based half-open ``[column 4 - 1, column 5)``, the strand byte of column 7, the gene's index."""

    def __init__(self, ids, chroms, by_chrom):
        self.ids, self.chroms, self.by_chrom = ids, chroms, by_chrom

    def arrays(self, chrom):
        empty = np.zeros(0, np.int64)
        return self.by_chrom.get(chrom, (empty, empty, np.zeros(0, np.uint8), empty))

    def genes_on(self, chrom):
        """Sorted indices of the genes with a feature on ``chrom`` (features without a base included: they are features)."""
        return np.unique(self.arrays(chrom)[3])


def attribute(text, key):
    """The value of attribute ``key`` in column 9, GTF form ``key "value";`` or GFF3 form ``key=value;``, quotes stripped; None when
    it is not there."""
    for field in text.split(";"):
        field = field.strip()
        if not field.startswith(key):
            continue
        rest = field[len(key):]
        if rest[:1] == "=":
            value = rest[1:].strip()
        elif rest[:1] in (" ", "\t"):
            value = rest.strip()
        else:
            continue                    # (a longer key that begins alike: gene_id_version)
        if len(value) >= 2 and value[0] == value[-1] == '"':
            value = value[1:-1]
        return value
    return None


def read_features(path, aType="exon", idAttr="gene_id"):
    """The plain reader: every non-comment line with at least 9 columns whose column 3 equals ``aType``.  A line of the type
    without ``idAttr`` is an error that names the line number.  -> Features (features with ``right <= left`` are kept here and
    ignored by ``gene_maps``)."""
    rows, names = {}, {}
    with open(path) as fh:
        for number, line in enumerate(fh, 1):
            if line.startswith("#"):
                continue
            cols = line.rstrip("\r\n").split("\t")
            if len(cols) < 9 or cols[2] != aType:
                continue
            gene = attribute(cols[8], idAttr)
            if gene is None:
                raise native.SpliserNativeError(-5, "%s: line %d: a %s feature without the attribute %s" % (path, number, aType, idAttr))
            try:
                left, right = int(cols[3]) - 1, int(cols[4])
            except ValueError:
                raise native.SpliserNativeError(-5, "%s: line %d: columns 4 and 5 are not numbers" % (path, number))
            names.setdefault(gene, None)
            rows.setdefault(cols[0], []).append((left, right, ord(cols[6][0]) if cols[6] else 0, gene))
    ids = sorted(names)
    index = {g: k for k, g in enumerate(ids)}
    by_chrom = {}
    for chrom, r in rows.items():
        by_chrom[chrom] = (np.array([x[0] for x in r], np.int64), np.array([x[1] for x in r], np.int64), np.array([x[2] for x in r], np.uint8),
                           np.array([index[x[3]] for x in r], np.int64))
    return Features(ids, list(rows), by_chrom)


def merged_per_gene(left, right, gene):
    """Each gene's features (all with ``right > left``, int64 arrays, at least one) merged: overlapping or abutting exons of one gene
    are one interval.  -> (left, right, gene) of the merged intervals.  Sorted by (gene, left), a merged interval begins where left
    exceeds every right before it in the gene -- the running maximum is kept per gene by lifting gene g's coordinates by g * big."""
    order = np.lexsort((left, gene))
    left, right, gene = left[order], right[order], gene[order]
    low = min(int(left.min()), 0)
    big = int(right.max()) - low + 1
    reach = np.maximum.accumulate(gene * big + (right - low))
    first = np.ones(left.shape[0], bool)
    first[1:] = gene[1:] * big + (left[1:] - low) > reach[:-1]
    begins = np.flatnonzero(first)
    ends = np.concatenate((begins[1:], [left.shape[0]])) - 1
    return left[begins], reach[ends] - gene[ends] * big + low, gene[begins]


def gene_map(left, right, gene):
    """The gene map of one selection of features: -> (start int32, code uint32), ascending; code[k] holds for the 0-based positions
    start[k] <= p < start[k + 1] (the last to the end; 0 below start[0]): 0 no feature, g + 1 only gene g, ``MANY`` two genes or
    more; an entry only where the code changes.  A sweep: each gene's features are merged first (overlapping exons of one gene are
    one gene), then every merged interval is an event pair carrying +-1 and +-(g + 1); where the depth is 1 the running sum is the code."""
    left, right, gene = np.asarray(left, np.int64), np.asarray(right, np.int64), np.asarray(gene, np.int64)
    keep = right > left
    left, right, gene = left[keep], right[keep], gene[keep]
    if not left.shape[0]:
        return np.zeros(0, np.int32), np.zeros(0, np.uint32)
    if int(right.max()) + 1 > COORD_MAX:
        raise native.SpliserNativeError(-6, "a gene ends beyond the int32 coordinate space")
    m_left, m_right, m_gene = merged_per_gene(left, right, gene)
    at = np.concatenate((m_left, m_right))
    step = np.concatenate((np.ones(m_left.shape[0], np.int64), -np.ones(m_left.shape[0], np.int64)))
    points = np.unique(at)
    slot = np.searchsorted(points, at)
    depth, total = np.zeros(points.shape[0], np.int64), np.zeros(points.shape[0], np.int64)
    np.add.at(depth, slot, step)
    np.add.at(total, slot, step * (np.concatenate((m_gene, m_gene)) + 1))
    depth, total = np.cumsum(depth), np.cumsum(total)
    code = np.where(depth == 0, 0, np.where(depth == 1, total, MANY)).astype(np.uint32)
    change = np.ones(points.shape[0], bool)
    change[1:] = code[1:] != code[:-1]
    change[0] = code[0] != 0
    return points[change].astype(np.int32), code[change]


def gene_maps(left, right, strand, gene, stranded=False):
    """The gene maps of one chromosome's features: -> (map a, map b).  Unstranded: map a of all features, map b None.  Stranded: map a
    (the ``+`` reads') holds the features whose strand is not ``-``, map b those whose strand is not ``+``; a ``.`` is in both."""
    left, right, strand, gene = np.asarray(left, np.int64), np.asarray(right, np.int64), np.asarray(strand, np.uint8), np.asarray(gene, np.int64)
    if not stranded:
        return gene_map(left, right, gene), None
    plus, minus = strand != 45, strand != 43
    return gene_map(left[plus], right[plus], gene[plus]), gene_map(left[minus], right[minus], gene[minus])


def maps_of(features, chroms, stranded=False):
    """{chrom: (map a, map b)} of the chromosomes of ``chroms`` that have a feature."""
    out = {}
    for chrom in chroms:
        if chrom in features.by_chrom:
            out[chrom] = gene_maps(*features.arrays(chrom), stranded=bool(stranded))
    return out


def mate_row(dr):
    """-> the row a read set adds to ``mates``: reads, pairable reads, reads with a mate, pairable reads without one whose flag says
    the mate is mapped (``spl_mate_table``)."""
    stats = dr.mate_table(0)[1]
    return [dr.n, stats["pairable"], stats["paired"], stats["unpaired_mate_mapped"]]


def add_row(rows, chrom, row):
    """``rows[chrom] += row`` (int64[4]) where both are kept; under the caller's lock."""
    if rows is not None and row is not None:
        got = rows.setdefault(chrom, np.zeros(4, np.int64))
        got += row


def counts_of_source(source, devices, chroms, maps, n_genes, stranded=0, per_chrom=None, fragments=False, mates=None, dedup=False, removed=None):
    """``spl_gene_count`` over every chromosome of ``chroms`` -> int64[n_genes + 3], the sums: the genes' reads, then no feature,
    ambiguous, not counted.  On the plan of ``readsets.over_fused_sets``: counts add over reads, so the pieces of a decode in shares are
    counted where they lie and the host adds.  ``maps``: {chrom: (map a, map b)} (``maps_of``); a chromosome without one has no feature.
    ``per_chrom``: a dict that gets, per chromosome with reads, int64[4]: counted, no feature, ambiguous, not counted.
    ``fragments``: ``spl_gene_count_fragments`` -- a pair of mates counts once; the source was decoded with ``mate_keys`` and not in
    shares (an error otherwise).  ``mates``: a dict that then gets, per chromosome with reads, int64[4]: reads, pairable reads, reads
    with a mate, pairable reads without one whose flag says the mate is mapped.  ``dedup``: every set is counted without its
    duplicate fragments (``readsets.fused_set``: name keys and one device, as for ``fragments``); ``removed``: a list whose two entries
    get the reads removed and the reads they were removed from added."""
    n_genes = int(n_genes)
    total, lock = np.zeros(n_genes + 3, np.int64), threading.Lock()
    if fragments or dedup:
        readsets.check_fragment_source(source)

    def count(dr, chrom):
        a, b = maps.get(chrom, (None, None))
        t = dr.gene_counts(n_genes, a, b, stranded, fragments=fragments)
        row = mate_row(dr) if fragments and mates is not None else None
        verdicts = [int(t[:n_genes].sum()), int(t[n_genes]), int(t[n_genes + 1]), int(t[n_genes + 2])] if per_chrom is not None else None
        with lock:
            add_row(mates, chrom, row)
            total[:] += t
            add_row(per_chrom, chrom, verdicts)

    readsets.over_fused_sets(source, devices, chroms, count, with_keys=bool(fragments or dedup), dedup=bool(dedup), removed=removed)
    return total


def mates_line(row):
    """reads, pairable, paired, unpaired with a mapped mate -> the log's words."""
    reads, pairable, paired, lonely = (int(v) for v in row)
    return ("%d reads, %d pairable, %d pairs, %d pairable reads without a mate on their chromosome (%d of them with a mapped mate by their flag)"
            % (reads, pairable, paired // 2, pairable - paired, lonely))


def log_annotation(features, aType, t0, log, more=""):
    """The line a command says once its annotation is read (``more``: what the command made of it)."""
    log("Annotation: %d %s features of %d genes on %d chromosomes%s (read in %.3f s)" % (sum(v[0].shape[0] for v in features.by_chrom.values()), aType, len(features.ids),
                                                                                          len(features.chroms), more, timeit.default_timer() - t0))


def log_verdicts(chroms, per_chrom, mates, log):
    """Per chromosome with reads its verdict line -- and, ``mates`` not None (fragments were counted), its mates line, then their sum."""
    what = "reads" if mates is None else "fragments"
    for chrom in chroms:
        if chrom in per_chrom:
            log("  %s: %d %s counted, %d without a feature, %d ambiguous, %d not counted" % ((chrom, int(per_chrom[chrom][0]), what) + tuple(int(v) for v in per_chrom[chrom][1:])))
        if mates is not None and chrom in mates:
            log("  %s: %s" % (chrom, mates_line(mates[chrom])))
    if mates is not None:
        log("  mates: %s" % mates_line(sum(mates.values(), np.zeros(4, np.int64))))


def write_counts(path, ids, counts, only=None):
    """``id\\tcount\\n`` for every gene in the order of ``ids`` (``only``: just the genes with these indices), zeros included, then the
    three ``__`` rows.  -> the number of gene rows."""
    n = len(ids)
    rows = range(n) if only is None else [int(k) for k in only]
    with open(path, "w") as fh:
        for k in rows:
            fh.write("%s\t%d\n" % (ids[k], int(counts[k])))
        for k, name in enumerate(SPECIALS):
            fh.write("%s\t%d\n" % (name, int(counts[n + k])))
    return len(rows)


def genecounts(inBAM, annotationFile, outputPath, aType="exon", idAttr="gene_id", qChrom="All", isStranded=False, strandedType=None, devices=(0,), threads=0, log=None,
               gpuDecode=None, minMapQ=0, requireFlags=0, excludeFlags=0, anyOrder=False, fragments=False, dedup=False):
    """The ``genecounts`` command: one decode, the annotation read meanwhile, ``<outputPath>.genecounts.tsv``.  ``qChrom``: the reads
    of that chromosome, and the genes with a feature on it.  ``fragments``: a pair of mates counts once (the module's text); the
    file's format is the same.  ``dedup``: the reads that are no PCR duplicates are counted (``spl_reads_dedup``): what the command
    writes of a file from which the marked reads have been taken.  -> int64[n_genes + 3], the counts written."""
    log = _process.logger(log)
    if annotationFile is None:
        raise ValueError("genecounts: an annotation file (-A) is required")
    stranded = _process.stranded_code("genecounts", isStranded, strandedType)
    devices = (_process.one_device(devices, log, "%s: the alignment file is decoded and counted" % ("--fragments" if fragments else "--dedup")) if fragments or dedup
               else tuple(devices))
    options = _process.DecodeOptions(_process.read_filter(minMapQ, requireFlags, excludeFlags), any_order=bool(anyOrder), mate_keys=bool(fragments or dedup))
    with _process.decoding(inBAM, devices, gpuDecode, threads, options, log=log) as source:
        t0 = timeit.default_timer()
        features = read_features(annotationFile, aType, idAttr)
        n_genes = len(features.ids)
        log_annotation(features, aType, t0, log)
        _process.wait_decoded(source, anyOrder, log)
        chroms = _process.chroms_of(source, qChrom)
        maps = maps_of(features, chroms, stranded)
        per_chrom, mates = {}, ({} if fragments else None)
        n_removed = [0, 0]
        counts = counts_of_source(source, devices, chroms, maps, n_genes, stranded, per_chrom, fragments=bool(fragments), mates=mates, dedup=bool(dedup), removed=n_removed)
        log_verdicts(chroms, per_chrom, mates, log)
        if dedup:
            log("  (dedup: %d of %d reads removed as duplicates)" % (n_removed[0], n_removed[1]))
        _process.log_filter(source, options.read_filter, log)
    only = None if qChrom == "All" else features.genes_on(qChrom)
    path = outputPath + SUFFIX
    n_rows = write_counts(path, features.ids, counts, only)
    log("%s: %d genes, %d %s counted, %d without a feature, %d ambiguous, %d not counted" % (path, n_rows, int(counts[:n_genes].sum()), "fragments" if fragments else "reads",
                                                                                             int(counts[n_genes]), int(counts[n_genes + 1]), int(counts[n_genes + 2])))
    return counts
