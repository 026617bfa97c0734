"""``intronretention`` -- per annotated intron the depth of its measurable bases, the splice counts at its ends and the IR ratio, from
the decode of the alignment file: whether the intron behind a change in SSE is retained, without a sorted BAM and a second tool.

Not part of SpliSER v0.1.8.  Intron retention is the most common class of alternative splicing in plants; SSE sees it only through
alpha.  It has meant IRFinder or iREAD over the file this build has just decoded -- both want the sorted BAM ``--anyOrder`` exists to
spare.  After one decode everything is on the device: ``spl_intron_depth`` runs the coverage stages there, keeps the depth as
boundaries and takes an order statistic of it per intron (the rule: include/spliser.h, csrc/spl_intron_rule.h); the junction table
of the same reads gives the splice counts.

The rule.  Features, genes and selections are ``genecounts``' (``-t``, ``--idAttr``; stranded: the features that are not ``-`` are
measured on the ``+`` track, those that are not ``+`` on the ``-`` track).  Per selection, chromosome and gene the features are merged;
every gap between two consecutive merged intervals is an intron.  Its measurable pieces are the intron minus ALL features of the
selection, of any gene, clipped to the chromosome; over the ascending depths D of their L bases, with t = ``--trimPercent``:
``lo = L * t // 100``, ``hi = L - lo``, ``depth_n = hi - lo``, ``depth_sum = sum(D[lo:hi])``.  ``depth = depth_sum / depth_n``;
``IRratio = depth / (depth + max(splice_left, splice_right))``, the splice counts being the junctions that begin where the intron
begins, and end where it ends.  This is IRFinder's published measure -- a trimmed mean over max-side splicing -- as this project restates
it; parity with IRFinder is intended and unpinned (it is not on the build machine): the yardstick is tests/introncases.py.
Transcript-level introns, IRFinder's warnings column and known-exon blacklists are out of scope.

``--fragments`` takes both sides of the ratio per FRAGMENT, as IRFinder does.  Per read, a pair whose mates overlap inside an intron
adds two to its depth, and a pair whose mates both cross it adds two to its splice count: numerator and denominator are inflated by
different factors that depend on the library's insert size.  With the switch the depth is ``coverage --fragments``' (the union of
both mates' blocks, once: ``spl_intron_depth_fragments``) and the junction table is ``spl_junctions_fragments``': a junction whose
read has an earlier mate that supports the same junction adds nothing (csrc/spl_junctionfragment_rule.h).  Same file, same header.
``junctions`` and ``process`` have no such switch: the BED score feeds SpliSER's alpha, which stays per read beside beta1 / beta2.
"""
import timeit

import numpy as np

from . import coverage as _coverage, genecounts as _gc, native, process as _process, shard

SUFFIX = ".introns.tsv"
HEADER = ("id", "gene", "chrom", "start", "end", "strand", "measurable", "covered", "depth_n", "depth_sum", "depth", "splice_left", "splice_right", "splice_exact", "IRratio")
PLUS, MINUS = 43, 45


def tracks_of(stranded):
    """-> [(track text, strand argument of ``spl_intron_depth``)] of a run."""
    return [("+", "+"), ("-", "-")] if stranded else [(".", 0)]


def selection(left, right, strand, gene, track):
    """The features of a track, with a base: -> (left, right, gene) int64; a base below 0 is none."""
    left, right, strand, gene = np.asarray(left, np.int64), np.asarray(right, np.int64), np.asarray(strand, np.uint8), np.asarray(gene, np.int64)
    left = np.maximum(left, 0)
    keep = right > left
    if track == "+":
        keep &= strand != MINUS
    elif track == "-":
        keep &= strand != PLUS
    return left[keep], right[keep], gene[keep]


def introns_of(left, right, gene):
    """The introns of one selection on one chromosome: every gap between two consecutive merged intervals of a gene.  -> (gene, s, e)
    int64, sorted by (gene, s); 0-based, half-open."""
    empty = np.zeros(0, np.int64)
    if not left.shape[0]:
        return empty, empty, empty
    if int(right.max()) + 1 > shard.COORD_MAX:
        raise native.SpliserNativeError(-6, "a feature ends beyond the int32 coordinate space")
    m_left, m_right, m_gene = _gc.merged_per_gene(left, right, gene)
    same = m_gene[1:] == m_gene[:-1]
    return m_gene[:-1][same], m_right[:-1][same], m_left[1:][same]


def pieces_of(s, e, left, right, length=None):
    """The measurable pieces of the introns [s, e) of a selection whose features are (left, right): each intron minus the union of
    the features, clipped to [0, length) (None: not clipped).  -> (piece_off int64[n + 1], piece_start int32, piece_end int32)."""
    n = int(s.shape[0])
    if not n:
        return np.zeros(1, np.int64), np.zeros(0, np.int32), np.zeros(0, np.int32)
    u_left, u_right, _ = _gc.merged_per_gene(left, right, np.zeros(left.shape[0], np.int64))     # the union: disjoint, ascending
    first = np.searchsorted(u_right, s, "right")          # the first interval that ends beyond s
    last = np.searchsorted(u_left, e, "left")             # the first that begins at or beyond e
    count = last - first + 1                              # candidates: in front of, between and behind the intervals in reach
    off = np.concatenate(([0], np.cumsum(count)))
    owner = np.repeat(np.arange(n), count)
    j = np.arange(int(off[-1])) - off[owner]
    at = first[owner] + j
    a = np.where(j == 0, s[owner], u_right[np.maximum(at - 1, 0)])
    b = np.where(j == count[owner] - 1, e[owner], u_left[np.minimum(at, u_left.shape[0] - 1)])
    a, b = np.maximum(a, s[owner]), np.minimum(b, e[owner])
    if length is not None:
        b = np.minimum(b, int(length))
    keep = b > a
    piece_off = np.concatenate(([0], np.cumsum(np.bincount(owner[keep], minlength=n)))).astype(np.int64)
    return piece_off, a[keep].astype(np.int32), b[keep].astype(np.int32)


class Table(object):
    """The introns of an annotation under one strandedness, in the file's order: arrays ``gene`` (index into ``ids``), ``chrom``
    (index into ``chroms``, the annotation's order), ``s``, ``e`` (0-based, half-open), ``track`` (index into ``tracks``) and ``rank``
    (1-based within the gene: over the chromosomes in order, then start, end, track)."""

    def __init__(self, features, stranded=False):
        self.ids, self.chroms, self.tracks = features.ids, list(features.chroms), [t for t, _ in tracks_of(stranded)]
        self.features = features
        cols = [[], [], [], [], []]
        for c, chrom in enumerate(self.chroms):
            for t, track in enumerate(self.tracks):
                gene, s, e = introns_of(*selection(*features.arrays(chrom), track=track))
                for col, v in zip(cols, (gene, np.full(gene.shape[0], c, np.int64), s, e, np.full(gene.shape[0], t, np.int64))):
                    col.append(v)
        gene, chrom, s, e, track = [np.concatenate(col) if col else np.zeros(0, np.int64) for col in cols]
        order = np.lexsort((track, e, s, chrom, gene))
        self.gene, self.chrom, self.s, self.e, self.track = gene[order], chrom[order], s[order], e[order], track[order]
        n = self.gene.shape[0]
        begins = np.ones(n, bool)
        begins[1:] = self.gene[1:] != self.gene[:-1]
        at = np.flatnonzero(begins)
        self.rank = np.arange(n) - np.repeat(at, np.diff(np.concatenate((at, [n])))) + 1

    def rows_on(self, chrom, track):
        """Indices of the rows of one chromosome (its name) and track (its text), ascending."""
        if chrom not in self.chroms or track not in self.tracks:
            return np.zeros(0, np.int64)
        return np.flatnonzero((self.chrom == self.chroms.index(chrom)) & (self.track == self.tracks.index(track)))

    def pieces(self, rows, chrom, track, length=None):
        left, right, _ = selection(*self.features.arrays(chrom), track=track)
        return pieces_of(self.s[rows], self.e[rows], left, right, length)


def no_read_numbers(piece_off, piece_start, piece_end, trim):
    """What ``spl_intron_depth`` gives a set without a read: L, 0, depth_n, 0 per intron."""
    size = np.concatenate(([0], np.cumsum(piece_end.astype(np.int64) - piece_start.astype(np.int64))))
    total = size[piece_off[1:]] - size[piece_off[:-1]]
    out = np.zeros((total.shape[0], 4), np.int64)
    out[:, 0] = total
    out[:, 2] = total - 2 * ((total * int(trim)) // 100)
    return out


def splice_counts(junctions, s, e, track, stranded):
    """The junction table (``DeviceReads.junctions``' dict) joined to the introns [s, e): -> int64[n, 3], the counts of the junctions
    with left == s, with right == e, and with both.  Under a stranded run only rows of the intron's track count."""
    left, right, count = junctions["left"].astype(np.int64), junctions["right"].astype(np.int64), junctions["count"].astype(np.int64)
    if stranded:
        mine = junctions["strand"] == ord(track)
        left, right, count = left[mine], right[mine], count[mine]
    out = np.zeros((s.shape[0], 3), np.int64)
    for col, key, want in ((0, left, s), (1, right, e), (2, left * (1 << 32) + right, s * (1 << 32) + e)):
        order = np.argsort(key, kind="stable")
        key, sums = key[order], np.concatenate(([0], np.cumsum(count[order])))
        out[:, col] = sums[np.searchsorted(key, want, "right")] - sums[np.searchsorted(key, want, "left")]
    return out


def ratio_texts(depth_n, depth_sum, splice_left, splice_right):
    """-> (depth, IRratio) as the file has them."""
    if depth_n == 0:
        return "NA", "NA"
    depth = depth_sum / depth_n
    below = depth + max(splice_left, splice_right)
    return repr(depth), ("NA" if below == 0 else repr(depth / below))


def write_rows(path, table, rows, numbers, splices):
    """``rows``: indices into the table, in its order; ``numbers``: int64[len(rows), 4]; ``splices``: int64[len(rows), 3].  -> the
    number of rows written."""
    with open(path, "w") as fh:
        fh.write("\t".join(HEADER) + "\n")
        for k, r in enumerate(np.asarray(rows).tolist()):
            gene = table.ids[int(table.gene[r])]
            total, covered, depth_n, depth_sum = (int(v) for v in numbers[k])
            left, right, exact = (int(v) for v in splices[k])
            depth, ratio = ratio_texts(depth_n, depth_sum, left, right)
            fh.write("%s:I%03d\t%s\t%s\t%d\t%d\t%s\t%d\t%d\t%d\t%d\t%s\t%d\t%d\t%d\t%s\n" % (
                gene, int(table.rank[r]), gene, table.chroms[int(table.chrom[r])], int(table.s[r]) + 1, int(table.e[r]), table.tracks[int(table.track[r])], total, covered,
                depth_n, depth_sum, depth, left, right, exact, ratio))
    return len(rows)


def intronretention(inBAM, annotationFile, outputPath, aType="exon", idAttr="gene_id", trimPercent=30, qChrom="All", isStranded=False, strandedType=None, devices=(0,), threads=0,
                    log=None, gpuDecode=None, minMapQ=0, requireFlags=0, excludeFlags=0, anyOrder=False, fragments=False):
    """The ``intronretention`` command: one decode, the annotation read meanwhile, ``<outputPath>.introns.tsv``.  ``qChrom``: the rows
    of that chromosome, under the ids they have in the whole annotation.  With several devices the file is decoded and measured on
    the first: there are no shares.  ``fragments``: depth and splice counts per fragment (the module's text).  -> the number of rows
    written."""
    log = _process.logger(log)
    if annotationFile is None:
        raise ValueError("intronretention: an annotation file (-A) is required")
    stranded = _process.stranded_code("intronretention", isStranded, strandedType)
    trim = int(trimPercent)
    if not 0 <= trim <= 49:
        raise ValueError("intronretention: --trimPercent must be in 0..49")
    devices = _process.one_device(devices, log, "intronretention: the alignment file is decoded and measured")
    options = _process.DecodeOptions(_process.read_filter(minMapQ, requireFlags, excludeFlags), any_order=bool(anyOrder), mate_keys=bool(fragments))
    pair_sums = np.zeros(2, np.int64)      # --fragments: pairable reads, pairs found
    with _process.decoding(inBAM, devices, gpuDecode, threads, options, log=log) as source:
        t0 = timeit.default_timer()
        features = _gc.read_features(annotationFile, aType, idAttr)
        table = Table(features, bool(stranded))
        _gc.log_annotation(features, aType, t0, log, ", %d introns" % table.gene.shape[0])
        _process.wait_decoded(source, anyOrder, log)
        wanted = list(table.chroms) if qChrom == "All" else [c for c in table.chroms if c == qChrom]
        n = table.gene.shape[0]
        numbers, splices, done = np.zeros((n, 4), np.int64), np.zeros((n, 3), np.int64), set()
        visit = [c for c in source.ref_names if c in wanted]
        if fragments:
            log("  (--fragments: depth and splice counts are per fragment -- a base under both mates of a pair, and a junction both support, count once)")
        for chrom, length, dr in _coverage.sets_of_source(source, devices[0], visit, with_keys=bool(fragments)):
            junctions = dr.junctions(stranded, 0, 0, 0, fragments=bool(fragments))
            if fragments:
                mates = dr.mate_table(0)[1]
                log("  %s: %d pairable reads, %d pairs found" % (chrom, mates["pairable"], mates["paired"] // 2))
                pair_sums += [mates["pairable"], mates["paired"] // 2]
            for track, strand in tracks_of(stranded):
                rows = table.rows_on(chrom, track)
                piece_off, piece_start, piece_end = table.pieces(rows, chrom, track, length)
                got = dr.intron_depth(length, piece_off, piece_start, piece_end, trim, stranded, strand, fragments=bool(fragments))
                numbers[rows] = got
                splices[rows] = splice_counts(junctions, table.s[rows], table.e[rows], track, stranded)
                name = "%s (%s)" % (chrom, track) if stranded else chrom
                log("  %s: %d introns, %d measurable bases, %d introns without one" % (name, rows.shape[0], int(got[:, 0].sum()), int((got[:, 0] == 0).sum())))
                done.add((chrom, track))
        lengths = dict(zip(source.ref_names, source.ref_lengths)) if getattr(source, "ref_lengths", None) else {}
        for chrom in wanted:       # a chromosome the file lacks, or one without a read: the numbers no read gives
            for track, _ in tracks_of(stranded):
                if (chrom, track) in done:
                    continue
                rows = table.rows_on(chrom, track)
                length = int(lengths.get(chrom, 0))
                numbers[rows] = no_read_numbers(*table.pieces(rows, chrom, track, length if length >= 1 else None), trim=trim)
        if fragments:
            log("Mates: %d pairable reads, %d pairs found" % (pair_sums[0], pair_sums[1]))
        _process.log_filter(source, options.read_filter, log)
    keep = np.flatnonzero(np.isin(table.chrom, [table.chroms.index(c) for c in wanted]))
    path = outputPath + SUFFIX
    written = write_rows(path, table, keep, numbers[keep], splices[keep])
    log("%s: %d introns of %d genes" % (path, written, np.unique(table.gene[keep]).shape[0]))
    return written
