"""``junctions`` -- the BED12 junction file ``process`` takes with ``-b``, derived from the BAM itself on the GPU.

Not part of SpliSER v0.1.8: its README (README.md:41) sends the user to ``regtools junctions extract`` for this file.  The
table comes from ``spl_junctions`` (one insert per N op into a device hash table, see spl_kernels.hip); the line layout is
the one findAlphaCounts reads (SpliSER_v0_1_8.py:259-277): ``leftpos = chromStart + blockSizes[0]``, ``rightpos =
chromEnd - blockSizes[1]``, ``alpha = score``, strand in column 6.  Defaults of the policy knobs are regtools' (-a 8 -m 70
-M 500000); strand is the read strand by check_strand's rule for a stranded library and ``?`` otherwise -- or, with
``strandFromXS`` (regtools' ``-s XS``, its mode for unstranded libraries), the value of the XS:A tag the aligner wrote on the read
(STAR --outSAMstrandField intronMotif, HISAT2, TopHat): the decode leaves a strand byte per spliced read (``spl_bam_set_aux_strand``)
and ``spl_junctions`` keys its table by it (mode 3), so that a junction carried by ``+``-tagged, ``-``-tagged and untagged reads
is three lines.  An XS of another type (BWA's XS:i) or another value counts as no tag: ``?``.
"""
import threading

import numpy as np

from . import native, process as _process, readsets


def write_junction_bed(handle, chrom, table, first_number=1):
    n = len(table["left"])
    left, right = table["left"].tolist(), table["right"].tolist()
    strand, count = table["strand"].tolist(), table["count"].tolist()
    a_left, a_right = table["anchor_left"].tolist(), table["anchor_right"].tolist()
    for i in range(n):
        start, end = left[i] - a_left[i], right[i] + a_right[i]
        handle.write("%s\t%d\t%d\tJUNC%08d\t%d\t%s\t%d\t%d\t255,0,0\t2\t%d,%d\t0,%d\n" % (
            chrom, start, end, first_number + i, count[i], chr(strand[i]), start, end, a_left[i], a_right[i], end - start - a_right[i]))
    return n


def track_line(minAnchor, minIntron, maxIntron):
    return 'track name=junctions description="spliser_amd junctions (a>=%d, %d<=intron<=%d)"\n' % (minAnchor, minIntron, maxIntron)


def write_bed_file(path, chroms, tables, minAnchor, minIntron, maxIntron, log=None):
    """The BED12 file of ``junctions``: the track line, then every chromosome of ``chroms`` that has a table, numbered through.
    ``tables``: {chrom: table} (dicts of arrays as ``DeviceReads.junctions`` returns them).  -> the number of lines."""
    total = 0
    with open(path, "w") as out:
        out.write(track_line(minAnchor, minIntron, maxIntron))
        for chrom in chroms:
            if chrom not in tables:
                continue
            n = write_junction_bed(out, chrom, tables[chrom], total + 1)
            if log is not None:
                log(chrom, n)
            total += n
    return total


_COLUMNS = (("left", np.int32), ("right", np.int32), ("strand", np.uint8), ("count", np.uint32), ("anchor_left", np.uint32), ("anchor_right", np.uint32))


def merge_tables(parts):
    """Junction tables of disjoint pieces of one chromosome's reads (the shares of a decode in shares) -> the table of all of
    them: by key (left, right, strand) the counts added, the anchors the maximum; sorted like every table, by the signed left,
    then right, then strand."""
    if len(parts) == 1:
        return parts[0]
    cat = {k: np.concatenate([np.asarray(t[k]) for t in parts]) for k, _ in _COLUMNS}
    order = np.lexsort((cat["strand"], cat["right"], cat["left"]))
    cat = {k: v[order] for k, v in cat.items()}
    n = order.shape[0]
    head = np.ones(n, bool)
    head[1:] = (cat["left"][1:] != cat["left"][:-1]) | (cat["right"][1:] != cat["right"][:-1]) | (cat["strand"][1:] != cat["strand"][:-1])
    starts = np.flatnonzero(head)
    out = {k: cat[k][starts] for k in ("left", "right", "strand")}
    if n:
        out["count"] = np.add.reduceat(cat["count"].astype(np.int64), starts).astype(np.uint32)
        out["anchor_left"] = np.maximum.reduceat(cat["anchor_left"], starts)
        out["anchor_right"] = np.maximum.reduceat(cat["anchor_right"], starts)
    else:
        out.update({k: cat[k] for k in ("count", "anchor_left", "anchor_right")})
    return {k: out[k].astype(dt) for k, dt in _COLUMNS}


def log_xs_tally(tally, log):
    """What a user of ``strandFromXS`` needs to learn first: whether the aligner wrote the tag at all."""
    log("  (strand from XS: junction-supporting reads tagged +: %d, tagged -: %d, without a usable XS:A tag: %d)" % tuple(tally))
    if tally[0] + tally[1] == 0 and tally[2]:
        log("  (no spliced read carries XS:A:+/-: was the file aligned with STAR --outSAMstrandField intronMotif, HISAT2 or TopHat?)")


MOTIF_NAMES = ("GT/AG", "CT/AC", "GC/AG", "CT/GC", "AT/AC", "GT/AT")


class GenomeOnDevices(object):
    """``--genome``: the FASTA as base codes on every device that builds junction tables -- each loads its own copy, once per
    command (``native.Genome``) --, what ``--strandFromMotif`` adds up over the read sets (``tally``, ``native.MOTIF_TALLY``), and
    the check that the FASTA is the genome the reads were aligned to.  ``close()`` when the command is done with it."""

    def __init__(self, path):
        self.path = path
        self.tally = np.zeros(12, np.int64)
        self._genomes, self._locks, self._lock = {}, {}, threading.Lock()

    def on(self, ctx):
        """The device's copy, loaded by the first context of that device that asks; the devices load side by side."""
        with self._lock:
            of_device = self._locks.setdefault(ctx.device, threading.Lock())
        with of_device:
            if ctx.device not in self._genomes:
                self._genomes[ctx.device] = native.Genome(ctx, self.path).detach()
            return self._genomes[ctx.device]

    def sequence(self, genome, source, chrom):
        """The FASTA's sequence of a chromosome a command visits -> its index; an error names a chromosome that is missing or whose
        length is not the alignment header's."""
        if chrom not in genome:
            raise native.SpliserNativeError(-5, "%s is in the alignment and not in the FASTA %s: is this the genome the reads were aligned to?" % (chrom, self.path))
        lengths = getattr(source, "ref_lengths", None)
        if lengths:
            want = dict(zip(source.ref_names, lengths)).get(chrom)
            if want is not None and want > 0 and want != genome.length(chrom):
                raise native.SpliserNativeError(-5, "%s is %d in the alignment and %d in the FASTA: is this the genome the reads were aligned to?"
                                                % (chrom, want, genome.length(chrom)))
        return genome.index(chrom)

    def add(self, tally):
        with self._lock:
            self.tally += tally

    def close(self):
        for g in self._genomes.values():
            g.free()
        self._genomes = {}


def log_motif_tally(tally, log):
    t = [int(v) for v in tally]
    log("  (strand from motif: reads +: %d, -: %d, conflicting: %d, spliced without a canonical motif: %d; junction walks %s, other: %d)"
        % (t[7], t[8], t[9], t[10], ", ".join("%s: %d" % (n, t[1 + k]) for k, n in enumerate(MOTIF_NAMES)), t[0]))
    if t[11]:
        log("  (%d reads have a junction beyond the ends of their FASTA sequence)" % t[11])


def drop_noncanonical(tables, chroms, genome, source, devices, log):
    """``--canonicalOnly``: the rows of every chromosome's merged table whose motif code is 0 go (``spl_junction_motifs``), before
    the BED is written and before the site table is made -> the tables that remain."""
    out, gone, gone_reads = {}, 0, 0
    with native.Context(devices[0]) as ctx:
        g = genome.on(ctx)
        for chrom in chroms:
            if chrom not in tables:
                continue
            t = tables[chrom]
            code = g.junction_motifs(genome.sequence(g, source, chrom), t["left"], t["right"], ctx=ctx) if len(t["left"]) else np.zeros(0, np.uint8)
            keep = code != 0
            n, reads = int((~keep).sum()), int(t["count"][~keep].sum())
            if n:
                log("%s: %d junctions without a canonical motif dropped (%d supporting reads)" % (chrom, n, reads))
            gone, gone_reads = gone + n, gone_reads + reads
            out[chrom] = {k: v[keep] for k, v in t.items()}
    log("Junctions without a canonical motif dropped:\t%d (%d supporting reads)" % (gone, gone_reads))
    return out


def tables_of_source(source, devices, chroms, stranded, minAnchor, minIntron, maxIntron, tally=None, motif=None, subsample=None, kept=None, dedup=False, removed=None):
    """The junction table of every chromosome of ``chroms`` that has reads, from an alignment source whose decode has been
    started (``process.open_and_decode``): -> {chrom: (reads, table)}.  On the plan of ``readsets``: after a decode on the device
    the read sets are fused and stay so (``spl_junctions`` reads the arrays; nothing is laid out, nothing decoded again by whoever
    counts the same reads afterwards); after a decode in shares every device takes the table of ITS piece of a chromosome, and the
    pieces are merged here (``merge_tables``).  Reads on the host -- a file the host's threads decode, SAM text -- are this
    function's own case: they go to the first device unfused (``add_bam`` / ``add``), chromosome by chromosome AS THEY BECOME COMPLETE,
    not after the whole file (``process`` without ``-b`` counts on behind them).  ``stranded`` = ``native.STRAND_FROM_XS``: the source
    must have been opened with ``aux_strand`` -- the device decode's sets have the strand bytes, reads on the host go up with theirs
    as arrays, by the plan (``spl_soa_upload3``: that mode is the fused kernel's).  ``tally``: a list whose three entries get the
    junction-supporting reads by strand (+, -, ?) added: the sums of the tables' counts.  ``motif`` (a ``GenomeOnDevices``, with
    ``native.STRAND_FROM_XS``): every fused set's strand bytes are written over by the genome's splice motifs before its table is
    made (``spl_reads_motif_strand``) -- the decode's XS walk has left the array, its cost accepted.  ``subsample`` = (seed,
    threshold): every set's table is that of the reads the subsampling rule keeps (``readsets.fused_set``: selected on the device; the
    source must have been opened with ``mate_keys``, and reads on the host go up as arrays with their keys); ``kept``: a list whose
    two entries get the reads kept and the reads they were selected from added.  ``dedup``: every set's table is that of the set
    without its duplicate fragments (``readsets.fused_set``; behind ``subsample``), ``removed``: a list whose two entries get the reads
    removed and the reads they were removed from added."""
    if dedup:
        readsets.check_fragment_source(source)
    from_xs = stranded == native.STRAND_FROM_XS
    if motif is not None and not from_xs:
        raise ValueError("strand from motif is the mode of the reads' strand bytes (STRAND_FROM_XS)")
    if from_xs and not getattr(source, "aux_strand", False):
        raise ValueError("strand from XS: the alignment source was opened without aux_strand")
    pieces, lock = {}, threading.Lock()

    def add_host(dr, chrom):
        if isinstance(source, native.BamFile):
            return dr.add_bam(source, chrom)
        rs = source.reads(chrom)
        if rs is None or not rs.n:
            return 0
        dr.add(native.ReadArrays(rs.pos, rs.flag, rs.cig_off, rs.cigar))
        return rs.n

    def job(ctx, chrom, add):
        if add is None and not from_xs and subsample is None and not dedup:
            def add(dr):
                return add_host(dr, chrom)
        with readsets.fused_set(ctx, source, chrom, add, with_strand=from_xs, subsample=subsample, kept=kept, dedup=dedup, removed=removed) as dr:
            if dr is None:
                return
            if motif is not None:
                genome = motif.on(ctx)
                motif.add(dr.motif_strand(genome, motif.sequence(genome, source, chrom)))
            n, table = dr.n, dr.junctions(stranded, minAnchor, minIntron, maxIntron)
        with lock:
            pieces.setdefault(chrom, []).append((n, table))

    readsets.run_plans(readsets.plans_of(source, devices, chroms), job)
    if tally is not None:
        for got in pieces.values():
            for _, t in got:
                for k, byte in enumerate(b"+-?"):
                    tally[k] += int(t["count"][t["strand"] == byte].sum())
    return {c: (sum(n for n, _ in got), merge_tables([t for _, t in got])) for c, got in pieces.items()}


def check_motif_options(genome, strandFromMotif, canonicalOnly, isStranded, strandFromXS, auto):
    """The refusals ``junctions`` and ``process`` share: what needs ``genome``, and what ``strandFromMotif`` is an alternative to."""
    if strandFromMotif and genome is None:
        raise ValueError("strandFromMotif needs genome: the FASTA the reads were aligned to")
    if canonicalOnly and genome is None:
        raise ValueError("canonicalOnly needs genome: the FASTA the reads were aligned to")
    for other, name in ((isStranded, "isStranded"), (strandFromXS, "strandFromXS"), (auto, "strandedType 'auto'")):
        if strandFromMotif and other:
            raise ValueError("strandFromMotif and %s are alternatives: one source for a junction's strand" % name)


def junctions(inBAM, outputPath, isStranded=False, strandedType=None, minAnchor=8, minIntron=70, maxIntron=500000,
              qChrom="All", devices=(0,), threads=0, log=None, minMapQ=0, requireFlags=0, excludeFlags=0, strandFromXS=False, anyOrder=False,
              minEvidence=None, genome=None, strandFromMotif=False, canonicalOnly=False, subsample=None, seed=0, dedup=False):
    """Writes ``outputPath`` (a BED12 file) and returns the number of junctions.  ``strandedType="auto"``: the library's strandedness
    is inferred first, from the reads' XS:A tags (``strandedness.py``), and the call goes on as if the verdict had been passed.  ``minMapQ`` / ``requireFlags`` / ``excludeFlags``:
    the read filter of ``process`` (samtools view's -q / -f / -F; changes results) -- the junctions of the reads that pass.
    ``strandFromXS``: for an unstranded library, the strand column from the reads' XS:A tag (regtools' ``-s XS``) instead of ``?``;
    an alternative to ``isStranded``.  ``anyOrder`` (changes no result): the BAM may be in any record order -- its reads are
    coordinate-sorted on the GPU after the decode instead of by ``samtools sort`` beforehand (``process``).  ``genome`` (this
    build only): the uncompressed FASTA the reads were aligned to, for ``strandFromMotif`` -- an alternative to ``isStranded``,
    ``strandFromXS`` and ``strandedType="auto"``: the strand column from the splice motifs of each read's junctions, as STAR's
    ``--outSAMstrandField intronMotif`` would have tagged it, for a file that has no tags -- and ``canonicalOnly`` (changes results):
    junctions whose motif is none of the six are not written.  ``subsample`` (this build only; changes results): a fraction in
    (0, 1] -- the junctions of that share of the reads, chosen by name and ``seed`` on the GPU (``spl_reads_subsample``: mates stay
    together, the same names whatever the file's order or container; not samtools view -s' choice of reads): what this command writes
    of a file that holds exactly those reads.  ``dedup`` (this build only; changes results): the junctions of the reads that are no
    PCR duplicates (``spl_reads_dedup``; the rule is ``csrc/spl_dup_rule.h``), behind ``subsample`` when both are given: what this
    command writes of a file from which the marked reads have been taken."""
    log = _process.logger(log)
    if dedup:
        devices = _process.one_device(devices, log, "--dedup: the alignment file is decoded and deduplicated")
    selection = None if subsample is None else (int(seed), readsets.subsample_threshold(subsample))
    if selection is not None and not 0 <= selection[0] < 1 << 64:
        raise ValueError("seed must be in 0 .. 2^64 - 1")
    auto = strandedType == "auto"
    check_motif_options(genome, strandFromMotif, canonicalOnly, isStranded, strandFromXS, auto)
    if auto and strandFromXS:
        raise ValueError("strandedType 'auto' and strandFromXS are alternatives: the tag tells the library's strandedness, or the junctions' strands")
    stranded = 0 if auto else native.STRANDED_CODE[strandedType] if isStranded else 0
    if isStranded and stranded == 0 and not auto:
        raise ValueError("strandedType must be 'fr' or 'rf' for a stranded library")
    if strandFromXS and isStranded:
        raise ValueError("strandFromXS and isStranded are alternatives: the strand of the tag, or the strand of the read")
    from_bytes = bool(strandFromXS or strandFromMotif)      # mode 3: a junction's strand is its read's strand byte, whoever wrote it
    if from_bytes:
        stranded = native.STRAND_FROM_XS
    options = _process.DecodeOptions(_process.read_filter(minMapQ, requireFlags, excludeFlags), aux_strand=bool(from_bytes or auto), any_order=bool(anyOrder),
                                     mate_keys=selection is not None or bool(dedup))
    fasta = GenomeOnDevices(genome) if genome is not None else None
    try:
        with _process.decoding(inBAM, devices, None, threads, options, log=log) as source:   # (on the GPU(s), like `process`)
            if auto:     # (the library's strandedness from the reads' XS:A tags -- this command has no annotation --, then as if it had been typed)
                from . import strandedness as _strandedness
                isStranded, strandedType = _strandedness.resolve_auto(source, devices, isStranded, None, _strandedness.MIN_EVIDENCE if minEvidence is None else int(minEvidence), log)
                stranded = native.STRANDED_CODE[strandedType] if isStranded else 0
            chroms = _process.chroms_of(source, qChrom)
            if anyOrder:
                _process.log_any_order(source, log)
            tally = [0, 0, 0] if strandFromXS else None
            n_kept, n_removed = [0, 0], [0, 0]
            tables = tables_of_source(source, tuple(devices), chroms, stranded, minAnchor, minIntron, maxIntron, tally=tally, motif=fasta if strandFromMotif else None,
                                      subsample=selection, kept=n_kept, dedup=bool(dedup), removed=n_removed)
            if isinstance(source, native.BamFile) and not source.wait_all():
                raise native.SpliserNativeError(-5, "%s is not sorted by reference: sort it (samtools sort) first" % inBAM)
            _process.log_filter(source, options.read_filter, log)
            if selection is not None:
                log("  (subsample: %d of %d reads kept, fraction %r, seed %d)" % (n_kept[0], n_kept[1], float(subsample), selection[0]))
            if dedup:
                log("  (dedup: %d of %d reads removed as duplicates)" % (n_removed[0], n_removed[1]))
            if strandFromXS:
                log_xs_tally(tally, log)
            if strandFromMotif:
                log_motif_tally(fasta.tally, log)
            if canonicalOnly:
                kept = drop_noncanonical({c: t for c, (_, t) in tables.items()}, chroms, fasta, source, tuple(devices), log)
                tables = {c: (n, kept[c]) for c, (n, _) in tables.items()}
    finally:
        if fasta is not None:
            fasta.close()
    total = write_bed_file(outputPath, chroms, {c: t for c, (_, t) in tables.items()}, minAnchor, minIntron, maxIntron,
                           log=lambda chrom, n: log("%s: %d reads, %d junctions" % (chrom, tables[chrom][0], n)))
    log("Junctions written:\t%d" % total)
    return total
