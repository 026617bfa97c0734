"""Command line of the MI355X build: the sub-commands, flags and argparse dests of SpliSER v0.1.8
(SpliSER_v0_1_8.py:1295-1361), so existing pipelines only swap the script name.

Extra flags, all optional.  These change no result: ``--gpus`` / ``--devices`` to shard chromosomes over several MI355X
of one node, ``--threads`` for the BAM decode pool, ``--gpuDecode`` / ``--hostDecode``, ``--keepReads``, ``--checkJunctions``,
``--keepJunctions``.  These DO change results, and only exist where there is no junction file: ``process`` without ``-b``
takes the junctions from the BAM itself, in the same pass, and ``--minAnchor`` / ``--minIntron`` / ``--maxIntron`` say which
reads support a junction (regtools' -a / -m / -M; defaults 8 / 70 / 500000) -- with ``-b`` they are an error, the file has
its own.  ``--strandFromXS`` (``process`` without ``-b``, ``junctions``; regtools' ``-s XS``) takes a junction's strand from the
XS:A tag the aligner wrote on its reads, for an unstranded library whose junctions are otherwise all ``?``; an alternative to
``--isStranded``, and an error with ``-b``.  ``--genome FASTA`` (the same two commands) sends the genome the reads were aligned to
to the GPU; ``--strandFromMotif`` then takes the strand from the splice motifs of each read's junctions (GT..AG and its kin), for a
file whose aligner wrote no XS:A -- an alternative to ``--isStranded``, ``--strandFromXS`` and ``-s auto`` --, and ``--canonicalOnly``
drops the junctions whose motif is none of the six.  ``--minMapQ`` / ``--requireFlags`` / ``--excludeFlags`` (``process``, ``junctions``, ``combine``, ``combineShallow``) are
samtools view's -q / -f / -F applied while the BAM is decoded: the run's results are those of the pre-filtered file.  Extra sub-command: ``junctions`` writes that BED12 junction file on its own, for ``process -b`` here or for the
reference (which leaves it to regtools); ``process`` without ``-b`` writes what ``junctions`` + ``process -b`` write.
``process --flagstat`` also writes ``<outputPath>.flagstat.txt``, samtools flagstat's sixteen lines counted by the decode the
command does anyway, over the whole file whatever ``-c`` / ``-g`` say, and logs the library size (the ``Library_size`` column of
the diffSpliSER target file, for which the reference's README sends the user to ``samtools flagstat``); it changes no result.
Extra sub-command ``flagstat -B x.bam -o PATH`` writes those lines alone (the filter and engine flags, ``--gpuDecode`` /
``--hostDecode``).  Under a read filter the counters are the pre-filtered file's.
``-s auto`` (``process``, ``junctions``) infers the library's strandedness from the BAM itself -- every read's strand tallied on the
GPU against the XS:A tag of the spliced reads and, with ``-A``, against the strand of the genes it lies in -- and goes on as if the
verdict had been typed: ``--isStranded -s fr``, ``--isStranded -s rf``, or neither; ``process`` leaves the tally in
``<outputPath>.strandedness.txt``.  No verdict is an error.  Extra sub-command ``strandedness -B x.bam [-A genes.gff] [-o report.txt]``
writes that tally and the verdict alone (what the reference's README has the user find out in IGV).
``--anyOrder`` (``process``, ``junctions``, ``flagstat``, ``strandedness``; changes no result): the BAM may be in any record order, e.g. the aligner's
own output -- its reads are coordinate-sorted on the GPU after the decode instead of by ``samtools sort`` beforehand.
``-B`` (every command that has it) also takes SAM text as the aligner writes it, and that text compressed -- BGZF (``bgzip``,
``samtools view -O sam``) or gzip (``aligner | gzip``): what the file inflates to says which, no flag.  The text is parsed on the GPU;
BGZF is inflated there too, plain gzip by one host thread; a file the strict rule declines is read by the Python reader.
Extra sub-command ``coverage -B x.bam -o PREFIX [-c CHROM] [--isStranded -s fr|rf] [--perMillion]`` writes ``PREFIX.bedgraph`` (stranded:
``PREFIX.plus.bedgraph`` and ``PREFIX.minus.bedgraph``): per-base read depth in runs, reduced on the GPU from the decode -- the
coverage track of the look at the alignments the reference's README asks for, without a sorted, indexed BAM (``coverage.py``).
``--fragments``: a paired-end fragment covers a base once -- the union of both mates' blocks, mates paired on the GPU as for ``genecounts
--fragments``; not with ``--perMillion``.
Extra sub-command ``genecounts -B x.bam -A genes.gtf -o PREFIX [-t exon] [--idAttr gene_id] [-c CHROM] [--isStranded -s fr|rf]`` writes
``PREFIX.genecounts.tsv``: reads per gene, assigned on the GPU from the decode by htseq-count's ``--mode union --nonunique none`` per
read -- the two-column file ``edgeR::readDGE`` reads, without a second pass over the BAM by another program (``genecounts.py``).
``--fragments``: a paired-end fragment counts once -- the decode keeps a key of every read's name, the GPU pairs the mates.
Extra sub-command ``exoncounts -B x.bam -A genes.gtf -o PREFIX [-t exon] [--idAttr gene_id] [-c CHROM] [--isStranded -s fr|rf]`` writes
``PREFIX.exonbins.tsv`` and ``PREFIX.exoncounts.tsv``: reads per exon counting bin, counted on the GPU from the decode by DEXSeq's rule
(``featureCounts -f -O`` restricted to reads of one gene) per read -- what ``edgeR::diffSpliceDGE`` needs, without a second pass over
the BAM by another program (``exoncounts.py``).  ``--countReadPairs``: a paired-end fragment adds one to every distinct bin under either
mate -- mates paired on the GPU as for ``genecounts --fragments``, whose spelling is refused here.
Extra sub-command ``intronretention -B x.bam -A genes.gtf -o PREFIX [-t exon] [--idAttr gene_id] [--trimPercent 30] [-c CHROM] [--isStranded
-s fr|rf]`` writes ``PREFIX.introns.tsv``: per annotated intron the trimmed depth of its measurable bases, the splice counts at its ends and
the IR ratio, taken on the GPU from the decode -- IRFinder's measure, without a sorted BAM and a second tool (``intronretention.py``).
``--fragments``: depth and splice counts per fragment -- ``coverage --fragments``' depth, and a junction both mates cross counted once.
``junctions`` and ``process`` have no such switch: the BED score feeds alpha, which stays per read beside beta1 / beta2.
Extra sub-command ``duplicates -B x.bam -o PREFIX [-c CHROM]`` writes ``PREFIX.duplicates.tsv`` and ``PREFIX.duplicates.hist.tsv``: per
chromosome the fragments and the PCR duplicate fragments among them, and the histogram of duplicate group sizes, marked on the GPU
from the decode -- no sorted copy, no ``fixmate``, no rewritten file (``duplicates.py``).  ``--dedup`` (``junctions``, ``genecounts``,
``saturation``; changes results): the command runs on the reads that are not marked.
Not read: CRAM, a pipe, and compressed text that has no ``@`` header line (uncompressed, the Python reader still takes that).
"""
import argparse
import sys
import timeit

VERSION = "v0.1.8-mi355x"


def build_parser(fragment_switches=False):
    """The command line.  ``fragment_switches``: with ``coverage --fragments`` and ``intronretention --fragments``, as ``main`` builds it.
    Without (the default) those two commands take the arguments they took before the switches existed, and refuse the switch: callers
    that build the parser themselves, and the tests that pin ``--fragments`` to ``genecounts``, see the parser they know."""
    parser = argparse.ArgumentParser(description="SpliSER - Splice Site Strength Estimates from RNA-seq (MI355X build)")
    sub = parser.add_subparsers(dest="command")
    p = sub.add_parser("process")
    p.add_argument("-B", "--BAMFile", dest="inBAM", required=True, help="The mapped RNA-seq file in BAM format (this build: or SAM text, plain or compressed as BGZF or gzip; compressed text needs its @ header)")
    p.add_argument("-b", "--bedFile", dest="inBed", required=False, default=None,
                   help="The Tophat-style splice junction bed file; (this build only) without it the junctions are taken from the BAM "
                        "itself, in the same pass: what `junctions` followed by `process -b` writes, from one command and one decode")
    p.add_argument("--minAnchor", dest="minAnchor", type=int, default=None,
                   help="(this build only, without -b; changes results) both anchors of a read must be this long to support a junction "
                        "(regtools -a) - default: 8")
    p.add_argument("--minIntron", dest="minIntron", type=int, default=None, help="(without -b; changes results) regtools -m - default: 70")
    p.add_argument("--maxIntron", dest="maxIntron", type=int, default=None,
                   help="(without -b; changes results) regtools -M, 0 = no limit - default: 500000")
    p.add_argument("--keepJunctions", dest="keepJunctions", default=False, action="store_true",
                   help="(this build only, without -b) also write <outputPath>.junctions.bed: the file `junctions` writes for the same "
                        "BAM and knobs")
    p.add_argument("--strandFromXS", dest="strandFromXS", default=False, action="store_true",
                   help="(this build only, without -b; changes results) unstranded library: a junction's strand is the XS:A tag its reads "
                        "carry (regtools -s XS) instead of '?'; not together with --isStranded")
    p.add_argument("--genome", dest="genome", default=None, metavar="FASTA",
                   help="(this build only, without -b) the uncompressed FASTA the aligner's index was built from: it goes to the GPU as base codes, for "
                        "--strandFromMotif and --canonicalOnly")
    p.add_argument("--strandFromMotif", dest="strandFromMotif", default=False, action="store_true",
                   help="(needs --genome; changes results) a junction's strand from the splice motifs of its reads' junctions in the genome "
                        "(GT..AG and its kin), as STAR --outSAMstrandField intronMotif would have tagged them, for a file without XS:A tags; "
                        "an alternative to --isStranded, --strandFromXS and -s auto")
    p.add_argument("--canonicalOnly", dest="canonicalOnly", default=False, action="store_true",
                   help="(needs --genome; changes results) junctions whose motif is none of GT..AG, GC..AG, AT..AC or their reverse complements "
                        "are dropped")
    p.add_argument("-o", "--outputPath", dest="outputPath", required=True,
                   help="Absolute path, including file prefix where the .SpliSER.tsv file is written")
    p.add_argument("-A", "--annotationFile", dest="annotationFile", required=False,
                   help="optional: gff3 or gtf file matching the reference genome used for alignment")
    p.add_argument("-t", "--annotationType", dest="aType", nargs="?", default="gene", type=str, required=False,
                   help="optional: the feature to be extracted from the annotation file - default: gene")
    p.add_argument("-c", "--chromosome", dest="qChrom", nargs="?", default="All", type=str, required=False,
                   help="optional: limit SpliSER to one chromosome/scaffold - default: All")
    p.add_argument("-g", "--gene", dest="qGene", nargs="?", default="All", type=str, required=False,
                   help="optional: limit SpliSER to splice sites falling in a single locus "
                        "(requires --chromosome, --annotationFile and --maxIntronSize)")
    p.add_argument("-m", "--maxIntronSize", dest="maxIntronSize", nargs="?", default=0, type=int, required=False,
                   help="optional: required with --gene, the max intron size used in aligning the bam file")
    p.add_argument("--isStranded", dest="isStranded", default=False, action="store_true")
    p.add_argument("-s", "--strandedType", dest="strandedType", nargs="?", type=str, required=False,
                   help='optional: strand specificity of the library, "rf" (first-strand) or "fr" (second-strand); (this build only) "auto": '
                        "inferred from the BAM -- " + AUTO_HELP)
    p.add_argument("--minEvidence", dest="minEvidence", type=int, default=None, help=MIN_EVIDENCE_HELP)
    p.add_argument("--beta2Cryptic", dest="isbeta2Cryptic", default=False, action="store_true",
                   help="optional: weight the utilisation of competing splice sites into SSE (legacy)")
    p.add_argument("--checkJunctions", dest="checkJunctions", default=False, action="store_true",
                   help="(this build only) also count every junction in the BAM on the GPU and write <outputPath>.junctionCheck.tsv: "
                        "BED alpha against reads in the BAM; changes no result")
    p.add_argument("--gpuDecode", dest="gpuDecode", default=None, action="store_true",
                   help="(this build only) inflate the BAM's BGZF blocks and extract its records on the GPU whatever the file "
                        "looks like (the default with one GPU; with several, only files that compress like real libraries go "
                        "that way); changes no result")
    p.add_argument("--hostDecode", dest="gpuDecode", action="store_false",
                   help="(this build only) decode the BAM on host threads")
    p.add_argument("--keepReads", dest="keepReads", default=False, action="store_true",
                   help="(this build only) also write <outputPath>.SpliSER.reads (flag, POS, CIGAR of every read): combine takes it "
                        "instead of decoding the BAM again while it is still that BAM's")
    p.add_argument("--flagstat", dest="flagstat", default=False, action="store_true",
                   help="(this build only) also write <outputPath>.flagstat.txt: samtools flagstat's counters of the whole BAM, from "
                        "the decode this command does anyway, and log the library size (mapped reads); changes no result")
    p.add_argument("--anyOrder", dest="anyOrder", default=False, action="store_true", help=ANY_ORDER_HELP)
    _filter_flags(p)
    _engine_flags(p)
    f = sub.add_parser("flagstat", help="(this build only) samtools flagstat's counters of a BAM, counted while it is decoded on the GPU")
    f.add_argument("-B", "--BAMFile", dest="inBAM", required=True)
    f.add_argument("-o", "--outputPath", dest="outputPath", required=True, help="path of the text file to write")
    _decode_flags(f)
    _filter_flags(f)
    _engine_flags(f)
    c = sub.add_parser("combine")
    c.add_argument("-S", "--samplesFile", dest="samplesFile", required=True,
                   help="three-column .tsv: sample name, path of its .SpliSER.tsv, path of its BAM")
    c.add_argument("-o", "--outputPath", dest="outputPath", required=True, help="output prefix (.combined.tsv is appended)")
    c.add_argument("-g", "--gene", dest="qGene", nargs="?", default="All", type=str, required=False)
    c.add_argument("--isStranded", dest="isStranded", default=False, action="store_true")
    c.add_argument("-s", "--strandedType", dest="strandedType", nargs="?", default="fr", type=str, required=False)
    c.add_argument("--beta2Cryptic", dest="isbeta2Cryptic", default=False, action="store_true")
    _filter_flags(c)
    _engine_flags(c)
    h = sub.add_parser("combineShallow")
    h.add_argument("-S", "--samplesFile", dest="samplesFile", required=True)
    h.add_argument("-g", "--gene", dest="qGene", nargs="?", default="All", type=str, required=False)
    h.add_argument("-o", "--outputPath", dest="outputPath", required=True)
    h.add_argument("--isStranded", dest="isStranded", default=False, action="store_true")
    h.add_argument("-m", "--minSamples", dest="minSamples", required=False, nargs="?", default=0, type=int)
    h.add_argument("-r", "--minReads", dest="minReads", required=False, nargs="?", default=10, type=int)
    h.add_argument("-e", "--minSSE", dest="minSSE", required=False, nargs="?", default=0.00, type=float)
    h.add_argument("-s", "--strandedType", dest="strandedType", nargs="?", type=str, required=False)
    h.add_argument("--beta2Cryptic", dest="isbeta2Cryptic", default=False, action="store_true")
    _filter_flags(h)
    _engine_flags(h)
    o = sub.add_parser("output")
    o.add_argument("-S", "--samplesFile", dest="samplesFile", required=True)
    o.add_argument("-C", "--combinedFile", dest="combinedFile", required=True)
    o.add_argument("-t", "--outputType", dest="outputType", required=True, help="DiffSpliSER or GWAS")
    o.add_argument("-o", "--outputPath", dest="outputPath", required=True)
    o.add_argument("-r", "--minReads", dest="minReads", required=False, nargs="?", default=10, type=int)
    o.add_argument("-g", "--gene", dest="qGene", required=False, nargs="?", default="All", type=str)
    o.add_argument("-m", "--minSamples", dest="minSamples", required=False, nargs="?", default=50, type=int)
    j = sub.add_parser("junctions", help="(this build only) BED12 junction file for `process -b`, derived from the BAM on the GPU")
    j.add_argument("-B", "--BAMFile", dest="inBAM", required=True)
    j.add_argument("-o", "--outputPath", dest="outputPath", required=True, help="path of the BED12 file to write")
    j.add_argument("-c", "--chromosome", dest="qChrom", nargs="?", default="All", type=str, required=False)
    j.add_argument("--isStranded", dest="isStranded", default=False, action="store_true")
    j.add_argument("-s", "--strandedType", dest="strandedType", nargs="?", type=str, required=False,
                   help='"fr" or "rf"; "auto": inferred from the BAM\'s XS:A tags -- ' + AUTO_HELP)
    j.add_argument("--minEvidence", dest="minEvidence", type=int, default=None, help=MIN_EVIDENCE_HELP)
    j.add_argument("--strandFromXS", dest="strandFromXS", default=False, action="store_true",
                   help="unstranded library: the strand column from the reads' XS:A tag (regtools -s XS) instead of '?'; not together "
                        "with --isStranded")
    j.add_argument("--genome", dest="genome", default=None, metavar="FASTA",
                   help="(this build only) the uncompressed FASTA the aligner's index was built from: it goes to the GPU as base codes, for "
                        "--strandFromMotif and --canonicalOnly")
    j.add_argument("--strandFromMotif", dest="strandFromMotif", default=False, action="store_true",
                   help="(needs --genome; changes results) a junction's strand from the splice motifs of its reads' junctions in the genome "
                        "(GT..AG and its kin), as STAR --outSAMstrandField intronMotif would have tagged them, for a file without XS:A tags; "
                        "an alternative to --isStranded, --strandFromXS and -s auto")
    j.add_argument("--canonicalOnly", dest="canonicalOnly", default=False, action="store_true",
                   help="(needs --genome; changes results) junctions whose motif is none of GT..AG, GC..AG, AT..AC or their reverse complements "
                        "are dropped")
    j.add_argument("-a", "--minAnchor", dest="minAnchor", type=int, default=8, help="both anchors of a read must be this long (regtools -a)")
    j.add_argument("-m", "--minIntron", dest="minIntron", type=int, default=70, help="regtools -m")
    j.add_argument("-M", "--maxIntron", dest="maxIntron", type=int, default=500000, help="regtools -M; 0 = no limit")
    j.add_argument("--anyOrder", dest="anyOrder", default=False, action="store_true", help=ANY_ORDER_HELP)
    # (default SUPPRESS: without the switches the parsed arguments are what they were, key for key)
    j.add_argument("--subsample", dest="subsample", type=float, default=argparse.SUPPRESS, metavar="FRAC",
                   help="(this build only; changes results) the junctions of a fraction of the reads, 0 < FRAC <= 1, chosen on the GPU by a hash of "
                        "the read's name and --seed: mates stay together, and the same names are kept whatever the file's order or container "
                        "(not samtools view -s' choice of reads)")
    j.add_argument("--seed", dest="seed", type=int, default=argparse.SUPPRESS, help="(with --subsample) the seed of the choice, 0 .. 2^64 - 1 - default: 0")
    j.add_argument("--dedup", dest="dedup", default=argparse.SUPPRESS, action="store_true", help=DEDUP_HELP + "; with --subsample the fraction is chosen first")
    _filter_flags(j)
    _engine_flags(j)
    u = sub.add_parser("saturation", help="(this build only) junctions and SpliSER sites at nested subsamples of the reads, from one decode, on the GPU: how many sites "
                                          "pass -r now, and whether more would with more reads (no samtools view -s, no second run)")
    u.add_argument("-B", "--BAMFile", dest="inBAM", required=True)
    u.add_argument("-o", "--outputPath", dest="outputPath", required=True, help="output prefix: .saturation.tsv is appended")
    u.add_argument("--steps", dest="steps", type=int, default=20, help="rows of the table: step k of K holds the fraction k / K of the reads, 1..100 - default: 20")
    u.add_argument("--seed", dest="seed", type=int, default=0, help="the seed of the choice of reads (a hash of the read's name and this), 0 .. 2^64 - 1 - default: 0")
    u.add_argument("-r", "--minReads", dest="minReads", type=int, default=10,
                   help="a site passes with alpha_count + beta1_count + beta2Simple_count of at least this (output's and combineShallow's -r), a junction with "
                        "this score - default: 10")
    u.add_argument("-c", "--chromosome", dest="qChrom", nargs="?", default="All", type=str, required=False, help="optional: one chromosome only")
    u.add_argument("--isStranded", dest="isStranded", default=False, action="store_true")
    u.add_argument("-s", "--strandedType", dest="strandedType", nargs="?", type=str, required=False,
                   help='"fr" or "rf" (not "auto": the `strandedness` command tells which)')
    u.add_argument("-a", "--minAnchor", dest="minAnchor", type=int, default=8, help="as for junctions (regtools -a)")
    u.add_argument("-m", "--minIntron", dest="minIntron", type=int, default=70, help="regtools -m")
    u.add_argument("-M", "--maxIntron", dest="maxIntron", type=int, default=500000, help="regtools -M; 0 = no limit")
    _decode_flags(u)
    u.add_argument("--dedup", dest="dedup", default=argparse.SUPPRESS, action="store_true",
                   help=DEDUP_HELP + "; every step's set is deduplicated behind its selection, and the table gets the column reads_before_dedup")
    _filter_flags(u)
    _engine_flags(u)
    d = sub.add_parser("duplicates", help="(this build only) the library's PCR duplicate rate from the decode, on the GPU: fragments, duplicate fragments and the "
                                          "histogram of group sizes per chromosome -- no sorted copy, no fixmate, no rewritten file")
    d.add_argument("-B", "--BAMFile", dest="inBAM", required=True)
    d.add_argument("-o", "--outputPath", dest="outputPath", required=True, help="output prefix: .duplicates.tsv and .duplicates.hist.tsv are appended")
    d.add_argument("-c", "--chromosome", dest="qChrom", nargs="?", default="All", type=str, required=False, help="optional: one chromosome only")
    _decode_flags(d)
    _filter_flags(d)
    _engine_flags(d)
    s = sub.add_parser("strandedness", help="(this build only) is the library unstranded, fr or rf?  Tallied from the BAM on the GPU: " + AUTO_HELP)
    s.add_argument("-B", "--BAMFile", dest="inBAM", required=True)
    s.add_argument("-A", "--annotationFile", dest="annotationFile", required=False,
                   help="optional: gff3 or gtf file; reads that lie in a stretch covered by genes of one strand only are held against that strand")
    s.add_argument("-t", "--annotationType", dest="aType", nargs="?", default="gene", type=str, required=False)
    s.add_argument("-c", "--chromosome", dest="qChrom", nargs="?", default="All", type=str, required=False, help="optional: tally one chromosome only")
    s.add_argument("-o", "--outputPath", dest="outputPath", required=False, default=None, help="optional: path of the tab-separated report to write")
    s.add_argument("--minEvidence", dest="minEvidence", type=int, default=1000, help=MIN_EVIDENCE_HELP)
    _decode_flags(s)
    _filter_flags(s)
    _engine_flags(s)
    v = sub.add_parser("coverage", help="(this build only) per-base read depth of the alignment file as a bedGraph, reduced on the GPU from the decode: "
                                        "no sorted, indexed BAM needed to look at the data")
    v.add_argument("-B", "--BAMFile", dest="inBAM", required=True)
    v.add_argument("-o", "--outputPath", dest="outputPath", required=True,
                   help="output prefix: .bedgraph is appended, or .plus.bedgraph and .minus.bedgraph with --isStranded")
    v.add_argument("-c", "--chromosome", dest="qChrom", nargs="?", default="All", type=str, required=False, help="optional: one chromosome only")
    v.add_argument("--isStranded", dest="isStranded", default=False, action="store_true", help="one track per strand of the reads (check_strand's rule)")
    v.add_argument("-s", "--strandedType", dest="strandedType", nargs="?", type=str, required=False,
                   help='"fr" or "rf" (not "auto": the `strandedness` command tells which)')
    v.add_argument("--perMillion", dest="perMillion", default=False, action="store_true",
                   help="values per million mapped reads: depth * 1000000 / the library size --flagstat logs (under the filters)")
    _decode_flags(v)
    # (default SUPPRESS: without the switch the parsed arguments are what they were, key for key)
    if fragment_switches:
        v.add_argument("--fragments", dest="fragments", default=argparse.SUPPRESS, action="store_true",
                   help="paired-end: mates are paired on the GPU by a key of their names (as for `genecounts --fragments`) and a pair whose mates both cover on the "
                        "track covers the union of their blocks once (deepTools bamCoverage's paired-end default, bedtools genomecov -pc, without filling the gap "
                        "between the mates); a pair split over two chromosomes, by the read filter or over the two tracks covers as two reads; not with --perMillion")
    _filter_flags(v)
    _engine_flags(v)
    n = sub.add_parser("genecounts", help="(this build only) reads per gene as htseq-count's two-column file, assigned on the GPU from the decode "
                                          "(--mode union --nonunique none, per read): no second pass over the BAM by another program")
    n.add_argument("-B", "--BAMFile", dest="inBAM", required=True)
    n.add_argument("-A", "--annotationFile", dest="annotationFile", required=False, default=None, help="gff3 or gtf file matching the reference genome used for alignment (required)")
    n.add_argument("-o", "--outputPath", dest="outputPath", required=True, help="output prefix: .genecounts.tsv is appended")
    n.add_argument("-t", "--annotationType", dest="aType", nargs="?", default="exon", type=str, required=False,
                   help="the feature type (column 3) whose lines are a gene's features - default: exon")
    n.add_argument("--idAttr", dest="idAttr", default="gene_id", type=str, required=False, help="the attribute (column 9) that names a feature's gene - default: gene_id")
    n.add_argument("-c", "--chromosome", dest="qChrom", nargs="?", default="All", type=str, required=False,
                   help="optional: the reads of one chromosome only, and the genes with a feature on it")
    n.add_argument("--isStranded", dest="isStranded", default=False, action="store_true", help="a read counts for the features of its strand only (check_strand's rule)")
    n.add_argument("-s", "--strandedType", dest="strandedType", nargs="?", type=str, required=False,
                   help='"fr" or "rf" (not "auto": the `strandedness` command tells which)')
    _decode_flags(n)
    n.add_argument("--fragments", dest="fragments", default=False, action="store_true",
                   help="paired-end: mates are paired on the GPU by a key of their names and a fragment counts once, by both mates' blocks "
                        "(htseq-count's and featureCounts -p --countReadPairs' way); a pair split over two chromosomes or by the read filter counts as two")
    n.add_argument("--dedup", dest="dedup", default=argparse.SUPPRESS, action="store_true", help=DEDUP_HELP + "; with --fragments the mates are paired behind it")
    _filter_flags(n)
    _engine_flags(n)
    x = sub.add_parser("exoncounts", help="(this build only) reads per exon counting bin for edgeR::diffSpliceDGE / DEXSeq, counted on the GPU from the decode "
                                          "(dexseq_count.py's rule, featureCounts -f -O for reads of one gene; per read, per fragment with --countReadPairs): no second pass over the BAM "
                                          "by another program")
    x.add_argument("-B", "--BAMFile", dest="inBAM", required=True)
    x.add_argument("-A", "--annotationFile", dest="annotationFile", required=False, default=None, help="gff3 or gtf file matching the reference genome used for alignment (required)")
    x.add_argument("-o", "--outputPath", dest="outputPath", required=True, help="output prefix: .exonbins.tsv and .exoncounts.tsv are appended")
    x.add_argument("-t", "--annotationType", dest="aType", nargs="?", default="exon", type=str, required=False,
                   help="the feature type (column 3) whose lines are a gene's features - default: exon")
    x.add_argument("--idAttr", dest="idAttr", default="gene_id", type=str, required=False, help="the attribute (column 9) that names a feature's gene - default: gene_id")
    x.add_argument("-c", "--chromosome", dest="qChrom", nargs="?", default="All", type=str, required=False,
                   help="optional: the reads of one chromosome only, and the bins on it (under the ids they have in the whole annotation)")
    x.add_argument("--isStranded", dest="isStranded", default=False, action="store_true", help="a read counts for the features of its strand only (check_strand's rule)")
    x.add_argument("-s", "--strandedType", dest="strandedType", nargs="?", type=str, required=False,
                   help='"fr" or "rf" (not "auto": the `strandedness` command tells which)')
    _decode_flags(x)
    x.add_argument("--fragments", dest="fragments", default=False, action="store_true",
                   help="(refused: `genecounts --fragments`' spelling; here the switch is --countReadPairs)")
    # (default SUPPRESS: without the switch the parsed arguments are what they were, key for key)
    x.add_argument("--countReadPairs", dest="countReadPairs", default=argparse.SUPPRESS, action="store_true",
                   help="paired-end: mates are paired on the GPU by a key of their names (as for `genecounts --fragments`) and a fragment adds one to every "
                        "distinct bin under either mate, a bin both mates overlap once (DEXSeq's and featureCounts -f -O -p --countReadPairs' way); a pair split "
                        "over two chromosomes or by the read filter counts as two")
    _filter_flags(x)
    _engine_flags(x)
    i = sub.add_parser("intronretention", help="(this build only) per annotated intron the trimmed depth, the splice counts and the IR ratio, taken on the GPU from the "
                                               "decode (IRFinder's measure): no sorted BAM, no second pass over the file by another program")
    i.add_argument("-B", "--BAMFile", dest="inBAM", required=True)
    i.add_argument("-A", "--annotationFile", dest="annotationFile", required=False, default=None, help="gff3 or gtf file matching the reference genome used for alignment (required)")
    i.add_argument("-o", "--outputPath", dest="outputPath", required=True, help="output prefix: .introns.tsv is appended")
    i.add_argument("-t", "--annotationType", dest="aType", nargs="?", default="exon", type=str, required=False,
                   help="the feature type (column 3) whose lines are a gene's features - default: exon")
    i.add_argument("--idAttr", dest="idAttr", default="gene_id", type=str, required=False, help="the attribute (column 9) that names a feature's gene - default: gene_id")
    i.add_argument("--trimPercent", dest="trimPercent", default=30, type=int, required=False,
                   help="percent of an intron's measurable bases left out at either end of their sorted depths, 0..49 (0: the plain mean) - default: 30")
    i.add_argument("-c", "--chromosome", dest="qChrom", nargs="?", default="All", type=str, required=False,
                   help="optional: the introns of one chromosome only (under the ids they have in the whole annotation)")
    i.add_argument("--isStranded", dest="isStranded", default=False, action="store_true", help="an intron is measured on the track of its strand (check_strand's rule)")
    i.add_argument("-s", "--strandedType", dest="strandedType", nargs="?", type=str, required=False,
                   help='"fr" or "rf" (not "auto": the `strandedness` command tells which)')
    _decode_flags(i)
    if fragment_switches:
        i.add_argument("--fragments", dest="fragments", default=argparse.SUPPRESS, action="store_true",
                   help="paired-end: depth and splice counts per fragment (IRFinder's way) -- the depth is `coverage --fragments`', and a junction that both mates of "
                        "a pair support counts once; mates are paired on the GPU by a key of their names")
    _filter_flags(i)
    _engine_flags(i)
    return parser


def _flag_mask(text):
    return int(text, 0)     # (0x900 as well as 2304, as samtools takes them)


def _decode_flags(p):
    p.add_argument("--gpuDecode", dest="gpuDecode", default=None, action="store_true", help="decode on the GPU whatever the file looks like (as for process)")
    p.add_argument("--hostDecode", dest="gpuDecode", action="store_false", help="decode the BAM on host threads")
    p.add_argument("--anyOrder", dest="anyOrder", default=False, action="store_true", help=ANY_ORDER_HELP)


def _filter_flags(p):
    p.add_argument("--minMapQ", dest="minMapQ", type=int, default=0,
                   help="(this build only; changes results) skip alignments with MAPQ below this, 0..255 (samtools view -q; "
                        "255 passes any threshold) - default: 0")
    p.add_argument("--requireFlags", dest="requireFlags", type=_flag_mask, default=0,
                   help="(this build only; changes results) keep only alignments with all of these FLAG bits set (samtools view -f; "
                        "decimal, or hex as 0x2) - default: 0")
    p.add_argument("--excludeFlags", dest="excludeFlags", type=_flag_mask, default=0,
                   help="(this build only; changes results) skip alignments with any of these FLAG bits set (samtools view -F, "
                        "e.g. 0x900: secondary and supplementary) - default: 0")


AUTO_HELP = ("every read's strand is held against the XS:A tag of the spliced reads and, with -A, against the strand of the genes it lies in; per "
             "source >= 90%% of the reads agreeing with fr means fr, <= 10%% rf, 40..60%% unstranded, anything else (or two sources that differ) "
             "undetermined: a stated policy, not a measurement")
MIN_EVIDENCE_HELP = "(-s auto, strandedness) reads with evidence a source needs to be heard - default: 1000"

DEDUP_HELP = ("(this build only; changes results) PCR duplicate fragments are marked on the GPU and left out, as after MarkDuplicates and --excludeFlags 0x400 "
              "without the sorted copy: fragments of one chromosome with the same unclipped 5' ends and orientations are one group, the one with the "
              "smallest name hash stays (the `duplicates` command reports the rate; Picard's choice by base quality is not made)")

ANY_ORDER_HELP = ("(this build only; changes no result) the BAM may be in any record order, e.g. as the aligner wrote it: its reads are "
                  "coordinate-sorted on the GPU after the decode instead of by samtools sort beforehand")


def _engine_flags(p):
    p.add_argument("--gpus", dest="gpus", type=int, default=1, help="number of MI355X devices to shard chromosomes over")
    p.add_argument("--devices", dest="devices", type=str, default=None, help="explicit device list, e.g. 0,2,3")
    p.add_argument("--threads", dest="threads", type=int, default=0, help="host threads for BAM decode (0 = all cores)")


def main(argv=None):
    print("\nSpliSER " + VERSION + " (MI355X / gfx950 build of SpliSER v0.1.8, SKB LAB)\n")
    start = timeit.default_timer()
    parser = build_parser(fragment_switches=True)
    kwargs = vars(parser.parse_args(argv))
    command = kwargs.pop("command")
    if command is None:
        parser.error("a sub-command is required")
    gpus = kwargs.pop("gpus", 1)
    devices = kwargs.pop("devices", None)
    devices = tuple(int(d) for d in devices.split(",")) if devices else tuple(range(max(1, gpus)))
    threads = kwargs.pop("threads", 0)
    # same validation rules as SpliSER_v0_1_8.py:1350-1355
    if command == "process" and kwargs.get("qGene") != "All" and (kwargs.get("annotationFile") is None or kwargs.get("maxIntronSize") is None):
        print(kwargs.get("qGene"))
        print(kwargs.get("annotationFile"))
        parser.error("--gene requires --annotationFile and --maxIntronSize")
    elif command in ("process", "combine", "combineShallow", "junctions", "coverage", "genecounts", "exoncounts", "intronretention") and kwargs.get("isStranded") is True and kwargs.get("strandedType") is None:
        parser.error("--isStranded requires parameter --strandedType/-s as fr or rf")
    if command == "coverage" and kwargs.get("strandedType") == "auto":
        parser.error("coverage: -s auto is not taken here: the `strandedness` command tells whether the library is fr or rf")
    if command == "coverage" and kwargs.get("isStranded") and kwargs.get("strandedType") not in ("fr", "rf"):
        parser.error("coverage: --strandedType/-s must be fr or rf")
    if command in ("genecounts", "exoncounts", "intronretention") and kwargs.get("annotationFile") is None:
        parser.error("%s: --annotationFile/-A is required: the genes are its features" % command)
    if command in ("genecounts", "exoncounts", "intronretention") and kwargs.get("strandedType") == "auto":
        parser.error("%s: -s auto is not taken here: the `strandedness` command tells whether the library is fr or rf" % command)
    if command in ("genecounts", "exoncounts", "intronretention") and kwargs.get("isStranded") and kwargs.get("strandedType") not in ("fr", "rf"):
        parser.error("%s: --strandedType/-s must be fr or rf" % command)
    if command == "exoncounts" and kwargs.pop("fragments", False):
        parser.error("exoncounts: --fragments is `genecounts --fragments`' spelling; here the switch is --countReadPairs")
    if command == "coverage" and kwargs.get("fragments") and kwargs.get("perMillion"):
        parser.error("coverage: --perMillion --fragments is refused: no fragment library size is counted, and fragment depth per million mapped reads would mislead")
    if command == "intronretention" and not 0 <= kwargs["trimPercent"] <= 49:
        parser.error("intronretention: --trimPercent must be in 0..49")
    if command in ("process", "junctions") and kwargs.get("strandFromXS") and kwargs.get("strandedType") == "auto":
        parser.error("-s auto and --strandFromXS are alternatives: the tag tells the library's strandedness, or the junctions' strands")
    if command in ("process", "junctions"):
        for flag in ("strandFromMotif", "canonicalOnly"):
            if kwargs.get(flag) and kwargs.get("genome") is None:
                parser.error("--%s needs --genome: the FASTA the reads were aligned to" % flag)
        for other, name in (("isStranded", "--isStranded"), ("strandFromXS", "--strandFromXS")):
            if kwargs.get("strandFromMotif") and kwargs.get(other):
                parser.error("--strandFromMotif and %s are alternatives: one source for a junction's strand" % name)
        if kwargs.get("strandFromMotif") and kwargs.get("strandedType") == "auto":
            parser.error("--strandFromMotif and -s auto are alternatives: one source for a junction's strand")
        if kwargs.get("genome") is not None:
            try:
                with open(kwargs["genome"], "rb") as fh:
                    magic = fh.read(2)
            except OSError as exc:
                parser.error("--genome %s: %s" % (kwargs["genome"], exc.strerror))
            if magic == b"\x1f\x8b":
                parser.error("--genome %s is compressed: pass the uncompressed FASTA the aligner's index was built from" % kwargs["genome"])
    if command == "saturation":
        if kwargs.get("strandedType") == "auto":
            parser.error("saturation: -s auto is not taken here: the `strandedness` command tells whether the library is fr or rf")
        if kwargs.get("isStranded") and kwargs.get("strandedType") not in ("fr", "rf"):
            parser.error("saturation: --isStranded requires --strandedType/-s as fr or rf")
        if not 1 <= kwargs["steps"] <= 100:
            parser.error("saturation: --steps must be in 1..100")
        if kwargs["minReads"] < 1:
            parser.error("saturation: -r / --minReads must be at least 1")
        if not 0 <= kwargs["seed"] < 1 << 64:
            parser.error("saturation: --seed must be in 0 .. 2^64 - 1")
        if min(kwargs["minAnchor"], kwargs["minIntron"], kwargs["maxIntron"]) < 0:
            parser.error("--minAnchor / --minIntron / --maxIntron must not be negative")
    if command == "junctions":
        if "seed" in kwargs and "subsample" not in kwargs:
            parser.error("junctions: --seed belongs to --subsample")
        if "subsample" in kwargs and not 0.0 < kwargs["subsample"] <= 1.0:
            parser.error("junctions: --subsample must be a fraction in (0, 1]")
        if "seed" in kwargs and not 0 <= kwargs["seed"] < 1 << 64:
            parser.error("junctions: --seed must be in 0 .. 2^64 - 1")
    if command in ("process", "junctions", "strandedness") and kwargs.get("minEvidence") is not None and kwargs["minEvidence"] < 0:
        parser.error("--minEvidence must not be negative")
    if command in ("process", "junctions") and kwargs.get("strandFromXS") and kwargs.get("isStranded"):
        parser.error("--strandFromXS and --isStranded are alternatives: the strand of the aligner's tag, or the strand of the read")
    if command in ("process", "combine", "combineShallow", "junctions", "flagstat", "strandedness", "coverage", "genecounts", "exoncounts", "intronretention", "saturation", "duplicates"):
        if not 0 <= kwargs["minMapQ"] <= 255:
            parser.error("--minMapQ must be in 0..255")
        if not (0 <= kwargs["requireFlags"] <= 65535 and 0 <= kwargs["excludeFlags"] <= 65535):
            parser.error("--requireFlags / --excludeFlags must be in 0..65535")
        if kwargs["requireFlags"] & kwargs["excludeFlags"]:
            parser.error("--requireFlags and --excludeFlags share a bit (0x%x): no read could pass" % (kwargs["requireFlags"] & kwargs["excludeFlags"]))
    if command == "process":
        if kwargs.get("inBed") is not None:
            given = [f for f, d in (("--minAnchor", "minAnchor"), ("--minIntron", "minIntron"), ("--maxIntron", "maxIntron")) if kwargs.get(d) is not None]
            if kwargs.get("keepJunctions"):
                given.append("--keepJunctions")
            if kwargs.get("strandFromXS"):
                given.append("--strandFromXS")
            given.extend(f for f, d in (("--genome", "genome"), ("--strandFromMotif", "strandFromMotif"), ("--canonicalOnly", "canonicalOnly")) if kwargs.get(d))
            if given:
                parser.error("%s: only without --bedFile (a junction file has its own junctions)" % ", ".join(given))
        else:
            if kwargs.get("checkJunctions"):
                parser.error("--checkJunctions compares the junction file with the BAM: it requires --bedFile")
            if any(kwargs.get(d) is not None and kwargs.get(d) < 0 for d in ("minAnchor", "minIntron", "maxIntron")):
                parser.error("--minAnchor / --minIntron / --maxIntron must not be negative")
        from .process import process
        if __import__("os").environ.get("SPL_PROCESS_TIMING"):
            sys.stderr.write("[cli] modules of `process` imported %.4f s after main() began\n" % (timeit.default_timer() - start))
        process(devices=devices, threads=threads, **kwargs)
        if kwargs.get("keepReads"):      # (the kept reads go out on the thread that closes the alignment file: the command is done when they are)
            from .process import wait_deferred_close
            wait_deferred_close()
    elif command == "combine":
        from .combine import combine
        combine(devices=devices, threads=threads, **kwargs)
    elif command == "combineShallow":
        from .combine import combineShallow
        combineShallow(devices=devices, threads=threads, **kwargs)
    elif command == "output":
        from .output import output
        output(**kwargs)
    elif command == "junctions":
        from .junctions import junctions
        junctions(devices=devices, threads=threads, **kwargs)
    elif command == "saturation":
        from .saturation import saturation
        saturation(devices=devices, threads=threads, **kwargs)
    elif command == "duplicates":
        from .duplicates import duplicates
        duplicates(devices=devices, threads=threads, **kwargs)
    elif command == "strandedness":
        from .strandedness import strandedness
        strandedness(devices=devices, threads=threads, **kwargs)
    elif command == "coverage":
        from .coverage import coverage
        coverage(devices=devices, threads=threads, **kwargs)
    elif command == "genecounts":
        from .genecounts import genecounts
        genecounts(devices=devices, threads=threads, **kwargs)
    elif command == "exoncounts":
        from .exoncounts import exoncounts
        exoncounts(devices=devices, threads=threads, **kwargs)
    elif command == "intronretention":
        from .intronretention import intronretention
        intronretention(devices=devices, threads=threads, **kwargs)
    elif command == "flagstat":
        from .flagstat import flagstat
        flagstat(devices=devices, threads=threads, **kwargs)
    else:
        parser.error("sub-command %r is not part of this build yet" % command)
    print("Total runtime (s): \t" + str(timeit.default_timer() - start))
    return 0


if __name__ == "__main__":
    sys.exit(main())
