"""``strandedness`` / ``-s auto`` without a GPU: the per-read rule (``spl_strand_rule_host``, the header the kernel includes) against
the yardstick of ``strandcases.py`` over every combination of the FLAG bits it reads and at the edges of a read's span; the same
header in a stand-alone program under AddressSanitizer and UBSan (tests/hostsim/strand_rule_asan.cpp); the cover-map builder
against the per-position code; the decision at its integer boundaries; the command line's refusals."""
import itertools
import os
import subprocess

import numpy as np
import pytest

import strandcases as S
from spliser_amd import cli, native, samio, strandedness as sd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLUS, MINUS = S.PLUS, S.MINUS
BITS = (0x1, 0x4, 0x10, 0x40, 0x80, 0x100, 0x200, 0x800)


@pytest.fixture(scope="module", autouse=True)
def _built():
    native.build()


def _ops(cigar):
    return np.asarray(samio.cigar_ops(cigar), np.uint32)


def _both(records, cover):
    """records: [(flag, pos, ops, xs)] -> (the hook's sums, the yardstick's)."""
    got, want = np.zeros(14, np.int64), [0] * 14
    starts, codes = ([], []) if cover is None else (list(cover[0]), list(cover[1]))
    for flag, pos, ops, xs in records:
        native.strand_rule_host(flag, pos, ops, xs, cover, got)
        S.add_read(want, flag, pos, [int(o) for o in ops], xs, starts, codes)
    return got.tolist(), want


def test_every_flag_combination_with_every_tag_and_cover_code():
    flags = [sum(b for b, on in zip(BITS, mask) if on) for mask in itertools.product((0, 1), repeat=len(BITS))]
    assert len(flags) == 256
    seen = np.zeros(14, np.int64)
    for xs in (0, PLUS, MINUS):
        for code in (0, 1, 2, 3):
            cover = (np.array([100], np.int32), np.array([code], np.uint8))
            got, want = _both([(f, 150, _ops("50M"), xs) for f in flags], cover)
            assert got == want, (xs, code)
            assert got[0] == 256 and got[1] == 16
            seen += np.asarray(got)
    assert (seen > 0).all()          # (every counter is reached by some combination)


LONG = "1M1I" * 1100 + "5M300N7M"      # 2203 ops, 1412 reference bases
COVER3 = (np.array([100, 200, 300], np.int32), np.array([1, 2, 1], np.uint8))
EDGES = [
    ("POS at start[k]", 16, 200, "50M", COVER3),
    ("POS one below start[k]", 16, 199, "50M", COVER3),
    ("POS one below start[0]", 0, 99, "1M", COVER3),
    ("end at start[k+1] - 1", 0, 150, "50M", COVER3),
    ("end at start[k+1]", 0, 151, "50M", COVER3),
    ("end at start[k+1] - 1, through an intron", 0, 110, "10M60N20M", COVER3),
    ("end at start[k+1], through an intron", 0, 110, "10M61N20M", COVER3),
    ("deletions and = X count, insertions and clips do not", 0, 110, "5S10=5I10X20D50M3S", COVER3),
    ("one base more", 0, 110, "5S10=5I10X20D51M3S", COVER3),
    ("before the first entry", 0, 10, "50M", COVER3),
    ("beyond the last entry", 0, 5000, "50M100000N50M", COVER3),
    ("no map", 0, 150, "50M", None),
    ("a map of one entry, inside", 16, 150, "50M", (np.array([100], np.int32), np.array([2], np.uint8))),
    ("a map of one entry, before it", 16, 50, "50M", (np.array([100], np.int32), np.array([2], np.uint8))),
    ("* as CIGAR", 0, 150, "*", COVER3),
    ("S and I only", 0, 150, "20S30I", COVER3),
    ("2203 ops, inside", 0, 300, LONG, COVER3),
    ("2203 ops, across a boundary", 0, 100, LONG, (np.array([100, 1511, 1512], np.int32), np.array([1, 1, 2], np.uint8))),
    ("2203 ops, up to a boundary", 0, 100, LONG, (np.array([100, 1512], np.int32), np.array([1, 2], np.uint8))),
    ("a span that needs int64", 0, 2147483581, "50M100N50M", (np.array([100, 2147483000], np.int32), np.array([3, 2], np.uint8))),
    ("a span that needs int64, an entry behind it", 0, 2147483500, "50M100N50M", (np.array([100, 2147483000, 2147483647], np.int32), np.array([3, 2, 1], np.uint8))),
    ("a span that ends beyond int32, an entry inside it", 0, 2147483500, "50M100N50M", (np.array([100, 2147483000, 2147483600], np.int32), np.array([3, 2, 1], np.uint8))),
]


@pytest.mark.parametrize("name,flag,pos,cigar,cover", EDGES, ids=[e[0] for e in EDGES])
def test_span_edges(name, flag, pos, cigar, cover):
    for xs in (0, PLUS):
        for f in (flag, flag | 1 | 0x40, flag | 1 | 0x80):
            got, want = _both([(f, pos, _ops(cigar), xs)], cover)
            assert got == want, (name, f, xs)


def test_the_edges_say_what_the_issue_says():
    """The yardstick itself, on the cases whose answer can be read off the rule."""
    def ann(flag, pos, cigar, cover):
        out = [0] * 14
        S.add_read(out, flag, pos, samio.cigar_ops(cigar), 0, list(cover[0]), list(cover[1]))
        return out[8:]
    assert ann(0, 150, "50M", COVER3) == [1, 0, 0, 0, 0, 0]         # ends at 199, in the + stretch
    assert ann(0, 151, "50M", COVER3) == [0] * 6                    # ends at 200
    assert ann(16, 200, "50M", COVER3) == [1, 0, 0, 0, 0, 0]        # a reverse read in the - stretch agrees under fr
    assert ann(0, 200, "50M", COVER3) == [0, 1, 0, 0, 0, 0]
    assert ann(163, 200, "50M", COVER3) == [0, 0, 0, 0, 1, 0]       # second, forward: fr strand -
    assert ann(0, 99, "1M", COVER3) == [0] * 6 and ann(0, 150, "*", COVER3) == [0] * 6 and ann(0, 150, "20S30I", COVER3) == [0] * 6
    assert ann(0, 5000, "50M100000N50M", COVER3) == [1, 0, 0, 0, 0, 0]


def test_a_descending_map_is_refused():
    with pytest.raises(native.SpliserNativeError) as err:
        native.strand_rule_host(0, 10, _ops("5M"), 0, (np.array([5, 5], np.int32), np.array([1, 2], np.uint8)))
    assert err.value.code == -1


def test_header_under_the_sanitizers(tmp_path):
    """The rule's header alone in a program of its own: ops and map in heap blocks of exactly their size, so that a read beyond
    either aborts the child.  Cases as lines "flag pos xs | ops | starts | codes"; answers as 14 numbers a line."""
    exe = str(tmp_path / "strand_asan")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "hostsim", "strand_rule_asan.cpp"), "-o", exe])
    cases = []
    for name, flag, pos, cigar, cover in EDGES:
        for xs in (0, MINUS):
            cases.append((flag, pos, samio.cigar_ops(cigar), xs, cover))
    for f in (0, 16, 99, 147, 83, 163, 256, 4, 0x200, 0x800):
        cases.append((f, 250, samio.cigar_ops("30M"), PLUS, COVER3))
    text = "".join("%d %d %d|%s|%s|%s\n" % (f, p, xs, " ".join(str(int(o)) for o in ops), " ".join(str(int(v)) for v in (c[0] if c else [])),
                                             " ".join(str(int(v)) for v in (c[1] if c else []))) for f, p, ops, xs, c in cases)
    out = subprocess.run([exe], input=text, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0"))
    assert out.returncode == 0, out.stderr
    lines = out.stdout.splitlines()
    assert len(lines) == len(cases)
    for (f, p, ops, xs, c), line in zip(cases, lines):
        want = [0] * 14
        S.add_read(want, f, p, ops, xs, list(c[0]) if c else [], list(c[1]) if c else [])
        assert [int(v) for v in line.split()] == want, (f, p, xs)


# ---- the cover map ------------------------------------------------------------------------------------------------------------
GENE_SETS = [
    ("nested, overlapping and abutting, one strand", [(10, 50, "+"), (20, 30, "+"), (40, 70, "+"), (70, 90, "+"), (95, 99, "+")]),
    ("both strands", [(10, 50, "+"), (30, 80, "-"), (80, 100, "-"), (60, 120, "+"), (130, 140, "-")]),
    ("genes without a strand", [(10, 50, "."), (30, 80, "-"), (70, 100, "."), (200, 210, ".")]),
    ("only genes without a strand", [(10, 50, ".")]),
    ("no genes", []),
    ("a gene at the chromosome's first base", [(0, 5, "-"), (5, 9, "+")]),
    ("the same gene twice", [(10, 20, "+"), (10, 20, "+"), (10, 20, "-")]),
]


@pytest.mark.parametrize("name,genes", GENE_SETS, ids=[g[0] for g in GENE_SETS])
def test_cover_map_against_the_code_of_every_position(name, genes):
    byte = {"+": 43, "-": 45, ".": 0}
    start, code = sd.cover_map([g[0] for g in genes], [g[1] for g in genes], [byte[g[2]] for g in genes])
    assert start.dtype == np.int32 and code.dtype == np.uint8 and start.shape == code.shape
    assert (np.diff(start) > 0).all()                              # strictly ascending ...
    assert (code[1:] != code[:-1]).all() and (not len(code) or code[0] != 0)      # ... and an entry only where the code changes
    end = max([g[1] for g in genes] + [0]) + 2
    for p in range(0, end + 1):
        assert S.map_code_at(start.tolist(), code.tolist(), p) == S.code_at(genes, p), p
    w_start, w_code = S.cover_of_genes(genes)
    assert start.tolist() == w_start.tolist() and code.tolist() == w_code.tolist()


def test_cover_map_of_the_gff_reader_columns(tmp_path):
    from spliser_amd import sites
    path = str(tmp_path / "g.gff")
    S.write_gff(path)
    bins = sites.GeneBins.from_annotation(path, "gene", "All", log=lambda m: None)
    covers = sd.covers_of(bins, S.NAMES + ["nobody"])
    assert sorted(covers) == S.NAMES
    for chrom in S.NAMES:
        want = S.library_cover(chrom)
        assert covers[chrom][0].tolist() == want[0].tolist() and covers[chrom][1].tolist() == want[1].tolist()
        assert {1, 2, 0} <= set(want[1].tolist())
    assert 3 in S.library_cover("c1")[1].tolist()


# ---- the decision -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("a,n,want", [(900, 1000, "fr"), (899, 1000, "undetermined"), (601, 1000, "undetermined"), (600, 1000, "unstranded"),
                                      (400, 1000, "unstranded"), (399, 1000, "undetermined"), (101, 1000, "undetermined"), (100, 1000, "rf"),
                                      (999, 999, "none"), (0, 999, "none"), (1000, 1000, "fr"), (0, 1000, "rf")])
def test_decision_at_its_integer_boundaries(a, n, want):
    assert S.source_verdict(a, n - a) == want
    assert sd.source_verdict(a, n - a) == want
    t = np.zeros(14, np.int64)
    t[2], t[5], t[7] = a, (n - a) // 2, (n - a) - (n - a) // 2        # (the three mate classes are added)
    assert sd.decide(t)[1]["tags"] == want and sd.decide(t)[1]["annotation"] == "none"


def _tally(tags, ann):
    t = np.zeros(14, np.int64)
    t[2], t[3], t[10], t[11] = tags[0], tags[1], ann[0], ann[1]
    return t


@pytest.mark.parametrize("tags,ann,want", [
    ((950, 50), (1900, 100), "fr"), ((50, 950), (0, 5000), "rf"), ((500, 500), (450, 550), "unstranded"),
    ((950, 50), (3, 1), "fr"), ((0, 0), (50, 950), "rf"), ((700, 300), (0, 0), "undetermined"), ((700, 300), (750, 250), "undetermined"),
    ((950, 50), (50, 950), "undetermined (tags and annotation disagree)"), ((950, 50), (500, 500), "undetermined (tags and annotation disagree)"),
    ((950, 50), (700, 300), "undetermined (tags and annotation disagree)"),
    ((10, 2), (0, 0), "undetermined (too little evidence)"), ((0, 0), (0, 0), "undetermined (too little evidence)"),
])
def test_two_sources(tags, ann, want):
    t = _tally(tags, ann)
    assert S.verdict(t.tolist()) == want
    assert sd.decide(t)[0] == want
    got, per, final, notes = S.parse_report(sd.report(t))
    assert got == t.tolist() and final == want and not notes
    for name, (a, b) in (("tags", tags), ("annotation", ann)):
        assert per[name] == (a, b, "%.4f" % (a / (a + b)) if a + b else "NA", S.source_verdict(a, b))


def test_min_evidence_and_the_note():
    t = _tally((95, 5), (0, 0))
    assert sd.decide(t)[0] == "undetermined (too little evidence)" and sd.decide(t, 100)[0] == "fr" and S.verdict(t.tolist(), 100) == "fr"
    t = _tally((0, 0), (1900, 100))
    assert S.parse_report(sd.report(t, 1000, 7))[3] == [sd.XS_HINT] and S.parse_report(sd.report(t, 1000, 0))[3] == []
    assert "intronMotif" in sd.XS_HINT


# ---- the command line -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("argv,match", [
    (["process", "-B", "x.bam", "-o", "x", "-s", "auto", "--strandFromXS"], "alternatives"),
    (["junctions", "-B", "x.bam", "-o", "x.bed", "-s", "auto", "--strandFromXS"], "alternatives"),
    (["process", "-B", "x.bam", "-o", "x", "-s", "auto", "--minEvidence", "-1"], "minEvidence"),
    (["strandedness", "-B", "x.bam", "--minEvidence", "-1"], "minEvidence"),
    (["strandedness", "-o", "r.txt"], "BAMFile"),
    (["strandedness", "-B", "x.bam", "--requireFlags", "0x10", "--excludeFlags", "0x10"], "share a bit"),
])
def test_parser_errors(argv, match, capsys):
    with pytest.raises(SystemExit) as err:
        cli.main(argv)
    assert err.value.code == 2
    assert match in capsys.readouterr().err


def test_auto_is_not_a_strand_for_who_does_not_infer():
    """``combine`` is out of scope: it takes what the user passes, and ``auto`` is neither fr nor rf there."""
    assert "auto" not in native.STRANDED_CODE
    with pytest.raises(ValueError, match="alternatives"):
        from spliser_amd import process as proc
        proc.process("x.bam", None, "x", strandedType="auto", strandFromXS=True)
