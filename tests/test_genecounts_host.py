"""``genecounts`` without a GPU: the gene maps of ``genecounts.gene_maps`` against the gene set under every base; the rule on the host
(``spl_gene_count_rule_host``) against the yardstick of ``genecases.py`` on random reads and on the corner cases, and the rule's
header in a stand-alone program under AddressSanitizer and UBSan (tests/hostsim/genecount_rule_asan.cpp); the annotation reader,
the writer and the command line's refusals."""
import os
import subprocess

import numpy as np
import pytest

import genecases as G
from spliser_amd import cli, genecounts as gc, native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BYTE = {"+": 43, "-": 45, ".": 46}


def _arrays(features):
    return (np.array([f[0] for f in features], np.int64), np.array([f[1] for f in features], np.int64), np.array([BYTE[f[2]] for f in features], np.uint8),
            np.array([f[3] for f in features], np.int64))


def _same_map(got, features, length, which):
    """Every position's code equals the set under it, and an entry exists only where the code changes."""
    start, code = got
    assert start.dtype == np.int32 and code.dtype == np.uint32 and start.shape == code.shape
    start, code = start.tolist(), code.tolist()
    assert all(a < b for a, b in zip(start, start[1:])) and all(a != b for a, b in zip(code, code[1:])) and (not code or code[0] != 0)
    sets = G.sets_per_base(G.select(features, which), length + 2)
    for p in range(length + 2):
        assert G.map_says(start, code, p) == G.code_of_set(sets[p]), p


# ---- the maps -----------------------------------------------------------------------------------------------------------------
NAMED = {
    "nested genes": [(100, 900, "+", 0), (300, 500, "-", 1), (350, 400, "+", 2)],
    "genes that touch": [(100, 200, "+", 0), (200, 300, "+", 1), (300, 400, "-", 0)],
    "one gene's exons overlapping": [(100, 300, "+", 3), (200, 400, "+", 3), (250, 260, "+", 3), (400, 450, "+", 3), (1000, 1100, "+", 3)],
    "one gene's exons overlapping under another gene": [(100, 300, "+", 1), (200, 400, "+", 1), (50, 250, "-", 0), (390, 600, ".", 2)],
    "features without a strand": [(100, 200, ".", 0), (150, 250, "+", 1), (300, 400, ".", 1), (350, 450, "-", 0)],
    "a feature without a base": [(100, 200, "+", 0), (150, 150, "-", 1), (180, 170, "-", 1), (300, 301, "+", 1)],
    "a feature from base 0": [(0, 10, "+", 0), (5, 20, "-", 1)],
    "nothing": [],
}


@pytest.mark.parametrize("name", list(NAMED))
def test_gene_maps_of_named_cases(name):
    features = NAMED[name]
    a, b = gc.gene_maps(*_arrays(features))
    assert b is None
    _same_map(a, features, 1200, None)
    plus, minus = gc.gene_maps(*_arrays(features), stranded=True)
    _same_map(plus, features, 1200, "+")
    _same_map(minus, features, 1200, "-")


@pytest.mark.parametrize("seed", range(6))
def test_gene_maps_of_random_chromosomes(seed):
    rng = np.random.default_rng(500 + seed)
    length = int(rng.integers(200, 5001))
    features = G.random_features(rng, length, int(rng.integers(1, 12)), int(rng.integers(1, 60)))
    a, _ = gc.gene_maps(*_arrays(features))
    _same_map(a, features, length, None)
    plus, minus = gc.gene_maps(*_arrays(features), stranded=True)
    _same_map(plus, features, length, "+")
    _same_map(minus, features, length, "-")
    assert int((a[1] == G.MANY).sum()) > 0 or seed > 2          # (the first seeds do have positions under two genes)


def test_a_feature_beyond_the_coordinate_space_is_the_cover_maps_error():
    from spliser_amd import strandedness as sd
    with pytest.raises(native.SpliserNativeError, match="int32 coordinate space") as mine:
        gc.gene_map([10], [2147483581], [0])
    with pytest.raises(native.SpliserNativeError, match="int32 coordinate space") as theirs:
        sd.cover_map([10], [2147483581], [43])
    assert mine.value.code == theirs.value.code == -6 and str(mine.value) == str(theirs.value)
    start, code = gc.gene_map([10], [2147483580], [0])
    assert start.tolist() == [10, 2147483580] and code.tolist() == [1, 0]


# ---- the rule -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def corner_maps():
    left, right, strand, gene = G.corner_arrays()
    a, _ = gc.gene_maps(left, right, strand, gene)
    plus, minus = gc.gene_maps(left, right, strand, gene, stranded=True)
    assert a[0].shape[0] >= 3000
    return a, plus, minus


def test_the_corner_cases_say_what_the_issue_says():
    """The yardstick itself, on the cases whose answer can be read off the rule."""
    bases = G.corner_bases(0)
    for name, flag, pos, cigar, want in G.CORNERS:
        assert G.result_of(flag, pos, G.ops(cigar).tolist(), bases) == want, name
    fr, rf = G.corner_bases(1), G.corner_bases(2)
    for flag in G.STRAND_FLAGS:
        plus = G.fr_strand(flag) == "+"
        assert (flag in (0, 99, 147)) == plus
        # gX is '+', gY has no strand: a '+' read sees both (ambiguous), a '-' read gY alone; g1 is '-': a '+' read sees nothing there
        assert G.result_of(flag, 3061, G.ops("10M").tolist(), fr, 1) == (G.AMBIGUOUS if plus else 7)
        assert G.result_of(flag, 3061, G.ops("10M").tolist(), rf, 2) == (7 if plus else G.AMBIGUOUS)
        assert G.result_of(flag, 311, G.ops("10M").tolist(), fr, 1) == (G.NO_FEATURE if plus else 1)
        assert G.result_of(flag, 311, G.ops("10M").tolist(), rf, 2) == (1 if plus else G.NO_FEATURE)


@pytest.mark.parametrize("stranded", [0, 1, 2])
def test_rule_on_the_corner_cases(corner_maps, stranded):
    a, plus, minus = corner_maps
    bases = G.corner_bases(stranded)
    seen = set()
    for name, flag, pos, cigar, _ in G.CORNERS:
        o = G.ops(cigar)
        want = G.result_of(flag, pos, o.tolist(), bases, stranded)
        got = native.gene_count_rule_host(flag, pos, o, len(G.CORNER_IDS), plus if stranded else a, minus if stranded else None, stranded)
        assert got == want, name
        seen.add(want)
    assert {G.NO_FEATURE, G.AMBIGUOUS, G.NOT_COUNTED, 8} <= seen and (stranded == 2 or 0 in seen)      # (g0 is '+', its reads there '-' under rf)


@pytest.mark.parametrize("seed", range(4))
def test_rule_on_random_reads_and_features(seed):
    rng = np.random.default_rng(900 + seed)
    length, n_genes = 5000, 9
    features = G.random_features(rng, length - 600, n_genes, 14 + 8 * seed)
    recs = G.random_records(rng, 700, length - 600)
    arrays = _arrays(features)
    maps = {0: gc.gene_maps(*arrays), 1: gc.gene_maps(*arrays, stranded=True)}
    maps[2] = maps[1]
    for stranded, shift in ((0, 0), (1, 0), (2, 0), (0, 37)):
        moved = [(l + shift, r + shift, s, g) for l, r, s, g in features]
        bases = {w: G.bases_of_features(moved, length, w) for w in "+-"} if stranded else G.bases_of_features(moved, length)
        a, b = maps[stranded]
        if shift:
            a = (a[0] + shift, a[1])
        seen = set()
        for flag, pos, cigar in recs:
            o = G.ops(cigar)
            want = G.result_of(flag, pos, o.tolist(), bases, stranded, shift)
            assert native.gene_count_rule_host(flag, pos, o, n_genes, a, b, stranded, shift) == want, (flag, pos, cigar, stranded)
            seen.add(min(want, 0))
        assert seen == {0, G.NO_FEATURE, G.AMBIGUOUS, G.NOT_COUNTED}


def test_rule_with_maps_of_no_entry_and_of_one():
    o = G.ops("20M")
    assert native.gene_count_rule_host(0, 100, o, 3, None) == G.NO_FEATURE
    assert native.gene_count_rule_host(4, 100, o, 3, None) == G.NOT_COUNTED
    one = (np.array([110], np.int32), np.array([3], np.uint32))          # gene 2 from base 110 to the end
    assert native.gene_count_rule_host(0, 91, o, 3, one) == G.NO_FEATURE and native.gene_count_rule_host(0, 92, o, 3, one) == 2
    assert native.gene_count_rule_host(0, 2000000000, o, 3, one) == 2
    assert native.gene_count_rule_host(16, 92, o, 3, one, None, 1) == G.NO_FEATURE          # the '-' read's map has no entry


def test_rule_refusals():
    o = G.ops("20M")
    for bad, match in (((np.array([30, 20], np.int32), np.array([1, 2], np.uint32)), "ascending"), ((np.array([20, 20], np.int32), np.array([1, 2], np.uint32)), "ascending"),
                       ((np.array([20, 30], np.int32), np.array([1, 4], np.uint32)), "code")):
        for maps in ((bad, None), (None, bad)):
            with pytest.raises(native.SpliserNativeError, match=match) as err:
                native.gene_count_rule_host(0, 10, o, 3, *maps)
            assert err.value.code == -1
    with pytest.raises(native.SpliserNativeError, match="stranded"):
        native.gene_count_rule_host(0, 10, o, 3, None, None, 3)
    fine = (np.array([20, 25], np.int32), np.array([3, G.MANY], np.uint32))          # the greatest code there is, and "many"
    assert native.gene_count_rule_host(0, 10, G.ops("12M"), 3, fine) == 2 and native.gene_count_rule_host(0, 10, o, 3, fine) == G.AMBIGUOUS


def test_header_under_the_sanitizers(tmp_path, corner_maps):
    """The rule's header alone in a program of its own: ops and maps in heap blocks of exactly their size, so that a read beyond
    either aborts the child.  Cases as lines "flag pos shift stranded | ops | a starts | a codes | b starts | b codes"."""
    exe = str(tmp_path / "genecount_asan")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "hostsim", "genecount_rule_asan.cpp"), "-o", exe])
    a, plus, minus = corner_maps
    text_of = lambda v: " ".join(str(int(x)) for x in v)
    lines, want = [], []
    for stranded in (0, 1, 2):
        ma, mb = (plus, minus) if stranded else (a, (np.zeros(0, np.int32), np.zeros(0, np.uint32)))
        bases = G.corner_bases(stranded)
        for name, flag, pos, cigar, _ in G.CORNERS:
            o = G.ops(cigar)
            lines.append("%d %d 0 %d|%s|%s|%s|%s|%s" % (flag, pos, stranded, text_of(o), text_of(ma[0]), text_of(ma[1]), text_of(mb[0]), text_of(mb[1])))
            want.append(G.result_of(flag, pos, o.tolist(), bases, stranded))
    # a map of one entry and of none, a read at the top of the coordinate space with a shift on top: int64 throughout
    lines.append("0 2147483000 500000 0|%s|2147483500|2||" % text_of(G.ops("1000M")))
    want.append(1)
    lines.append("0 5 0 0|%s||||" % text_of(G.ops("10M")))
    want.append(G.NO_FEATURE)
    out = subprocess.run([exe], input="\n".join(lines) + "\n", stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0"))
    assert out.returncode == 0, out.stderr
    assert [int(v) for v in out.stdout.split()] == want


# ---- the reader ---------------------------------------------------------------------------------------------------------------
GTF = "\n".join([
    "#!genome-build test",
    'c1\tsrc\tgene\t101\t900\t.\t+\t.\tgene_id "gB"; gene_name "B";',
    'c1\tsrc\texon\t101\t200\t.\t+\t.\tgene_id "gB"; transcript_id "t1"; gene_name "B";',
    'c1\tsrc\texon\t301\t400\t.\t+\t.\ttranscript_id "t1"; gene_id "gB";',
    'c2\tsrc\texon\t11\t20\t.\t-\t.\tgene_id "gA"; gene_id_version "7"',
    "c2\tsrc\texon\t51\t60\t.\t.\t.\tID=e9;gene_id=gC;Parent=t3",
    'c2\tsrc\texon\t71\t70\t.\t-\t.\tgene_version "2"; gene_id gB',
    "c2\tsrc\tCDS\t81\t90\t.\t-\t0\tID=cds1;Parent=t9;Name=gD",
    "c2\tsrc\texon\t81",
    "",
])


def test_reader_on_gtf_and_gff3_syntax(tmp_path):
    path = str(tmp_path / "a.gtf")
    open(path, "w").write(GTF)
    f = gc.read_features(path)
    ids, by_chrom = G.features_of_text(GTF)
    assert f.ids == ids == ["gA", "gB", "gC"] and f.chroms == ["c1", "c2"]
    for chrom, rows in by_chrom.items():
        left, right, strand, gene = f.arrays(chrom)
        assert list(zip(left.tolist(), right.tolist(), [chr(s) for s in strand.tolist()], gene.tolist())) == rows
    assert by_chrom["c2"] == [(10, 20, "-", 0), (50, 60, ".", 2), (70, 70, "-", 1)]          # 0-based, half-open; quotes stripped; the empty feature is a feature
    assert f.genes_on("c2").tolist() == [0, 1, 2] and f.genes_on("c1").tolist() == [1] and f.genes_on("c9").tolist() == []
    cds = gc.read_features(path, "CDS", "Name")                     # -t other than exon, another attribute
    assert cds.ids == ["gD"] and [a.tolist() for a in cds.arrays("c2")] == [[80], [90], [45], [0]]
    genes = gc.read_features(path, "gene")
    assert genes.ids == ["gB"] and genes.arrays("c1")[1].tolist() == [900]


def test_reader_names_the_line_of_a_feature_without_the_attribute(tmp_path):
    path = str(tmp_path / "bad.gtf")
    text = GTF + 'c3\tsrc\texon\t5\t9\t.\t+\t.\ttranscript_id "t4"; gene_name "E";\n'
    open(path, "w").write(text)
    with pytest.raises(ValueError, match="line 10"):
        G.features_of_text(text)
    with pytest.raises(native.SpliserNativeError, match=r"line 10: .*gene_id") as err:
        gc.read_features(path)
    assert err.value.code == -5
    with pytest.raises(native.SpliserNativeError, match="line 5: .*transcript_id"):
        gc.read_features(path, "exon", "transcript_id")
    assert gc.read_features(path, "CDS", "Name").ids == ["gD"]      # a type whose lines all have the attribute reads on


# ---- the writer ---------------------------------------------------------------------------------------------------------------
def test_writer_order_zeros_and_one_chromosome(tmp_path):
    ids = ["a1", "a10", "a2", "b"]
    counts = np.array([5, 0, 70000000000, 0, 11, 2, 3], np.int64)
    path = str(tmp_path / "x.genecounts.tsv")
    assert gc.write_counts(path, ids, counts) == 4
    text = open(path).read()
    assert text == "a1\t5\na10\t0\na2\t70000000000\nb\t0\n__no_feature\t11\n__ambiguous\t2\n__not_counted\t3\n" == G.file_text(ids, counts.tolist())
    assert gc.write_counts(path, ids, counts, only=np.array([1, 2])) == 2
    assert open(path).read() == "a10\t0\na2\t70000000000\n__no_feature\t11\n__ambiguous\t2\n__not_counted\t3\n" == G.file_text(ids, counts.tolist(), only={1, 2})
    assert gc.SUFFIX == ".genecounts.tsv" and gc.SPECIALS == G.SPECIALS


# ---- the command line ---------------------------------------------------------------------------------------------------------
def test_parser_results():
    p = cli.build_parser()
    a = vars(p.parse_args(["genecounts", "-B", "x.bam", "-A", "g.gtf", "-o", "out"]))
    assert (a["inBAM"], a["annotationFile"], a["outputPath"], a["aType"], a["idAttr"], a["qChrom"], a["isStranded"], a["strandedType"]) == \
        ("x.bam", "g.gtf", "out", "exon", "gene_id", "All", False, None)
    assert (a["anyOrder"], a["gpuDecode"], a["minMapQ"], a["requireFlags"], a["excludeFlags"], a["gpus"], a["devices"], a["threads"]) == (False, None, 0, 0, 0, 1, None, 0)
    a = vars(p.parse_args(["genecounts", "-B", "x.sam.gz", "-A", "g.gff", "-o", "out", "-t", "CDS", "--idAttr", "Parent", "-c", "chr2", "--isStranded", "-s", "rf", "--anyOrder",
                           "--hostDecode", "--minMapQ", "255", "--requireFlags", "0x2", "--excludeFlags", "0x400", "--gpus", "2", "--threads", "4"]))
    assert (a["aType"], a["idAttr"], a["qChrom"], a["isStranded"], a["strandedType"], a["anyOrder"], a["gpuDecode"]) == ("CDS", "Parent", "chr2", True, "rf", True, False)
    assert (a["minMapQ"], a["requireFlags"], a["excludeFlags"], a["gpus"], a["threads"]) == (255, 2, 0x400, 2, 4)
    assert vars(p.parse_args(["genecounts", "-B", "x", "-A", "g", "-o", "o", "--gpuDecode", "--devices", "0,1"]))["gpuDecode"] is True
    assert "geneCounts" not in vars(p.parse_args(["process", "-B", "x", "-o", "o"]))          # (process has no such flag)


@pytest.mark.parametrize("argv, match", [
    (["genecounts", "-B", "x.bam", "-o", "o"], "-A is required"),
    (["genecounts", "-B", "x.bam", "-A", "g.gtf", "-o", "o", "-s", "auto"], "-s auto is not taken here: the `strandedness` command"),
    (["genecounts", "-B", "x.bam", "-A", "g.gtf", "-o", "o", "--isStranded", "-s", "auto"], "-s auto is not taken here"),
    (["genecounts", "-B", "x.bam", "-A", "g.gtf", "-o", "o", "--isStranded"], "--isStranded requires parameter --strandedType/-s as fr or rf"),
    (["genecounts", "-B", "x.bam", "-A", "g.gtf", "-o", "o", "--isStranded", "-s", "ff"], "must be fr or rf"),
    (["genecounts", "-B", "x.bam", "-A", "g.gtf", "-o", "o", "--minMapQ", "256"], "minMapQ"),
    (["genecounts", "-B", "x.bam", "-A", "g.gtf", "-o", "o", "--requireFlags", "4", "--excludeFlags", "0x4"], "share a bit"),
    (["genecounts", "-A", "g.gtf", "-o", "o"], "-B"),
    (["genecounts", "-B", "x.bam", "-A", "g.gtf"], "-o"),
    (["process", "-B", "x.bam", "-o", "o", "--geneCounts"], "unrecognized"),
])
def test_parser_errors(argv, match, capsys):
    with pytest.raises(SystemExit) as err:
        cli.main(argv)
    assert err.value.code == 2
    assert match in capsys.readouterr().err


def test_the_function_refuses_what_the_parser_refuses():
    with pytest.raises(ValueError, match="-A"):
        gc.genecounts("x.bam", None, "o")
    with pytest.raises(ValueError, match="-s fr or -s rf"):
        gc.genecounts("x.bam", "g.gtf", "o", isStranded=True, strandedType="auto")
