"""``intronretention`` on the host: the intron and piece tables (``intronretention.Table``, numpy sorts and searches) and the rule for
one intron (``spl_intron_depth_host``: pairs collected, sorted and walked) against the yardstick of ``introncases.py``; the rule
header in a stand-alone program under AddressSanitizer and UBSan (tests/hostsim/intron_rule_asan.cpp); ids, ranks, ``-c`` and the
file byte for byte; the command line.  No GPU."""
import os
import re
import subprocess

import numpy as np
import pytest

import introncases as I
from spliser_amd import cli, genecounts as gc, intronretention as ir, native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# name -> (ids, chromosomes in the annotation's order, {chrom: [(left, right, strand, gene index)]}, {chrom: LN})
NAMED = {
    "a nested gene": (["gA", "gB"], ["c1"], {"c1": [(100, 200, "+", 0), (400, 500, "+", 0), (250, 300, "+", 1)]}, {"c1": 1000}),
    "abutting exons": (["gA"], ["c1"], {"c1": [(100, 200, "+", 0), (200, 300, "+", 0), (400, 500, "+", 0), (450, 480, "+", 0)]}, {"c1": 1000}),
    "a gene on two chromosomes": (["gA", "gB"], ["c2", "c1"], {"c2": [(5, 10, "+", 0), (50, 60, "+", 0), (1, 3, "-", 1), (70, 80, "-", 1)],
                                                              "c1": [(30, 40, "+", 0), (10, 20, "+", 0), (60, 90, "+", 0)]}, {"c1": 100, "c2": 100}),
    "a . gene under stranded": (["gA", "gB"], ["c1"], {"c1": [(100, 200, ".", 0), (400, 500, ".", 0), (300, 320, "-", 1), (340, 350, "-", 1)]}, {"c1": 1000}),
    "a mixed-strand gene": (["gA"], ["c1"], {"c1": [(100, 200, "+", 0), (300, 400, "-", 0), (500, 600, "+", 0), (700, 800, "-", 0)]}, {"c1": 1000}),
    "an intron wholly covered by another gene": (["gA", "gB"], ["c1"], {"c1": [(100, 200, "+", 0), (300, 400, "+", 0), (150, 350, "+", 1)]}, {"c1": 1000}),
    "a piece clipped by LN": (["gA"], ["c1"], {"c1": [(100, 200, "+", 0), (400, 500, "+", 0), (900, 950, "+", 0)]}, {"c1": 300}),
    "a chromosome without a length": (["gA"], ["c1"], {"c1": [(100, 200, "+", 0), (400, 500, "+", 0)]}, {}),
}


def features_of(ids, chroms, by_chrom):
    arrays = {}
    for chrom in chroms:
        f = by_chrom[chrom]
        arrays[chrom] = (np.array([x[0] for x in f], np.int64), np.array([x[1] for x in f], np.int64), np.array([ord(x[2]) for x in f], np.uint8), np.array([x[3] for x in f], np.int64))
    return gc.Features(list(ids), list(chroms), arrays)


def check_tables(ids, chroms, by_chrom, lengths):
    """The table's introns and pieces per chromosome and track, and the file of a run without a read, against the yardstick."""
    for stranded in (False, True):
        table = ir.Table(features_of(ids, chroms, by_chrom), stranded)
        n = table.gene.shape[0]
        numbers = np.zeros((n, 4), np.int64)
        for chrom in chroms:
            for track in I.tracks_of(stranded):
                rows = table.rows_on(chrom, track)
                off, start, end = table.pieces(rows, chrom, track, lengths.get(chrom))
                got = [(int(table.gene[r]), int(table.s[r]), int(table.e[r]), list(zip(start[off[k]:off[k + 1]].tolist(), end[off[k]:off[k + 1]].tolist()))) for k, r in enumerate(rows)]
                assert got == I.introns_of(by_chrom[chrom], track, lengths.get(chrom)), (chrom, track)
                numbers[rows] = ir.no_read_numbers(off, start, end, 30)
        want = I.rows_of(ids, chroms, by_chrom, stranded, 30, lengths, {}, {})
        assert len(want) == n
        yield stranded, table, numbers, want


@pytest.mark.parametrize("name", sorted(NAMED))
def test_named_cases(name, tmp_path):
    for stranded, table, numbers, want in check_tables(*NAMED[name]):
        path = str(tmp_path / ("s%d.tsv" % stranded))
        ir.write_rows(path, table, np.arange(table.gene.shape[0]), numbers, np.zeros((table.gene.shape[0], 3), np.int64))
        assert open(path).read() == I.file_text(want)


def test_what_the_named_cases_say():
    """Read off the rule, not off either implementation."""
    first = lambda name, stranded: [(r[0], r[2], r[3], r[4], r[5], r[6]) for r in I.rows_of(*NAMED[name][:3], stranded, 0, NAMED[name][3], {}, {})]
    assert first("a nested gene", False) == [("gA:I001", "c1", "201", "400", ".", "150")]
    assert first("abutting exons", False) == [("gA:I001", "c1", "301", "400", ".", "100")]
    assert first("a gene on two chromosomes", False) == [("gA:I001", "c2", "11", "50", ".", "40"), ("gA:I002", "c1", "21", "30", ".", "10"), ("gA:I003", "c1", "41", "60", ".", "20"),
                                                         ("gB:I001", "c2", "4", "70", ".", "52")]
    assert first("a . gene under stranded", True) == [("gA:I001", "c1", "201", "400", "+", "200"), ("gA:I002", "c1", "201", "400", "-", "170"), ("gB:I001", "c1", "321", "340", "-", "20")]
    assert first("a mixed-strand gene", True) == [("gA:I001", "c1", "201", "500", "+", "300"), ("gA:I002", "c1", "401", "700", "-", "300")]
    assert first("a mixed-strand gene", False) == [("gA:I001", "c1", "201", "300", ".", "100"), ("gA:I002", "c1", "401", "500", ".", "100"), ("gA:I003", "c1", "601", "700", ".", "100")]
    assert first("an intron wholly covered by another gene", False) == [("gA:I001", "c1", "201", "300", ".", "0")]
    assert first("a piece clipped by LN", False) == [("gA:I001", "c1", "201", "400", ".", "100"), ("gA:I002", "c1", "501", "900", ".", "0")]
    row = I.rows_of(*NAMED["an intron wholly covered by another gene"][:3], False, 30, {"c1": 1000}, {}, {})[0]
    assert row[6:] == ("0", "0", "0", "0", "NA", "0", "0", "0", "NA")


def test_random_chromosomes():
    import genecases as G
    rng = np.random.default_rng(4711)
    for _ in range(12):
        length = int(rng.integers(200, 500))
        n_genes = int(rng.integers(1, 7))
        chroms = ["cB", "cA"]
        by_chrom = {c: G.random_features(rng, length, n_genes, int(rng.integers(2, 25))) for c in chroms}
        ids = ["g%d" % k for k in range(n_genes)]
        for _ in check_tables(ids, chroms, by_chrom, {"cB": length - 50}):
            pass


def test_rule_on_the_host_against_the_sorted_expansion():
    rng = np.random.default_rng(99)
    for n_bound, max_depth in ((0, 1), (1, 2), (12, 3), (80, 50), (80, 2 ** 32 - 1)):
        length = 300
        pos, depth = I.random_bounds(rng, length, n_bound, max_depth)
        per_base = I.depth_per_base(pos, depth, length)
        for _ in range(30):
            pieces = I.random_pieces(rng, length, int(rng.integers(1, 6)))
            for trim in (0, 30, 49):
                got = native.intron_depth_host(pos, depth, [p[0] for p in pieces], [p[1] for p in pieces], trim)
                assert tuple(got) == I.stats_of(per_base, pieces, trim) == I.stats_of_runs(pos, depth, pieces, trim)


def test_rule_on_the_host_few_bases_ties_and_the_greatest_depth():
    top = 2 ** 32 - 1
    pos, depth = [0, 1, 2], [4, 0, top]
    for pieces in ([], [(0, 1)], [(0, 2)], [(0, 3)], [(1, 2)], [(0, 1), (2, 3)]):
        for trim in (0, 30, 49):
            assert tuple(native.intron_depth_host(pos, depth, [p[0] for p in pieces], [p[1] for p in pieces], trim)) == I.stats_of([4, 0, top], pieces, trim)
    # ties that straddle lo and hi: D = 2 2 2 9 9 9 9 300 300 300
    assert native.intron_depth_host([0, 3, 7], [2, 9, 300], [0], [10], 30) == [10, 10, 4, 36]
    assert native.intron_depth_host([0, 3, 7], [2, 9, 300], [0], [10], 20) == [10, 10, 6, 338]
    assert native.intron_depth_host([0], [top], [0], [1000], 0) == [1000, 1000, 1000, 1000 * top]
    assert native.intron_depth_host([], [], [5], [10], 49) == [5, 0, 1, 0]


def test_refusals_of_the_host_rule():
    fine = ([0, 10], [1, 2], [0], [5])
    for args, match in ((([0, 0], [1, 2], [0], [5], 30), "boundaries are not strictly ascending at entry 1"), (([5, 3], [1, 2], [0], [5], 30), "strictly ascending"),
                        ((fine[0], fine[1], [5], [5], 30), "piece 0 ends at or before its start"), ((fine[0], fine[1], [-1], [5], 30), "outside"),
                        ((fine[0], fine[1], [0, 4], [5, 9], 30), "not strictly ascending and disjoint at piece 1"), ((fine[0], fine[1], [6, 0], [9, 5], 30), "disjoint"),
                        (fine + (50,), "trim_percent must be in 0 .. 49, not 50"), (fine + (-1,), "trim_percent")):
        with pytest.raises(native.SpliserNativeError, match=match) as err:
            native.intron_depth_host(*args)
        assert err.value.code == -1 and str(err.value).count("spl_intron_depth_host") == 1          # the text names the call, no context involved
    assert native.intron_depth_host(*fine) == [5, 5, 3, 3]                                           # abutting pieces are fine: [0, 5) [5, 9)
    assert native.intron_depth_host(fine[0], fine[1], [0, 5], [5, 9], 0) == [9, 9, 9, 9]


def test_the_threshold_the_tests_straddle_is_the_kernel_s():
    text = open(os.path.join(ROOT, "spliser_amd", "csrc", "spl_intron.h")).read()
    assert int(re.search(r"#define SPL_INTRON_LONG_BASES (\d+)", text).group(1)) == native.INTRON_LONG_BASES


def test_header_under_the_sanitizers(tmp_path):
    """The rule's header alone in a program of its own: boundaries and pieces in heap blocks of exactly their size, so that an
    access beyond any aborts the child."""
    exe = str(tmp_path / "intron_asan")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "hostsim", "intron_rule_asan.cpp"), "-o", exe])
    rng = np.random.default_rng(5)
    text_of = lambda v: " ".join(str(int(x)) for x in v)
    lines, want = [], []
    length = 400
    for n_bound, max_depth in ((0, 1), (1, 5), (40, 9), (150, 2 ** 32 - 1)):
        pos, depth = I.random_bounds(rng, length, n_bound, max_depth)
        per_base = I.depth_per_base(pos, depth, length)
        for k in range(40):
            pieces = I.random_pieces(rng, length, int(rng.integers(1, 6))) if k else []
            trim = (0, 30, 49)[k % 3]
            lines.append("%d %d|%s|%s|%s|%s" % (trim, length, text_of(pos), text_of(depth), text_of(p[0] for p in pieces), text_of(p[1] for p in pieces)))
            want.append("%d %d %d %d" % I.stats_of(per_base, pieces, trim))
    lines += ["30 2147483646|0 2147483645|4294967295 1|0|2147483646", "0 400|3 3|1 1|0|9", "0 400|||5 2|9 7", "0 400|||5|401", "0 400|||5|5"]
    want += ["2147483646 2147483646 858993460 %d" % (858993460 * 4294967295), "bound 1", "flaw 1 2", "flaw 0 1", "flaw 0 0"]
    done = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert done.returncode == 0, done.stderr[-2000:]
    assert done.stdout.split("\n")[:-1] == want


def test_splice_counts_against_the_loop():
    rng = np.random.default_rng(3)
    n = 200
    left, right = rng.integers(0, 30, n), rng.integers(30, 60, n)
    rows = sorted({(int(l), int(r), "+-"[int(s)]): int(c) for l, r, s, c in zip(left, right, rng.integers(0, 2, n), rng.integers(1, 2 ** 31, n))}.items())
    table = dict(left=np.array([k[0] for k, _ in rows], np.int32), right=np.array([k[1] for k, _ in rows], np.int32), strand=np.array([ord(k[2]) for k, _ in rows], np.uint8),
                 count=np.array([c for _, c in rows], np.uint32))
    flat = [(k[0], k[1], k[2], c) for k, c in rows]
    s, e = np.arange(0, 32, dtype=np.int64), np.arange(28, 60, dtype=np.int64)
    for stranded, track in ((0, "."), (1, "+"), (2, "-")):
        got = ir.splice_counts(table, s, e, track, stranded)
        assert got.tolist() == [list(I.splice_of(flat, int(a), int(b), track, stranded)) for a, b in zip(s, e)]
    none = dict(left=np.zeros(0, np.int32), right=np.zeros(0, np.int32), strand=np.zeros(0, np.uint8), count=np.zeros(0, np.uint32))
    assert ir.splice_counts(none, s, e, ".", 0).tolist() == [[0, 0, 0]] * 32


def test_file_with_depths_and_junctions_byte_for_byte(tmp_path):
    """ids, ranks, -c and every column: the numbers from the host rule per intron, the splice sums from the join."""
    ids, chroms, by_chrom, lengths = NAMED["a gene on two chromosomes"]
    rng = np.random.default_rng(8)
    for stranded in (0, 1):
        table = ir.Table(features_of(ids, chroms, by_chrom), bool(stranded))
        n = table.gene.shape[0]
        bounds = {(c, t): I.random_bounds(rng, lengths[c], 25, 9) for c in chroms for t in I.tracks_of(stranded)}
        depths = {k: I.depth_per_base(v[0], v[1], lengths[k[0]]) for k, v in bounds.items()}
        junctions = {"c2": [(10, 50, "+", 7), (10, 60, "+", 2), (3, 70, "-", 5), (3, 70, "+", 1), (4, 50, "+", 11)], "c1": [(20, 30, "+", 3), (20, 30, "-", 4)]}
        numbers, splices = np.zeros((n, 4), np.int64), np.zeros((n, 3), np.int64)
        for c in chroms:
            j = junctions[c]
            as_table = dict(left=np.array([r[0] for r in j], np.int32), right=np.array([r[1] for r in j], np.int32), strand=np.array([ord(r[2]) for r in j], np.uint8),
                            count=np.array([r[3] for r in j], np.uint32))
            for t in I.tracks_of(stranded):
                rows = table.rows_on(c, t)
                off, start, end = table.pieces(rows, c, t, lengths[c])
                for k, r in enumerate(rows):
                    numbers[r] = native.intron_depth_host(bounds[(c, t)][0], bounds[(c, t)][1], start[off[k]:off[k + 1]], end[off[k]:off[k + 1]], 30)
                splices[rows] = ir.splice_counts(as_table, table.s[rows], table.e[rows], t, stranded)
        for only in (None, "c1", "c2"):
            keep = np.arange(n) if only is None else np.flatnonzero(table.chrom == chroms.index(only))
            path = str(tmp_path / "out.tsv")
            assert ir.write_rows(path, table, keep, numbers[keep], splices[keep]) == keep.shape[0]
            want = I.file_text(I.rows_of(ids, chroms, by_chrom, stranded, 30, lengths, depths, junctions, only))
            assert open(path).read() == want
            assert only is None or all(line.split("\t")[2] == only for line in want.split("\n")[1:-1])
    assert I.ratio_texts(4, 10, 3, 1) == ("2.5", repr(2.5 / 5.5)) and I.ratio_texts(4, 0, 0, 0) == ("0.0", "NA") and I.ratio_texts(0, 0, 5, 5) == ("NA", "NA")
    assert ir.ratio_texts(4, 10, 3, 1) == ("2.5", repr(2.5 / 5.5)) and ir.ratio_texts(4, 0, 0, 0) == ("0.0", "NA") and ir.ratio_texts(0, 0, 5, 5) == ("NA", "NA")


def test_parser():
    p = cli.build_parser()
    a = vars(p.parse_args(["intronretention", "-B", "x.bam", "-A", "g.gtf", "-o", "out"]))
    assert (a["command"], a["inBAM"], a["annotationFile"], a["outputPath"], a["aType"], a["idAttr"], a["trimPercent"], a["qChrom"], a["isStranded"], a["strandedType"], a["gpuDecode"],
            a["anyOrder"], a["minMapQ"], a["requireFlags"], a["excludeFlags"]) == ("intronretention", "x.bam", "g.gtf", "out", "exon", "gene_id", 30, "All", False, None, None, False, 0, 0, 0)
    a = vars(p.parse_args(["intronretention", "-B", "x.sam", "-A", "g.gff", "-o", "o", "-t", "CDS", "--idAttr", "Parent", "--trimPercent", "0", "-c", "Chr2", "--isStranded", "-s", "rf",
                           "--hostDecode", "--anyOrder", "--excludeFlags", "0x900", "--minMapQ", "3"]))
    assert (a["aType"], a["idAttr"], a["trimPercent"], a["qChrom"], a["isStranded"], a["strandedType"], a["gpuDecode"], a["anyOrder"], a["excludeFlags"], a["minMapQ"]) == (
        "CDS", "Parent", 0, "Chr2", True, "rf", False, True, 0x900, 3)


@pytest.mark.parametrize("extra, said", [(["--isStranded", "-s", "auto"], "auto"), (["--trimPercent", "50"], "trimPercent"), (["--trimPercent", "-1"], "trimPercent"),
                                         (["--isStranded"], "strandedType"), (["--isStranded", "-s", "ff"], "fr or rf"), (["--minMapQ", "256"], "minMapQ")])
def test_parser_errors(extra, said, capsys):
    with pytest.raises(SystemExit) as err:
        cli.main(["intronretention", "-B", "x.bam", "-A", "g.gtf", "-o", "out"] + extra)
    assert err.value.code == 2 and said in capsys.readouterr().err


def test_an_annotation_is_required(capsys):
    with pytest.raises(SystemExit):
        cli.main(["intronretention", "-B", "x.bam", "-o", "out"])
    assert "annotationFile" in capsys.readouterr().err
    with pytest.raises(ValueError, match="trimPercent"):
        ir.intronretention("x.bam", "g.gtf", "out", trimPercent=50)
