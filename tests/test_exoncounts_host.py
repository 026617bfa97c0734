"""``exoncounts`` on the host: the bin maps (``exoncounts.exon_maps``, numpy sorts and sums) and the per-read rule
(``spl_exon_count_rule_host``, the kernel's own header compiled for the host) against the yardstick of ``exoncases.py``; the rule
header in a stand-alone program under AddressSanitizer and UBSan (tests/hostsim/exoncount_rule_asan.cpp); ids, ranks and both
writers byte for byte; the command line.  No GPU."""
import os
import subprocess

import numpy as np
import pytest

import exoncases as X
import genecases as G
from spliser_amd import cli, exoncounts as xc, genecounts as gc, native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BYTE = {"+": 43, "-": 45, ".": 46}
LENGTH = 400


def _arrays(features):
    return (np.array([f[0] for f in features], np.int64), np.array([f[1] for f in features], np.int64), np.array([BYTE[f[2]] for f in features], np.uint8),
            np.array([f[3] for f in features], np.int64))


def _labels(features, length, stranded):
    return {w: X.labels_of_features(features, length, w) for w in "+-"} if stranded else X.labels_of_features(features, length)


def check_maps(features, length=LENGTH, stranded=False):
    """``exon_maps`` of these features says under every base what the yardstick says, in the shape the rule gives a map.
    -> (map a, map b, the bins)."""
    a, b, (bin_gene, bin_start, bin_end) = xc.exon_maps(*_arrays(features), stranded=stranded)
    labels = _labels(features, length, stranded)
    sets = [labels["+"], labels["-"]] if stranded else [labels]
    bins = X.bins_of(sets)
    assert list(zip(bin_start.tolist(), bin_end.tolist(), bin_gene.tolist())) == bins
    assert (b is None) == (not stranded)
    for (start, code), lab in zip([a, b] if stranded else [a], sets):
        assert start.dtype == np.int32 and code.dtype == np.uint32 and start.shape == code.shape
        assert (np.diff(start.astype(np.int64)) > 0).all() and (code[1:] != code[:-1]).all()          # an entry only where the code changes
        assert not start.shape[0] or (code[0] != 0 and code[-1] == 0)
        for p in range(-1, length + 1):
            at = lab.at(p)
            want = 0 if at is None else G.MANY if at == X.SHARED else bins.index(at[1]) + 1
            assert G.map_says(start, code, p) == want, p
    return a, b, bins


CASES = {
    "abutting exons of one gene are two bins": [(10, 20, "+", 0), (20, 30, "+", 0)],
    "nested and identical exons": [(10, 50, "+", 0), (20, 30, "+", 0), (10, 50, "+", 0), (60, 70, "-", 1), (60, 70, "-", 1)],
    "two genes overlapping on one strand": [(10, 30, "+", 0), (20, 40, "+", 1)],
    "two genes overlapping on opposite strands": [(10, 30, "+", 0), (20, 40, "-", 1)],
    "a gene inside another's exon, and one's exons around the other's": [(10, 90, "+", 2), (30, 40, "+", 0), (100, 110, "-", 1), (120, 130, "+", 0), (140, 150, "-", 1)],
    "a . feature alone": [(10, 30, ".", 0)],
    "a . feature cut by a + feature": [(10, 30, ".", 0), (15, 20, "+", 0)],
    "zero-length and inverted features": [(10, 10, "+", 0), (30, 20, "+", 1), (40, 50, "+", 1), (45, 45, "-", 0)],
    "no feature": [],
    "features of one strand only": [(10, 30, "+", 0), (30, 35, "+", 1)],
    "three genes on one base": [(10, 30, "+", 0), (20, 40, "-", 1), (25, 26, ".", 2)],
}


@pytest.mark.parametrize("stranded", [False, True])
@pytest.mark.parametrize("name", sorted(CASES))
def test_exon_maps_of_named_cases(name, stranded):
    check_maps(CASES[name], stranded=stranded)


def test_what_the_named_cases_come_to():
    _, _, bins = check_maps(CASES["abutting exons of one gene are two bins"])
    assert bins == [(10, 20, 0), (20, 30, 0)]
    _, _, bins = check_maps(CASES["nested and identical exons"])
    assert bins == [(10, 20, 0), (20, 30, 0), (30, 50, 0), (60, 70, 1)]                     # the same exon in two transcripts is one bin
    a, _, bins = check_maps(CASES["two genes overlapping on one strand"])
    assert bins == [(10, 20, 0), (30, 40, 1)] and a[1].tolist() == [1, G.MANY, 2, 0]
    a, b, bins = check_maps(CASES["two genes overlapping on opposite strands"], stranded=True)
    assert bins == [(10, 30, 0), (20, 40, 1)] and a[1].tolist() == [1, 0] and b[1].tolist() == [2, 0]
    a, b, bins = check_maps(CASES["a . feature alone"], stranded=True)
    assert bins == [(10, 30, 0)] and a[1].tolist() == b[1].tolist() == [1, 0]              # one bin from both maps
    a, b, bins = check_maps(CASES["a . feature cut by a + feature"], stranded=True)
    assert bins == [(10, 15, 0), (10, 30, 0), (15, 20, 0), (20, 30, 0)] and a[1].tolist() == [1, 3, 4, 0] and b[1].tolist() == [2, 0]
    a, b, bins = check_maps(CASES["features of one strand only"], stranded=True)
    assert b[0].shape[0] == 0 and len(bins) == 2                                            # an empty selection
    a, _, bins = check_maps(CASES["no feature"])
    assert a[0].shape[0] == 0 and bins == []
    _, _, bins = check_maps(CASES["zero-length and inverted features"])
    assert bins == [(40, 50, 1)]


@pytest.mark.parametrize("seed", range(6))
def test_exon_maps_of_random_chromosomes(seed):
    rng = np.random.default_rng(500 + seed)
    features = G.random_features(rng, LENGTH - 20, 5, 14)
    for stranded in (False, True):
        _, _, bins = check_maps(features, stranded=stranded)
        assert len(bins) > 3


def test_the_coordinate_bound_is_genecounts():
    top = gc.COORD_MAX
    a, _, (gene, start, end) = xc.exon_maps(*_arrays([(top - 10, top - 1, "+", 0)]))
    assert a[0].tolist() == [top - 10, top - 1] and (gene.tolist(), start.tolist(), end.tolist()) == ([0], [top - 10], [top - 1])
    for stranded in (False, True):
        with pytest.raises(native.SpliserNativeError, match="int32 coordinate space") as err:
            xc.exon_maps(*_arrays([(5, 9, "-", 0), (top - 10, top, "-", 0)]), stranded=stranded)
        assert err.value.code == -6


# ---- the rule -----------------------------------------------------------------------------------------------------------------
def _rule(flag, pos, ops, bins, a, b, stranded, cap=64, shift=0):
    return native.exon_count_rule_host(flag, pos, ops, np.array([t[2] for t in bins], np.uint32), a, b, stranded, shift, cap)


@pytest.mark.parametrize("seed", range(4))
def test_rule_on_random_reads_and_features(seed):
    rng = np.random.default_rng(900 + seed)
    length = 3000
    features = G.random_features(rng, length - 700, 6, 24)
    records = G.random_records(rng, 700, length - 700)
    seen = set()
    for stranded in (0, 1, 2):
        a, b, bins = check_maps(features, length, bool(stranded)) if seed == 0 else (xc.exon_maps(*_arrays(features), stranded=bool(stranded))[:2] + (None,))
        labels = _labels(features, length, stranded)
        if bins is None:
            bins = X.bins_of([labels["+"], labels["-"]] if stranded else [labels])
        for flag, pos, cigar in records:
            o = G.ops(cigar)
            verdict, keys = X.read_of(flag, pos, o.tolist(), labels, stranded)
            want = [bins.index(k) for k in keys]
            assert _rule(flag, pos, o, bins, a, b, stranded) == (verdict, want, len(want)), (flag, pos, cigar)
            for cap in (0, 1):
                assert _rule(flag, pos, o, bins, a, b, stranded, cap) == (verdict, want[:cap], len(want))          # all hits, also beyond cap
            seen.add((verdict, min(len(want), 2)))
    assert seen == {(X.COUNTED, 1), (X.COUNTED, 2), (X.NO_FEATURE, 0), (X.AMBIGUOUS, 0), (X.NOT_COUNTED, 0)}          # (reads of several bins among them)


def test_rule_late_verdicts_deduplication_shift_and_many_hits():
    # gene 0: bins 0 (100..200), 1 (200..300; abuts); gene 1: bin 2 (400..500); shared 600..700; gene 0 again: 70 bins of 10 from 1000
    start = [100, 200, 300, 400, 500, 600, 700] + [1000 + 10 * k for k in range(71)]
    code = [1, 2, 0, 3, 0, G.MANY, 0] + [4 + k for k in range(70)] + [0]
    a = (np.array(start, np.int32), np.array(code, np.uint32))
    bin_gene = np.array([0, 0, 1] + [0] * 70, np.uint32)
    labels = X.MapLabels(start, code, bin_gene)
    for name, pos, cigar, want in (
            ("the first block in gene 0, the last in gene 1", 151, "10M239N10M", (X.AMBIGUOUS, [])),
            ("the last block in a shared stretch", 151, "10M439N10M", (X.AMBIGUOUS, [])),
            ("a deletion and an intron inside one bin: once", 111, "10M5D10M20N10M", (X.COUNTED, [0])),
            ("two blocks in abutting bins of one gene: each once", 191, "5M10N5M", (X.COUNTED, [0, 1])),
            ("one block over the two", 191, "20M", (X.COUNTED, [0, 1])),
            ("a block that ends exactly at a stretch's start", 91, "10M", (X.NO_FEATURE, [])),
            ("a block that begins exactly there", 101, "10M", (X.COUNTED, [0])),
            ("a block that ends at a bin's end and one on its last base", 291, "10M", (X.COUNTED, [1])),
            ("below the first entry and beyond the last", 1, "50M2000N50M", (X.NO_FEATURE, [])),
            ("one op over 70 bins", 991, "800M", (X.COUNTED, list(range(3, 73)))),
            ("over 70 bins and then gene 1 -- backwards: gene 1, then the 70", 451, "10M540N700M", (X.AMBIGUOUS, []))):
        o = G.ops(cigar)
        assert X.read_of(0, pos, o.tolist(), labels) == want, name
        assert native.exon_count_rule_host(0, pos, o, bin_gene, a, cap=100) == (want[0], want[1], len(want[1])), name
        assert native.exon_count_rule_host(0, pos, o, bin_gene, a, cap=2)[1:] == (want[1][:2], len(want[1])), name
        moved = (a[0] + 7000, a[1])
        assert native.exon_count_rule_host(0, pos, o, bin_gene, moved, shift=7000, cap=100) == (want[0], want[1], len(want[1])), name
    assert native.exon_count_rule_host(16, 101, G.ops("10M"), bin_gene, None, a, 1) == (X.COUNTED, [0], 1)          # the '-' read's map
    assert native.exon_count_rule_host(16, 101, G.ops("10M"), bin_gene, a, None, 1) == (X.NO_FEATURE, [], 0)
    assert native.exon_count_rule_host(4, 101, G.ops("10M"), bin_gene, a) == (X.NOT_COUNTED, [], 0)


def test_rule_refusals():
    o, genes = G.ops("20M"), np.array([0, 1, 1], np.uint32)
    for bad, match in (((np.array([30, 20], np.int32), np.array([1, 2], np.uint32)), "ascending"), ((np.array([20, 30], np.int32), np.array([1, 4], np.uint32)), "code"),
                       ((np.array([20, 30], np.int32), np.array([1, 0xFFFFFFFE], np.uint32)), "code")):
        for maps in ((bad, None), (None, bad)):
            with pytest.raises(native.SpliserNativeError, match=match) as err:
                native.exon_count_rule_host(0, 10, o, genes, *maps)
            assert err.value.code == -1
    with pytest.raises(native.SpliserNativeError, match="stranded"):
        native.exon_count_rule_host(0, 10, o, genes, None, None, 3)
    fine = (np.array([20, 25], np.int32), np.array([3, G.MANY], np.uint32))          # the greatest code there is, and "shared"
    assert native.exon_count_rule_host(0, 10, G.ops("12M"), genes, fine) == (0, [2], 1) and native.exon_count_rule_host(0, 10, o, genes, fine) == (X.AMBIGUOUS, [], 0)


def test_header_under_the_sanitizers(tmp_path):
    """The rule's header alone in a program of its own: ops, maps, genes and the hit list in heap blocks of exactly their size, so
    that an access beyond any aborts the child."""
    exe = str(tmp_path / "exoncount_asan")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "hostsim", "exoncount_rule_asan.cpp"), "-o", exe])
    rng = np.random.default_rng(77)
    length = 3000
    features = G.random_features(rng, length - 700, 6, 24) + [(2400 + 4 * k, 2402 + 4 * k, "+", 3) for k in range(70)]
    records = G.random_records(rng, 300, length - 700) + [(0, 2391, "300M"), (0, 1, "2500M"), (16, 2401, "1M3N" * 69 + "1M")]
    text_of = lambda v: " ".join(str(int(x)) for x in v)
    lines, want = [], []
    for stranded in (0, 1, 2):
        a, b, (bin_gene, bin_start, bin_end) = xc.exon_maps(*_arrays(features), stranded=bool(stranded))
        b = b or (np.zeros(0, np.int32), np.zeros(0, np.uint32))
        bins = list(zip(bin_start.tolist(), bin_end.tolist(), bin_gene.tolist()))
        labels = _labels(features, length, stranded)
        for k, (flag, pos, cigar) in enumerate(records):
            o, cap = G.ops(cigar), (0, 1, 3, 100)[k % 4]
            lines.append("%d %d 0 %d %d|%s|%s|%s|%s|%s|%s" % (flag, pos, stranded, cap, text_of(o), text_of(a[0]), text_of(a[1]), text_of(b[0]), text_of(b[1]), text_of(bin_gene)))
            verdict, keys = X.read_of(flag, pos, o.tolist(), labels, stranded)
            want.append([verdict, len(keys)] + [bins.index(key) for key in keys][:cap])
    assert max(w[1] for w in want) >= 70
    # a map of one entry and of none, a read at the top of the coordinate space with a shift on top: int64 throughout
    lines.append("0 2147483000 500000 0 4|%s|2147483500|1|||0" % text_of(G.ops("1000M")))
    want.append([0, 1, 0])
    lines.append("0 5 0 0 0|%s|||||" % text_of(G.ops("10M")))
    want.append([X.NO_FEATURE, 0])
    out = subprocess.run([exe], input="\n".join(lines) + "\n", stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0"))
    assert out.returncode == 0, out.stderr
    assert [[int(v) for v in line.split()] for line in out.stdout.splitlines()] == want


# ---- ids, ranks and the writers ----------------------------------------------------------------------------------------------------
GTF = "\n".join([
    'c2\tsrc\texon\t101\t200\t.\t+\t.\tgene_id "gB"; transcript_id "t1";',
    'c2\tsrc\texon\t151\t300\t.\t+\t.\tgene_id "gB"; transcript_id "t2";',
    'c1\tsrc\texon\t11\t20\t.\t-\t.\tgene_id "gA";',
    'c1\tsrc\texon\t21\t30\t.\t-\t.\tgene_id "gA";',
    'c1\tsrc\texon\t501\t600\t.\t+\t.\tgene_id "gB";',
    'c1\tsrc\texon\t551\t650\t.\t+\t.\tgene_id "gC";',
    'c2\tsrc\texon\t1\t50\t.\t.\t.\tgene_id "gA";',
    'c3\tsrc\texon\t5\t4\t.\t+\t.\tgene_id "gD";',
    "",
])


def test_ids_ranks_and_both_files_byte_for_byte(tmp_path):
    path = str(tmp_path / "a.gtf")
    open(path, "w").write(GTF)
    ids, by_chrom = G.features_of_text(GTF)
    chroms = ["c2", "c1", "c3"]                       # the annotation's order of first appearance
    for stranded in (False, True):
        bins = xc.Bins(gc.read_features(path), stranded)
        want_bins = {}
        for c in chroms:
            labels = _labels(by_chrom[c], 700, stranded)
            want_bins[c] = X.bins_of([labels["+"], labels["-"]] if stranded else [labels])
            assert list(zip(*[v.tolist() for v in (xc.exon_maps(*_arrays(by_chrom[c]), stranded=stranded)[2][k] for k in (1, 2, 0))])) == want_bins[c]
        rows = X.rows_of(ids, chroms, want_bins)
        assert bins.chroms == chroms and bins.n == len(rows) and [bins.row_id(k) for k in range(bins.n)] == [r[0] for r in rows]
        if not stranded:
            # gA: its bin on c2 ranks before its two on c1; gB: three on c2, then one on c1 (the rest of that exon is shared with gC); gD has none
            assert [r[:5] for r in rows] == [("gA:001", "gA", "c2", 0, 50), ("gA:002", "gA", "c1", 10, 20), ("gA:003", "gA", "c1", 20, 30), ("gB:001", "gB", "c2", 100, 150),
                                             ("gB:002", "gB", "c2", 150, 200), ("gB:003", "gB", "c2", 200, 300), ("gB:004", "gB", "c1", 500, 550), ("gC:001", "gC", "c1", 600, 650)]
        per_bin = {"c1": np.arange(len(want_bins["c1"]), dtype=np.int64) * 7 + 70000000000, "c2": np.arange(len(want_bins["c2"]), dtype=np.int64) + 1}
        verdicts = [99, 5, 6, 7]
        for only in (None, "c1", "c2", "c3", "c9"):
            use = bins.rows_on(only)
            want_rows = X.rows_of(ids, chroms, want_bins, only)
            b_path, c_path = str(tmp_path / "x.exonbins.tsv"), str(tmp_path / "x.exoncounts.tsv")
            assert xc.write_bins(b_path, bins, use) == len(want_rows)
            assert xc.write_counts(c_path, bins, use, xc.row_counts(bins, per_bin, use), verdicts) == len(want_rows)
            assert open(b_path).read() == X.bins_text(want_rows)
            assert open(c_path).read() == X.counts_text(want_rows, {c: v.tolist() for c, v in per_bin.items()}, verdicts)
        assert X.bins_text(X.rows_of(ids, chroms, want_bins, "c1")).splitlines()[1] == "gA:002\tgA\tc1\t11\t20"          # 1-based inclusive: the exon's own numbers
        assert open(c_path).read() == "__no_feature\t5\n__ambiguous\t6\n__not_counted\t7\n"
    assert (xc.BINS_SUFFIX, xc.COUNTS_SUFFIX, xc.SPECIALS) == (".exonbins.tsv", ".exoncounts.tsv", X.SPECIALS)


# ---- the command line ---------------------------------------------------------------------------------------------------------
def test_parser_results():
    p = cli.build_parser()
    a = vars(p.parse_args(["exoncounts", "-B", "x.bam", "-A", "g.gtf", "-o", "out"]))
    assert (a["inBAM"], a["annotationFile"], a["outputPath"], a["aType"], a["idAttr"], a["qChrom"], a["isStranded"], a["strandedType"]) == \
        ("x.bam", "g.gtf", "out", "exon", "gene_id", "All", False, None)
    assert (a["anyOrder"], a["gpuDecode"], a["minMapQ"], a["requireFlags"], a["excludeFlags"], a["gpus"], a["devices"], a["threads"]) == (False, None, 0, 0, 0, 1, None, 0)
    a = vars(p.parse_args(["exoncounts", "-B", "x.sam.gz", "-A", "g.gff", "-o", "out", "-t", "CDS", "--idAttr", "Parent", "-c", "chr2", "--isStranded", "-s", "rf", "--anyOrder",
                           "--hostDecode", "--minMapQ", "255", "--requireFlags", "0x2", "--excludeFlags", "0x400", "--gpus", "2", "--threads", "4"]))
    assert (a["aType"], a["idAttr"], a["qChrom"], a["isStranded"], a["strandedType"], a["anyOrder"], a["gpuDecode"]) == ("CDS", "Parent", "chr2", True, "rf", True, False)
    assert (a["minMapQ"], a["requireFlags"], a["excludeFlags"], a["gpus"], a["threads"]) == (255, 2, 0x400, 2, 4)
    assert vars(p.parse_args(["exoncounts", "-B", "x", "-A", "g", "-o", "o", "--gpuDecode", "--devices", "0,1"]))["gpuDecode"] is True
    assert "exonCounts" not in vars(p.parse_args(["process", "-B", "x", "-o", "o"]))          # (process has no such flag)
    assert set(vars(p.parse_args(["exoncounts", "-B", "x", "-A", "g", "-o", "o"]))) == set(vars(p.parse_args(["genecounts", "-B", "x", "-A", "g", "-o", "o"])))


@pytest.mark.parametrize("argv, match", [
    (["exoncounts", "-B", "x.bam", "-o", "o"], "exoncounts: --annotationFile/-A is required"),
    (["exoncounts", "-B", "x.bam", "-A", "g.gtf", "-o", "o", "-s", "auto"], "exoncounts: -s auto is not taken here: the `strandedness` command"),
    (["exoncounts", "-B", "x.bam", "-A", "g.gtf", "-o", "o", "--isStranded", "-s", "auto"], "-s auto is not taken here"),
    (["exoncounts", "-B", "x.bam", "-A", "g.gtf", "-o", "o", "--isStranded"], "--isStranded requires parameter --strandedType/-s as fr or rf"),
    (["exoncounts", "-B", "x.bam", "-A", "g.gtf", "-o", "o", "--isStranded", "-s", "ff"], "exoncounts: --strandedType/-s must be fr or rf"),
    (["exoncounts", "-B", "x.bam", "-A", "g.gtf", "-o", "o", "--minMapQ", "256"], "--minMapQ must be in 0..255"),
    (["exoncounts", "-B", "x.bam", "-A", "g.gtf", "-o", "o", "--excludeFlags", "65536"], "must be in 0..65535"),
    (["exoncounts", "-B", "x.bam", "-A", "g.gtf", "-o", "o", "--requireFlags", "4", "--excludeFlags", "0x4"], "share a bit"),
    (["exoncounts", "-A", "g.gtf", "-o", "o"], "-B"),
    (["exoncounts", "-B", "x.bam", "-A", "g.gtf"], "-o"),
    (["process", "-B", "x.bam", "-o", "o", "--exonCounts"], "unrecognized"),
])
def test_parser_errors(argv, match, capsys):
    with pytest.raises(SystemExit) as err:
        cli.main(argv)
    assert err.value.code == 2
    assert match in capsys.readouterr().err


def test_the_function_refuses_what_the_parser_refuses():
    with pytest.raises(ValueError, match="-A"):
        xc.exoncounts("x.bam", None, "o")
    with pytest.raises(ValueError, match="-s fr or -s rf"):
        xc.exoncounts("x.bam", "g.gtf", "o", isStranded=True, strandedType="auto")
