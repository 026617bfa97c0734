"""``--strandFromXS`` above the decode, without a GPU: the site table from arrays (``fast_sites.build_from_arrays``) against the
line-by-line ``sites.SiteTable`` on junction tables that have ``+``, ``-`` and ``?`` rows at shared positions -- what mode 3 of
``spl_junctions`` produces and modes 0 / 1 / 2 never did --, the yardstick of the GPU tests on a case worked out by hand, and
the command line's refusals."""
import io

import numpy as np
import pytest

import xscases as X
from spliser_amd import cli, fast_sites, junctions as jn, native, process as proc, samio, sites


@pytest.fixture(scope="module", autouse=True)
def _built():
    native.build()


def _three_strand_tables(rng, n_chrom=3, n_pairs=120):
    """[(chrom, table)]: junctions over a small set of ends, each pair with one, two or all three strands, counts and anchors
    random, sorted as spl_junctions sorts."""
    out = []
    for k in range(n_chrom):
        ends = np.sort(rng.choice(np.arange(200, 60000), 50, replace=False))
        rows = set()
        for _ in range(n_pairs):
            a, b = sorted(int(x) for x in rng.choice(ends, 2, replace=False))
            for s in rng.choice([43, 45, 63], int(rng.integers(1, 4)), replace=False):
                rows.add((a, b, int(s)))
        rows = sorted(rows)
        out.append(("c%d" % k, X.table_of([(a, b, s, int(rng.integers(1, 400)), int(rng.integers(1, 50)), int(rng.integers(1, 50))) for a, b, s in rows])))
    return out


@pytest.mark.parametrize("seed", range(4))
def test_site_table_from_arrays_with_all_three_strands_at_one_position(seed, tmp_path):
    rng = np.random.default_rng(100 + seed)
    rows = _three_strand_tables(rng)
    for _, t in rows:      # (the case is the case: some junction has all three strands, some position is shared by different strands)
        key = list(zip(t["left"].tolist(), t["right"].tolist()))
        assert max(key.count(k) for k in set(key)) == 3
    bed = str(tmp_path / "j.bed")
    jn.write_bed_file(bed, [c for c, _ in rows], dict(rows), 8, 70, 500000)
    slow = sites.SiteTable(sites.GeneBins(), is_stranded=False)
    slow.add_bed(bed)
    slow.find_competitors()
    fast = fast_sites.build_from_arrays(sites.GeneBins(), False, [(c, t["left"], t["right"], t["strand"], t["count"]) for c, t in rows])
    if fast is None:       # (declined: `process` then reads the lines, as for coinciding ends -- nothing more to hold it to)
        text = io.StringIO()
        first = 1
        for c, t in rows:
            first += jn.write_junction_bed(text, c, t, first)
        assert text.getvalue() == "".join(open(bed).readlines()[1:])
        return
    fast.find_competitors()
    assert list(fast.chrom_index) == list(slow.chrom_index)
    assert (fast.assessed, fast.created, fast.assigned, fast.n_sites()) == (slow.assessed, slow.created, slow.assigned, slow.n_sites())
    for chrom in slow.chrom_index:
        a, b = slow.chrom_arrays(chrom), fast.chrom_arrays(chrom)
        assert a.n == b.n
        for name in ("pos", "strand", "alpha", "part_off", "part_pos", "part_site", "edge_cnt", "comp_off", "comp_pos"):
            x, y = getattr(a, name), getattr(b, name)
            assert x.dtype == y.dtype and np.array_equal(x, y), (chrom, name)
        assert a.genes == b.genes and a.strand_text == b.strand_text


def test_the_yardstick_on_a_case_worked_out_by_hand():
    """One junction (left 119, right 219) carried by +-tagged, --tagged, untagged and XS:i reads: three rows, each with its own
    count and anchor maxima; and merge_tables adds pieces of it by (left, right, strand)."""
    rs = samio.ReadSet.from_records([(0, 100, "20M100N30M"), (16, 105, "15M100N9M"), (0, 110, "10M100N40M"), (0, 112, "8M100N8M"),
                                     (0, 90, "30M100N12M"), (0, 100, "50M")])
    xs = np.array([43, 43, 45, 0, 0, 0], np.uint8)      # (the XS:i read's byte is 0, like the untagged one's)
    assert X.yardstick(rs, xs) == [(119, 219, 43, 2, 20, 30), (119, 219, 45, 1, 10, 40), (119, 219, 63, 2, 30, 12)]
    assert X.yardstick(rs, xs, (9, 70, 500000)) == [(119, 219, 43, 2, 20, 30), (119, 219, 45, 1, 10, 40), (119, 219, 63, 1, 30, 12)]
    whole = X.table_of(X.yardstick(rs, xs))
    halves = [X.table_of(X.yardstick(X.subset(rs, m), xs[m])) for m in (np.arange(6) < 3, np.arange(6) >= 3)]
    assert X.rows_of(jn.merge_tables(halves)) == X.rows_of(whole)


@pytest.mark.parametrize("argv", [
    ["process", "-B", "x.bam", "-b", "j.bed", "-o", "out", "--strandFromXS"],
    ["process", "-B", "x.bam", "-o", "out", "--strandFromXS", "--isStranded", "-s", "fr"],
    ["junctions", "-B", "x.bam", "-o", "out.bed", "--strandFromXS", "--isStranded", "-s", "rf"],
])
def test_the_command_line_refuses_what_cannot_be_meant(argv, capsys):
    with pytest.raises(SystemExit) as err:
        cli.main(argv)
    assert err.value.code == 2
    assert "--strandFromXS" in capsys.readouterr().err


def test_the_functions_refuse_it_too(tmp_path):
    with pytest.raises(ValueError, match="strandFromXS"):
        proc.process("x.bam", inBed="j.bed", outputPath=str(tmp_path / "o"), strandFromXS=True)
    with pytest.raises(ValueError, match="alternatives"):
        proc.process("x.bam", outputPath=str(tmp_path / "o"), strandFromXS=True, isStranded=True, strandedType="fr")
    with pytest.raises(ValueError, match="alternatives"):
        jn.junctions("x.bam", str(tmp_path / "o.bed"), strandFromXS=True, isStranded=True, strandedType="fr")
    ns = cli.build_parser().parse_args(["junctions", "-B", "x.bam", "-o", "o.bed", "--strandFromXS"])
    assert ns.strandFromXS is True and cli.build_parser().parse_args(["process", "-B", "x", "-o", "o"]).strandFromXS is False
