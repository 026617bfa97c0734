"""`process` without -b, the parts that need no GPU: the per-read junction walk the two junction kernels share
(spl_junction_walk.h, compiled for the host: spl_junction_walk_host) against oracle.junction_table on every case of
junctioncases.py and on random CIGARs; the site table built straight from junction arrays against the one today's builders
read from the BED text of the same junctions; the command line."""
import io
import os

import numpy as np
import pytest

import helpers
import junctioncases as J
import randcase
from oracle import oracle
from spliser_amd import cli, fast_sites, junctions as jn, native, process as proc, samio

ARRAYS = ("pos", "strand", "alpha", "gene_idx", "part_off", "part_pos", "part_site", "edge_cnt", "comp_off", "comp_pos")


@pytest.fixture(scope="module", autouse=True)
def built():
    native.build()


# ---- the walk ---------------------------------------------------------------------------------------------------------------------

def _walk_table(reads, stranded, a, m, mx, walked=None):
    """oracle.junction_table's aggregation over the shared walk's per-read tuples."""
    table = {}
    pos, flag, off = reads.pos.tolist(), reads.flag.tolist(), reads.cig_off.tolist()
    for i in range(reads.n):
        if flag[i] & 4 or pos[i] < 0:
            continue
        if walked is not None and (i, a, m, mx) in walked:
            rows = walked[(i, a, m, mx)]
        else:
            rows, bad = native.junction_walk_host(reads.cigar[off[i]:off[i + 1]], pos[i], a, m, mx)
            assert not bad
            if walked is not None:
                walked[(i, a, m, mx)] = rows
        strand = (ord("-") if J.read_minus(flag[i], stranded) else ord("+")) if stranded else ord("?")
        for l, r, al, ar, ok in rows:
            if ok:
                c, x, y = table.get((l, r, strand), (0, 0, 0))
                table[(l, r, strand)] = (c + 1, max(x, al), max(y, ar))
    return [k + table[k] for k in sorted(table)]


@pytest.mark.parametrize("name", J.CASE_NAMES)
def test_shared_walk_gives_the_restated_table(name):
    case = J.case(name)
    walked = {}
    for a, m, mx in case.filters:
        for stranded in (0, 1, 2):
            assert _walk_table(case.reads, stranded, a, m, mx, walked) == case.want(stranded, a, m, mx), (name, stranded, (a, m, mx))


def _random_reads(seed, n=400):
    """CIGARs of every op code, N ops anywhere (first, last, adjacent, of length 0), a few unmapped and unplaced records."""
    rng = np.random.default_rng(seed)
    recs = []
    for _ in range(n):
        k = int(rng.integers(0, 9))
        ops = [(int(rng.integers(0, 40)), int(rng.choice([J.M, J.M, J.N, J.N, J.D, J.I, J.S, J.EQ, J.X, J.H, J.P]))) for _ in range(k)]
        flag = int(rng.choice([0, 16, 99, 147, 83, 163, 4, 20]))
        recs.append((flag, int(rng.integers(0, 3000)), ops))
    return J.reads_from(recs)


@pytest.mark.parametrize("seed", range(6))
def test_shared_walk_on_random_cigars(seed):
    sets = [_random_reads(seed), randcase.make_case(seed + 40, bool(seed & 1))[1]]
    for reads in sets:
        for a, m, mx in ((0, 0, 0), (1, 1, 0), (5, 10, 30), (8, 70, 500000), (0, 0, 20)):
            for stranded in (0, 1, 2):
                want = oracle.junction_table(reads.pos, reads.flag, reads.cig_off, reads.cigar, stranded, a, m, mx)
                assert _walk_table(reads, stranded, a, m, mx) == want, (seed, stranded, (a, m, mx))


def test_shared_walk_stops_at_the_end_of_the_coordinate_space():
    bad = J.beyond_coord_max()
    off = bad.cig_off.tolist()
    rows, err = native.junction_walk_host(bad.cigar[off[1]:off[2]], int(bad.pos[1]), 0, 0, 0)
    assert err and [r[:2] for r in rows] == [(J.COORD_MAX - 101, J.COORD_MAX - 51)]
    top = J.coordinates_case().reads
    off = top.cig_off.tolist()
    for i in range(top.n):
        assert not native.junction_walk_host(top.cigar[off[i]:off[i + 1]], int(top.pos[i]), 0, 0, 0)[1]


def test_fewest_ops_of_a_supporting_read_is_exact():
    """What lets the fused kernel pass over a read on its op count alone: with min_anchor > 0 no read of fewer than three ops
    supports a junction; with min_anchor = 0 one op is enough."""
    for ops in ([(50, J.N)], [(50, J.N), (20, J.M)], [(20, J.M), (50, J.N)], [(50, J.N), (60, J.N)], [(3, J.D), (50, J.N)]):
        rs = J.reads_from([(0, 100, ops)])
        assert all(not r[4] for r in native.junction_walk_host(rs.cigar, 100, 1, 0, 0)[0])
        assert all(r[4] for r in native.junction_walk_host(rs.cigar, 100, 0, 0, 0)[0])
    rs = J.reads_from([(0, 100, [(1, J.M), (50, J.N), (1, J.D)])])
    assert [r[4] for r in native.junction_walk_host(rs.cigar, 100, 1, 0, 0)[0]] == [True]


# ---- the site table from arrays --------------------------------------------------------------------------------------------------

def _rows_of_bed(path):
    """[(chrom, junction table)] of a BED12 file the `junctions` command wrote (chromosomes in the file's order)."""
    per, order = {}, []
    with open(path) as fh:
        for line in fh:
            v = line.rstrip("\n").split("\t")
            if len(v) != 12:
                continue
            a_l, a_r = (int(x) for x in v[10].split(","))
            if v[0] not in per:
                per[v[0]] = []
                order.append(v[0])
            per[v[0]].append((int(v[1]) + a_l, int(v[2]) - a_r, ord(v[5]), int(v[4]), a_l, a_r))
    return [(c, _table(per[c])) for c in order]


def _table(rows):
    cols = list(zip(*rows)) if rows else [()] * 6
    dt = (np.int32, np.int32, np.uint8, np.uint32, np.uint32, np.uint32)
    return {k: np.array(v, d) for k, v, d in zip(("left", "right", "strand", "count", "anchor_left", "anchor_right"), cols, dt)}


def _both_ways(rows, tmp_path, stranded=None, gff=None, gene="All", chrom="All", max_intron=0):
    """The site table (a) from the junction arrays, as `process` without -b builds it, and (b) from the BED file of the same
    junctions, as `process -b` builds it today."""
    bed = str(tmp_path / "j.bed")
    with open(bed, "w") as fh:
        fh.write(jn.track_line(1, 1, 0))
        first = 1
        for c, t in rows:
            first += jn.write_junction_bed(fh, c, t, first)
    quiet = lambda m: None
    a = proc._site_table(None, gene, chrom, max_intron, gff, "gene", bool(stranded), stranded, quiet, rows_of_bam=lambda: rows)
    b = proc._site_table(bed, gene, chrom, max_intron, gff, "gene", bool(stranded), stranded, quiet)
    return a, b


def _assert_same_tables(a, b, tag):
    assert list(a.chrom_index) == list(b.chrom_index), tag
    assert (a.assessed, a.created, a.assigned, a.n_sites()) == (b.assessed, b.created, b.assigned, b.n_sites()), tag
    for chrom in a.chrom_index:
        x, y = a.chrom_arrays(chrom), b.chrom_arrays(chrom)
        assert x.n == y.n, (tag, chrom)
        for k in ARRAYS:
            assert np.array_equal(np.asarray(getattr(x, k)), np.asarray(getattr(y, k))), (tag, chrom, k)
        for k in ("gene_names", "strand_text"):      # (lists, or None where the builder keeps the genes with the rows)
            u, v = getattr(x, k, None), getattr(y, k, None)
            assert (None if u is None else list(u)) == (None if v is None else list(v)), (tag, chrom, k)


@pytest.mark.parametrize("case,stranded", [("junctions_u", None), ("junctions_fr", "fr")])
def test_site_table_from_arrays_equals_the_one_from_text_on_the_goldens(case, stranded, tmp_path):
    """(These two cases have no annotation of their own: the annotated comparison is the next test.)"""
    rows = _rows_of_bed(os.path.join(helpers.GOLDEN, case, "junctions.bed"))
    assert rows
    for s in (None, stranded) if stranded else (None,):
        a, b = _both_ways(rows, tmp_path, stranded=s)
        assert isinstance(a, fast_sites.FastSiteTable)
        _assert_same_tables(a, b, (case, s))
        a, b = _both_ways(rows, tmp_path, stranded=s, chrom=rows[-1][0])
        _assert_same_tables(a, b, (case, s, "-c"))


def _oracle_rows(names, sets, scode, knobs=(1, 1, 0)):
    rows = []
    for c, rs in zip(names, sets):
        if rs is not None and rs.n:
            t = oracle.junction_table(rs.pos, rs.flag, rs.cig_off, rs.cigar, scode, *knobs)
            if t:
                rows.append((c, _table(t)))
    return rows


@pytest.mark.parametrize("stranded", [None, "fr"])
@pytest.mark.parametrize("source", ["single_gene", "synth"])
def test_site_table_from_arrays_with_an_annotation(source, stranded, tmp_path):
    """The array builder WITH an annotation, on the fast path (no gene query): gene_idx / gene_names / the assigned count come from
    the bins and must be what fast_sites.build gives for the text of the same junctions.  The annotation is the single_gene golden's
    (one chromosome) and a synthetic five-chromosome genome's, whose junctions lie in its genes on both strands."""
    scode = native.STRANDED_CODE[stranded]
    if source == "single_gene":
        d = os.path.join(helpers.GOLDEN, "single_gene")
        gff = os.path.join(d, "genes.gff")
        names, sets = samio.read_sam(os.path.join(d, "reads.sam"))
        rows = _oracle_rows(names, [sets.get(c) for c in names], scode)
    else:
        from spliser_amd import synth
        wl = synth.Workload("arabidopsis", scale=0.001, seed=77, workers=1)
        for r in wl.reads:
            r.flag[:] = np.random.default_rng(5).choice(np.array([99, 147, 83, 163], np.uint16), size=r.n)
        gff = str(tmp_path / "genes.gff")
        synth.write_gff(gff, wl.genome)
        rows = _oracle_rows(wl.genome.chrom_names, wl.reads, scode)
        assert len(rows) == 5
    assert os.path.exists(gff) and rows
    for chrom in ("All", rows[-1][0]):
        a, b = _both_ways(rows, tmp_path, stranded=stranded, gff=gff, chrom=chrom)
        assert isinstance(a, fast_sites.FastSiteTable) and isinstance(b, fast_sites.FastSiteTable)
        assert a.assigned > 0 and any(int((a.chrom_arrays(c).gene_idx >= 0).sum()) > 0 for c, _ in rows)
        _assert_same_tables(a, b, (source, stranded, chrom))
    # ... and without the annotation no site has a gene: the annotated table is another one
    plain, _ = _both_ways(rows, tmp_path, stranded=stranded)
    assert plain.assigned == 0


def _single_gene_rows():
    """The single_gene golden's reads -> junction rows by the oracle (stranded fr), with its annotation and gene."""
    d = os.path.join(helpers.GOLDEN, "single_gene")
    names, sets = samio.read_sam(os.path.join(d, "reads.sam"))
    rows = []
    for c in names:
        rs = sets.get(c)
        if rs is not None and rs.n:
            t = oracle.junction_table(rs.pos, rs.flag, rs.cig_off, rs.cigar, 0, 1, 1, 0)
            if t:
                rows.append((c, _table(t)))
    gene = None
    with open(os.path.join(d, "genes.gff")) as fh:
        for line in fh:
            v = line.split("\t")
            if len(v) >= 9 and v[2] == "gene" and v[0] == rows[0][0]:
                gene = v[8].split(";")[0].split("=")[-1].strip()
                break
    return d, rows, gene


def test_site_table_for_a_gene_query_takes_the_line_by_line_builder(tmp_path):
    d, rows, gene = _single_gene_rows()
    assert rows and gene
    a, b = _both_ways(rows, tmp_path, gff=os.path.join(d, "genes.gff"), gene=gene, chrom=rows[0][0], max_intron=2000)
    assert not isinstance(a, fast_sites.FastSiteTable)
    assert a.n_sites() > 0
    _assert_same_tables(a, b, "gene query")


@pytest.mark.parametrize("seed", range(4))
@pytest.mark.parametrize("stranded", [None, "fr"])
def test_site_table_from_random_junction_tables(seed, stranded, tmp_path):
    scode = native.STRANDED_CODE[stranded]
    rows = []
    for k in range(3):
        reads = _random_reads(100 + 10 * seed + k, n=300)
        t = oracle.junction_table(reads.pos, reads.flag, reads.cig_off, reads.cigar, scode, 0, 1, 0)
        t = [r for r in t if r[0] >= 0 and r[0] != r[1]]
        rows.append(("c%d" % k, _table(t)))
    a, b = _both_ways(rows, tmp_path, stranded=stranded)
    assert isinstance(a, fast_sites.FastSiteTable) and a.n_sites() > 0
    _assert_same_tables(a, b, (seed, stranded))


@pytest.mark.parametrize("stranded", [None, "fr"])
def test_site_table_with_a_left_of_minus_one_and_with_coinciding_ends(stranded, tmp_path):
    scode = native.STRANDED_CODE[stranded]
    minus_one = J.reads_from([(0, 0, [(30, J.N), (20, J.M)]), (0, 100, [(20, J.M), (50, J.N), (20, J.M)]), (16, 100, [(20, J.M), (80, J.N), (9, J.M)])])
    same_ends = J.reads_from([(0, 100, [(20, J.M), (0, J.N), (20, J.M)]), (0, 100, [(20, J.M), (50, J.N), (20, J.M)]), (16, 119, [(1, J.M), (50, J.N), (20, J.M)])])
    for reads, what in ((minus_one, "left -1"), (same_ends, "ends coincide")):
        t = oracle.junction_table(reads.pos, reads.flag, reads.cig_off, reads.cigar, scode, 0, 0, 0)
        assert any(r[0] == -1 for r in t) if what == "left -1" else any(r[0] == r[1] for r in t)
        rows = [("c0", _table(t))]
        a, b = _both_ways(rows, tmp_path, stranded=stranded)
        assert not isinstance(a, fast_sites.FastSiteTable)
        _assert_same_tables(a, b, (what, stranded))


def test_merge_of_partial_tables_is_the_table_of_the_whole():
    reads = _random_reads(77, n=600)
    off = reads.cig_off.tolist()
    cuts = [0, 150, 151, 420, 600]
    parts = []
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        t = oracle.junction_table(reads.pos[lo:hi], reads.flag[lo:hi], reads.cig_off[lo:hi + 1] - off[lo], reads.cigar[off[lo]:off[hi]], 1, 0, 0, 0)
        parts.append(_table(t))
    parts.append(_table([]))
    whole = oracle.junction_table(reads.pos, reads.flag, reads.cig_off, reads.cigar, 1, 0, 0, 0)
    extra = (-1, 29, ord("+"), 2, 0, 20)      # a left of -1 sorts first (signed), whichever piece brings it
    parts.append(_table([extra]))
    assert J.rows(jn.merge_tables(parts)) == sorted(whole + [extra])


# ---- the command line ------------------------------------------------------------------------------------------------------------

def test_parser_takes_process_without_a_bed_file():
    ns = cli.build_parser().parse_args(["process", "-B", "x", "-o", "y"])
    assert ns.inBed is None and (ns.minAnchor, ns.minIntron, ns.maxIntron, ns.keepJunctions) == (None, None, None, False)
    ns = cli.build_parser().parse_args(["process", "-B", "x", "-o", "y", "--minAnchor", "3", "--minIntron", "0", "--maxIntron", "9", "--keepJunctions"])
    assert (ns.minAnchor, ns.minIntron, ns.maxIntron, ns.keepJunctions) == (3, 0, 9, True)
    assert proc.JUNCTION_DEFAULTS == J.DEFAULTS


@pytest.mark.parametrize("argv", [
    ["process", "-B", "x", "-o", "y", "-b", "f", "--minAnchor", "3"],
    ["process", "-B", "x", "-o", "y", "-b", "f", "--minIntron", "3"],
    ["process", "-B", "x", "-o", "y", "-b", "f", "--maxIntron", "3"],
    ["process", "-B", "x", "-o", "y", "-b", "f", "--keepJunctions"],
    ["process", "-B", "x", "-o", "y", "--checkJunctions"],
    ["process", "-B", "x", "-o", "y", "--minAnchor", "-1"],
])
def test_parser_refuses_what_has_no_meaning(argv, capsys):
    with pytest.raises(SystemExit) as err:
        cli.main(argv)
    assert err.value.code == 2
    capsys.readouterr()


def test_process_function_refuses_the_same():
    with pytest.raises(ValueError):
        proc.process("x", "f", "y", minAnchor=3)
    with pytest.raises(ValueError):
        proc.process("x", None, "y", checkJunctions=True)
