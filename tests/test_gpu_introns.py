"""``spl_intron_depth`` on the device: the kernel over a caller's boundaries (``spl_intron_depth_runs``) against the yardstick's
base-by-base expansion (introncases.py) at the sizes where it takes another path -- the cases of the team's body, introns on each
side of the long-intron threshold, one intron of 10^5 boundaries among 10^4 small ones, more introns than a launch has workgroups --,
``spl_intron_depth`` over an uploaded read set against the yardstick's per-base depth, the refusals, and the ``intronretention``
command byte for byte after every decode.  The reference has no counterpart: it measures no intron."""
import os
import re

import numpy as np
import pytest

import covcases as C
import genecases as G
import introncases as I
import ordercases as O
from spliser_amd import cli, native, samio

pytestmark = pytest.mark.gpu
TRIMS = (0, 30, 49)


def _constant(name):
    """A geometry constant of csrc/spl_intron.h, read from the header."""
    text = open(os.path.join(os.path.dirname(os.path.abspath(native.__file__)), "csrc", "spl_intron.h")).read()
    return int(re.search(r"#define %s (\d+)" % name, text).group(1))


LONG, GRID_MAX = _constant("SPL_INTRON_LONG_BASES"), _constant("SPL_INTRON_GRID_MAX")


@pytest.fixture(scope="module")
def ctx():
    with native.Context(0) as c:
        yield c


def _tables(introns):
    off = np.zeros(len(introns) + 1, np.int64)
    off[1:] = np.cumsum([len(p) for p in introns])
    return off, np.array([p[0] for pieces in introns for p in pieces], np.int32), np.array([p[1] for pieces in introns for p in pieces], np.int32)


def _runs(ctx, pos, depth, introns, length, trim):
    got = native.intron_depth_runs(ctx, pos, depth, length, *_tables(introns), trim_percent=trim)
    assert got.dtype == np.int64 and got.shape == (len(introns), 4)
    return [tuple(r) for r in got.tolist()]


def _both(ctx, pos, depth, introns, length, trims=TRIMS, per_base=None):
    per_base = I.depth_per_base(pos, depth, length) if per_base is None else per_base
    for trim in trims:
        assert _runs(ctx, pos, depth, introns, length, trim) == [I.stats_of(per_base, pieces, trim) for pieces in introns], "trim %d" % trim


# ---- 1: the kernel over given boundaries --------------------------------------------------------------------------------------
def test_no_intron_and_no_boundary(ctx):
    assert native.intron_depth_runs(ctx, [3, 9], [1, 0], 100, [0], [], []).shape == (0, 4)
    assert native.intron_depth_runs(ctx, [], [], 100, [0], [], []).shape == (0, 4)
    assert _runs(ctx, [], [], [[(0, 10)], [], [(5, 6), (8, 100)]], 100, 30) == [(10, 0, 4, 0), (0, 0, 0, 0), (93, 0, 39, 0)]


CASES = I.body_cases()


@pytest.mark.parametrize("k", range(len(CASES)), ids=[c[0] for c in CASES])
def test_body_cases(ctx, k):
    _, pos, depth, introns, length = CASES[k]
    _both(ctx, pos, depth, introns, length)


def test_introns_on_each_side_of_the_long_intron_threshold_and_at_it(ctx):
    """LONG - 1 bases: a wave; LONG and LONG + 1: a team; as one piece and as three; with few boundaries inside and with thousands."""
    rng = np.random.default_rng(LONG)
    length = 2 * LONG + 500
    for n_bound, max_depth in ((40, 9), (6000, 300), (6000, 2 ** 32 - 1)):
        pos, depth = I.random_bounds(rng, length, n_bound, max_depth)
        introns = []
        for bases in (LONG - 1, LONG, LONG + 1):
            introns.append([(100, 100 + bases)])
            introns.append([(7, 1007), (1500, 1500 + bases - 1999), (length - 999, length)])
        assert [sum(e - s for s, e in p) for p in introns] == [LONG - 1] * 2 + [LONG] * 2 + [LONG + 1] * 2
        _both(ctx, pos, depth, introns, length)


def test_one_intron_of_100000_boundaries_among_10000_of_one(ctx):
    """The long one has a team, the others a wave each -- more of them than a launch has workgroups --; no timing is asserted."""
    rng = np.random.default_rng(100000)
    n_long, n_small = 100000, 10000
    assert n_small > GRID_MAX and 2 * n_long >= LONG
    small_at = 2 * n_long + 50
    pos = [2 * k for k in range(n_long)] + [small_at + 10 * k + 3 for k in range(n_small)]
    depth = [int(v) for v in rng.integers(0, 2000, n_long)] + [int(v) for v in rng.integers(1, 90, n_small)]
    for k in range(0, n_long, 977):
        depth[k] = 2 ** 32 - 1 - k
    length = small_at + 10 * n_small
    small = [[(small_at + 10 * k, small_at + 10 * k + 8)] for k in range(n_small)]
    introns = small[:5000] + [[(0, 2 * n_long)]] + small[5000:]
    per_base = I.depth_per_base(pos, depth, length)
    want = {trim: [I.stats_of(per_base, pieces, trim) for pieces in introns] for trim in TRIMS}
    assert want[0][5000][:3] == (2 * n_long, 2 * n_long - 2 * depth[:n_long].count(0), 2 * n_long) and want[30][0][0] == 8
    for trim in TRIMS:
        assert _runs(ctx, pos, depth, introns, length, trim) == want[trim]


def test_more_long_introns_than_a_launch_has_workgroups(ctx):
    """Teams grid-stride too.  Four different introns over the same bases, each many times: overlapping pieces of different introns."""
    rng = np.random.default_rng(7)
    length = LONG + 4000
    pos, depth = I.random_bounds(rng, length, 900, 50)
    kinds = [[(k, k + LONG)] for k in (0, 1, 1999)] + [[(5, 1005), (1100, 1100 + LONG)]]
    introns = [kinds[k % 4] for k in range(GRID_MAX + 37)]
    per_base = I.depth_per_base(pos, depth, length)
    for trim in (30,):
        want = [I.stats_of(per_base, pieces, trim) for pieces in kinds]
        assert _runs(ctx, pos, depth, introns, length, trim) == [want[k % 4] for k in range(len(introns))]


def test_overlapping_pieces_of_different_introns_at_random(ctx):
    rng = np.random.default_rng(20261020)
    for n_bound, max_depth in ((0, 1), (1, 3), (300, 40), (300, 2 ** 32 - 1)):
        length = 700
        pos, depth = I.random_bounds(rng, length, n_bound, max_depth)
        introns = [I.random_pieces(rng, length, int(rng.integers(1, 8))) for _ in range(150)] + [[(0, length)]] * 2
        _both(ctx, pos, depth, introns, length)


def test_the_greatest_depth_over_1000_bases_is_exact(ctx):
    top = 2 ** 32 - 1
    assert _runs(ctx, [0], [top], [[(0, 1000)]], 1000, 0) == [(1000, 1000, 1000, 1000 * top)]
    assert _runs(ctx, [0, 1000], [top, top - 1], [[(0, 2000)]], 2000, 30) == [(2000, 2000, 800, 400 * (top - 1) + 400 * top)]
    assert _runs(ctx, [5], [top], [[(0, LONG + 5)]], LONG + 5, 0) == [(LONG + 5, LONG, LONG + 5, LONG * top)]          # a team's sum


# ---- 2: over a read set -------------------------------------------------------------------------------------------------------
LENGTH = 6000


@pytest.fixture(scope="module")
def content():
    """4000 random reads of every kind on 6000 bases, the introns of random features (pieces clipped to 5100 bases, the length the
    reads are covered at), and the yardstick's per-base depth per track, computed once."""
    rng = np.random.default_rng(20261021)
    features = G.random_features(rng, LENGTH - 700, 9, 30)
    rs = samio.ReadSet.from_records(G.random_records(rng, 4000, LENGTH - 700))
    length = LENGTH - 900          # (reads run past it, features too)
    depth = {(0, "."): C.depth_of(rs, length)[0]}
    for stranded in (1, 2):
        for track in "+-":
            depth[(stranded, track)] = C.depth_of(rs, length, 0, stranded, track)[0]
    introns = {track: [x[3] for x in I.introns_of(features, track, length)] for track in ".+-"}
    assert all(len(v) > 3 for v in introns.values()) and any(len(p) > 1 for p in introns["."]) and any(not p for v in introns.values() for p in v)
    assert int(rs.pos.max()) + 20 > length
    return dict(rs=rs, length=length, depth=depth, introns=introns)


@pytest.mark.parametrize("stranded", [0, 1, 2])
def test_a_read_set_against_the_per_base_depth_and_against_its_own_runs(ctx, content, stranded):
    rs, length = content["rs"], content["length"]
    with ctx.upload_soa([native.ReadArrays(rs.pos, rs.flag, rs.cig_off, rs.cigar)]) as soa:
        with ctx.begin_reads() as dr:
            dr.add_soa(soa, 0)
            dr.finish()
            for track in (".",) if not stranded else ("+", "-"):
                introns = content["introns"][track]
                strand = 0 if not stranded else track
                per_base = content["depth"][(stranded, track)]
                start, end, depth, _ = dr.coverage(length, stranded, strand)
                # the boundaries of the runs that come down: a run's start, and its end where no run follows at once
                pos, dep = [], []
                for s, e, d in zip(start.tolist(), end.tolist(), depth.tolist()):
                    if pos and pos[-1] == s:
                        pos.pop(), dep.pop()
                    pos += [s, e]
                    dep += [d, 0]
                if pos and pos[-1] >= length:
                    pos.pop(), dep.pop()
                for trim in TRIMS:
                    got = dr.intron_depth(length, *_tables(introns), trim_percent=trim, stranded=stranded, strand=strand)
                    assert [tuple(r) for r in got.tolist()] == [I.stats_of(per_base, pieces, trim) for pieces in introns]
                    assert np.array_equal(got, native.intron_depth_runs(ctx, pos, dep, length, *_tables(introns), trim_percent=trim))
                assert int(got[:, 1].sum()) > 0
            assert dr.layout_bytes()[1] == 0          # (the set stays fused)


def test_a_set_without_a_read(ctx):
    with ctx.begin_reads() as dr:
        dr.finish()
        got = dr.intron_depth(100, *_tables([[(0, 10)], [], [(5, 6), (8, 100)]]), trim_percent=30)
        assert got.tolist() == [[10, 0, 4, 0], [0, 0, 0, 0], [93, 0, 39, 0]]
        assert dr.intron_depth(100, [0], [], []).shape == (0, 4)


# ---- 3: refusals --------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_working(ctx, content):
    rs, length = content["rs"], content["length"]
    fine = _tables([[(0, 10), (20, 30)], [(5, 25)]])
    bounds = ([3, 9], [1, 0])

    def works():
        assert _runs(ctx, [3, 9], [2, 0], [[(0, 10)]], 100, 0) == [(10, 6, 10, 12)]

    for args, kw, match in (((bounds[0], bounds[1], 100) + fine, dict(trim_percent=50), "trim_percent must be in 0 .. 49, not 50"),
                            ((bounds[0], bounds[1], 100) + fine, dict(trim_percent=-1), "trim_percent"),
                            ((bounds[0], bounds[1], 100, [1, 2, 3], fine[1], fine[2]), {}, "piece_off does not begin at 0"),
                            ((bounds[0], bounds[1], 100, [0, 2, 1], fine[1], fine[2]), {}, "piece_off decreases at intron 1"),
                            ((bounds[0], bounds[1], 100, [0, 1], [5], [5]), {}, "ends at or before its start"),
                            ((bounds[0], bounds[1], 100, [0, 1], [-1], [5]), {}, "outside"),
                            ((bounds[0], bounds[1], 100, [0, 1], [50], [101]), {}, "outside"),
                            ((bounds[0], bounds[1], 100, [0, 2], [0, 9], [10, 12]), {}, "not strictly ascending and disjoint at piece 1"),
                            ((bounds[0], bounds[1], 100, [0, 2], [20, 0], [30, 10]), {}, "disjoint"),
                            (([3, 3], [1, 0], 100) + fine, {}, "boundaries are not strictly ascending at entry 1"),
                            (([9, 3], [1, 0], 100) + fine, {}, "boundaries"),
                            ((bounds[0], bounds[1], 0) + fine, {}, "length"),
                            ((bounds[0], bounds[1], 2 ** 31 - 1) + fine, {}, "length")):
        with pytest.raises(native.SpliserNativeError, match=match) as err:
            native.intron_depth_runs(ctx, *args, **kw)
        assert err.value.code == -1
        works()
    # pieces of different introns may overlap; a piece may end at `length`; pieces may abut
    assert _runs(ctx, [3, 9], [2, 0], [[(0, 10), (10, 100)], [(5, 25)]], 100, 0) == [(100, 6, 100, 12), (20, 4, 20, 8)]
    with ctx.upload_soa([native.ReadArrays(rs.pos, rs.flag, rs.cig_off, rs.cigar)]) as soa:
        with ctx.begin_reads() as dr:
            dr.add_soa(soa, 0)
            with pytest.raises(native.SpliserNativeError, match="not finished"):
                dr.intron_depth(length, *fine)
            dr.finish()
            for kw, match in ((dict(stranded=3), "stranded"), (dict(stranded=0, strand="+"), "strand must be"), (dict(stranded=1, strand=0), "strand must be"),
                              (dict(trim_percent=50), "trim_percent")):
                with pytest.raises(native.SpliserNativeError, match=match):
                    dr.intron_depth(length, *fine, **kw)
            for bad_length in (0, 2 ** 31 - 1):
                with pytest.raises(native.SpliserNativeError, match="length"):
                    dr.intron_depth(bad_length, *fine)
            with pytest.raises(native.SpliserNativeError, match="outside"):
                dr.intron_depth(25, *fine)
            per_base = content["depth"][(0, ".")]
            got = dr.intron_depth(length, *fine)
            assert [tuple(r) for r in got.tolist()] == [I.stats_of(per_base, p, 30) for p in ([(0, 10), (20, 30)], [(5, 25)])]
    works()


# ---- 4: the command -----------------------------------------------------------------------------------------------------------
NAMES, LENGTHS = ["c1", "c2", "c3"], [20300, 15000, 10 ** 6]
IDS = ["gene%02d" % k for k in range(12)]
SPAN = 20000


def _gtf_text(features_by_chrom):
    text = "##gtf of the tests\n"
    for chrom in ("c4", "c2", "c1"):               # (the annotation's order is not the alignment file's; c4 is not in that file)
        for k, (left, right, strand, gene) in enumerate(features_by_chrom.get(chrom, [])):
            attrs = ('gene_id "%s"; transcript_id "t%d";' % (IDS[gene], k)) if k % 2 else ("ID=e%d;gene_id=%s" % (k, IDS[gene]))
            text += "%s\tsynth\texon\t%d\t%d\t.\t%s\t.\t%s\n" % (chrom, left + 1, right, strand, attrs)
    return text


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """Two chromosomes of some 3000 reads with features (genes 0..7 on c1, 4..11 on c2; c2's LN cuts its reads and its pieces), c3
    with reads and no feature, c4 with features and not in the file.  Among the random reads, spliced reads that begin and end where
    every third intron does, or at one of its ends only.  As a sorted BAM, its SAM text and a shuffled BAM."""
    d = tmp_path_factory.mktemp("idec")
    rng = np.random.default_rng(41)
    features = {}
    for k, chrom in enumerate(NAMES[:2]):
        features[chrom] = [(l, r, s, g + 4 * k) for l, r, s, g in G.random_features(rng, SPAN, 8, 40)]
    features["c4"] = [(100, 200, "+", 0), (300, 400, "+", 0), (250, 260, "-", 11)]
    sets = []
    for chrom in NAMES:
        recs = [r for r in G.random_records(rng, 3200, SPAN) if r[1] >= 1 and r[2]][:3000]
        for n, (_, s, e, _) in enumerate(I.introns_of(features.get(chrom, []), ".")[::3]):
            flag = G.STRAND_FLAGS[n % 6]
            if s >= 20:
                recs += [(flag, s - 19, "20M%dN20M" % (e - s))] * 2 + [(flag, s - 19, "20M%dN10M" % (e - s + 7))]
            if e - s > 3 and s >= 7:
                recs.append((G.STRAND_FLAGS[(n + 1) % 6], s + 3 - 9, "10M%dN10M" % (e - s - 3)))
        sets.append((chrom, samio.ReadSet.from_records(sorted(recs, key=lambda r: r[1]))))
    bam, sam, mixed, gtf = str(d / "d.bam"), str(d / "d.sam"), str(d / "mixed.bam"), str(d / "genes.gtf")
    samio.write_bam(bam, NAMES, LENGTHS, sets, with_seq=True, unplaced=3)
    with open(sam, "w") as fh:
        fh.write("@HD\tVN:1.6\tSO:coordinate\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % (n, ln) for n, ln in zip(NAMES, LENGTHS)))
        for chrom, rs in sets:
            for k in range(rs.n):
                fh.write("\t".join(["r", str(rs.flag[k]), chrom, str(rs.pos[k]), "60", samio.cigar_string(rs.cigar[rs.cig_off[k]:rs.cig_off[k + 1]]), "*", "0", "0", "*", "*"]) + "\n")
    O.write_bam(mixed, NAMES, LENGTHS, O.shuffled(O.records_of([rs for _, rs in sets]), 11))
    text = _gtf_text(features)
    open(gtf, "w").write(text)
    ids, by_chrom = G.features_of_text(text)
    assert ids == IDS and list(by_chrom) == ["c4", "c2", "c1"]
    return dict(dir=str(d), bam=bam, sam=sam, mixed=mixed, gtf=gtf, sets=sets, by_chrom=by_chrom, texts={})


def _want(f, stranded=0, exclude=0, only=None, trim=30):
    """The yardstick's file text (kept per kind of run)."""
    key = (stranded, exclude, trim)
    if key not in f["texts"]:
        depths, junctions = {}, {}
        for (chrom, rs), length in zip(f["sets"], LENGTHS):
            keep = ((rs.flag & exclude) == 0).tolist()
            for track in I.tracks_of(stranded):
                depths[(chrom, track)] = C.depth_of(rs, length, 0, stranded, 0 if not stranded else track, keep)[0]
            junctions[chrom] = I.junction_rows(rs, stranded, keep)
        f["texts"][key] = (depths, junctions)
    depths, junctions = f["texts"][key]
    return I.file_text(I.rows_of(IDS, ["c4", "c2", "c1"], f["by_chrom"], stranded, trim, dict(zip(NAMES, LENGTHS)), depths, junctions, only))


RUNS = {
    "gpuDecode": (lambda f: ["-B", f["bam"], "--gpuDecode"], {}),
    "hostDecode": (lambda f: ["-B", f["bam"], "--hostDecode"], {}),
    "gpuDecode fr": (lambda f: ["-B", f["bam"], "--gpuDecode", "--isStranded", "-s", "fr"], dict(stranded=1)),
    "hostDecode fr": (lambda f: ["-B", f["bam"], "--hostDecode", "--isStranded", "-s", "fr"], dict(stranded=1)),
    "one chromosome": (lambda f: ["-B", f["bam"], "-c", "c2"], dict(only="c2")),
    "excludeFlags": (lambda f: ["-B", f["bam"], "--excludeFlags", "0x900"], dict(exclude=0x900)),
    "SAM text": (lambda f: ["-B", f["sam"]], {}),
    "anyOrder": (lambda f: ["-B", f["mixed"], "--anyOrder"], {}),
    "trimPercent 0 rf": (lambda f: ["-B", f["sam"], "--trimPercent", "0", "--isStranded", "-s", "rf"], dict(stranded=2, trim=0)),
}


@pytest.mark.parametrize("name", list(RUNS))
def test_command_byte_for_byte(files, name, capsys):
    f = files
    argv, kind = RUNS[name]
    prefix = os.path.join(f["dir"], name.replace(" ", "_"))
    assert cli.main(["intronretention", "-A", f["gtf"], "-o", prefix] + argv(f)) == 0
    log = capsys.readouterr().out
    want = _want(f, **kind)
    assert open(prefix + ".introns.tsv").read() == want
    rows = [line.split("\t") for line in want.splitlines()[1:]]
    assert "introns, " in log and "measurable bases" in log and "Annotation: " in log
    if name == "gpuDecode":
        plain = rows
        assert [r for r in plain if r[2] == "c4"] == [["gene00:I001", "gene00", "c4", "201", "300", ".", "90", "0", "36", "0", "0.0", "0", "0", "0", "NA"]]
        assert any(int(r[13]) >= 2 for r in plain) and any(int(r[11]) > int(r[13]) for r in plain) and any(int(r[12]) > int(r[13]) for r in plain)      # exact, left only, right only
        assert any(r[6] == "0" and r[14] == "NA" for r in plain) and any(r[14] not in ("NA", "0.0", "1.0") for r in plain)
        assert any(not r[0].endswith("I001") and r[2] == "c1" for r in plain)
        assert want != _want(f, exclude=0x900) and want != _want(f, stranded=1)
    if name == "one chromosome":
        assert rows and all(r[2] == "c2" for r in rows) and set(want.splitlines()[1:]) < set(_want(f).splitlines()[1:])
    if name == "anyOrder":
        assert "is not in coordinate order" in log
