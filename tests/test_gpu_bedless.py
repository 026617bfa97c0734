"""`process` without -b on the GPU: the junction kernel of a fused read set (spl_junction_fused_kernel through spl_junctions)
against oracle.junction_table on the cases of junctioncases.py and on cases of the kernel's own limits -- the set stays fused,
and counts afterwards as before --; then the command end to end: byte for byte what `junctions` + `process -b` write, what the
real reference wrote for the golden junction cases, and what the oracle gives for a BED written from its own junction table."""
import os
import re
import sys

import numpy as np
import pytest

import helpers
import junctioncases as J
import limitcases as L
from oracle import oracle
from spliser_amd import cli, junctions as jn, native, process as proc, samio, synth
from test_gpu_configs import _files, _oracle_tsv
from test_gpu_junction_limits import Wants, _bam_cases, _case_of_set, _check_all, _count_and_check, _expected_bed, _share_holdings, _sorted, _table_for

pytestmark = pytest.mark.gpu

CHUNKS = (J.CHUNK, J.CHUNK_BIG)
with open(os.path.join(L.CSRC, "spl_junction_fused.h")) as _fh:
    _GEOMETRY = dict((k, int(v)) for k, v in re.findall(r"#define (SPL_J[A-Z]+) (\d+)", _fh.read()))
TILE, STAGE, SCAN = _GEOMETRY["SPL_JTILE"], _GEOMETRY["SPL_JSTAGE"], _GEOMETRY["SPL_JSCAN"]
M, N, D, I, S = J.M, J.N, J.D, J.I, J.S


@pytest.fixture(scope="module")
def ctx():
    with native.Context(0) as c:
        yield c


class _Fused(object):
    """A fused read set of a case's segments: upload_soa + add_soa with their shifts."""

    def __init__(self, ctx, segments):
        self.soa = ctx.upload_soa([native.ReadArrays(rs.pos, rs.flag, rs.cig_off, rs.cigar) for rs, _ in segments])
        self.dr = ctx.begin_reads()
        for k, (_, shift) in enumerate(segments):
            self.dr.add_soa(self.soa, k, shift)
        self.dr.finish()

    def __enter__(self):
        return self.dr

    def __exit__(self, *exc):
        self.dr.free()
        self.soa.free()


def _fused_check(ctx, oracle_lib, case, tag, count=True):
    want = Wants(case)
    with _Fused(ctx, case.segments) as dr:
        if case.reads.n:
            assert dr.layout_bytes()[1] == 0, tag + ("fused before",)
        _check_all(dr, case, want, tag)
        if case.reads.n:
            assert dr.layout_bytes()[1] == 0, tag + ("still fused after the junction table",)
            if count:
                _count_and_check(ctx, oracle_lib, dr, _table_for(case), case.reads, tag)
                assert dr.layout_bytes()[1] == 0, tag + ("still fused after the counting pass",)
                _check_all(dr, case, want, tag + ("again",))


# ---- the kernel --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", J.CASE_NAMES)
def test_fused_set_gives_the_restated_table_and_stays_fused(name, ctx, oracle_lib, monkeypatch):
    case = J.case(name)
    for chunk in CHUNKS:
        monkeypatch.setenv("SPL_FORCE_CHUNK", str(chunk))
        _fused_check(ctx, oracle_lib, case, (name, chunk))


@pytest.fixture(scope="module")
def bam_file(tmp_path_factory):
    cases = _bam_cases()
    names = ["r_%s" % c.name for c in cases]
    sets = [L.reads_from(_sorted(c.recs)) for c in cases]
    path = str(tmp_path_factory.mktemp("bedless") / "j.bam")
    native.write_bam(path, names, [1 << 30] * len(names), sets, level=1, threads=2, seq_mode=1)
    return path, names, cases, sets


def test_device_decoded_bam_stays_fused(ctx, oracle_lib, bam_file, monkeypatch):
    path, names, cases, sets = bam_file
    for chunk in CHUNKS:
        monkeypatch.setenv("SPL_FORCE_CHUNK", str(chunk))
        bam = native.BamFile(path, threads=2, defer=True)
        try:
            assert bam.decode_on_device(ctx), bam.decline_reason()
            for name, case, rs in zip(names, cases, sets):
                c = _case_of_set(case, rs)
                with ctx.begin_reads() as dr:
                    assert dr.add_bam(bam, name) == rs.n
                    dr.finish()
                    tag = (case.name, "add_bam", chunk)
                    assert dr.layout_bytes()[1] == 0, tag
                    _check_all(dr, c, Wants(c), tag)
                    assert dr.layout_bytes()[1] == 0, tag + ("after",)
                    if case.name in ("filter_boundaries", "hash", "shifted_segments"):
                        _count_and_check(ctx, oracle_lib, dr, _table_for(c), c.reads, tag)
        finally:
            bam.close()


def _spliced(i, flag=0):
    return (flag, 1000 + 3 * i, [(20 + i % 7, M), (100 + i % 3, N), (25 + i % 5, M)])


def _plain(i):
    return (0, 1000 + 3 * i, [(50, M)])


def _limit_cases():
    """Reads placed on the limits the fused kernel makes itself (tiles of TILE reads a workgroup, a stage of STAGE ops, SCAN ops
    looked through, the lists' ballots)."""
    cases = []
    filters = J.NO_FILTER + [(1, 0, 0), J.DEFAULTS, (8, 101, 101)]
    # a chunk whose reads all have one op: plain reads and lone N ops (junctions with min_anchor = 0 only); the next chunk has spliced ones
    recs = [((0, 1000 + i, [(30 + i % 4, N)]) if i % 97 == 0 else _plain(i)) for i in range(J.CHUNK_BIG)]
    recs += [_spliced(i) for i in range(J.CHUNK_BIG, J.CHUNK_BIG + 70)]
    cases.append(J.JCase("one_op_chunk", [(L.reads_from(recs), 0)], filters, "a chunk of one-op reads"))
    # exactly one lane of a tile / of a wave has an N op: at the tile's first, a middle and its last lane, and lane 63 / 64 of waves
    for where in (0, 63, 64, TILE - 1, TILE, 2 * TILE - 1, 5 * TILE + 130):
        recs = [_plain(i) for i in range(6 * TILE)]
        recs[where] = _spliced(where, 16)
        cases.append(J.JCase("one_lane_%d" % where, [(L.reads_from(recs), 0)], filters, "one lane with an N op"))
    # a WIDE read: more ops than the stage holds, N ops before, across and beyond the stage's end; reads after it in the same tile
    many = []
    for k in range(STAGE // 2 + 300):
        many += [(2 + k % 3, M), (100 + k % 5, N)]
    many.append((30, M))
    recs = [_spliced(i) for i in range(40)] + [(0, 2000, many)] + [_spliced(i, 99) for i in range(41, 120)] + [(16, 2500, many[10:])]
    cases.append(J.JCase("wide_beyond_stage", [(L.reads_from(recs), 0)], filters + [(2, 100, 102)], "N ops beyond the LDS stage", n_ops=len(many)))
    # ops that fill the stage exactly / one more (the last staged read ends on the stage's last word, the next one is read from memory)
    for extra in (0, 1, 4):
        recs = [_spliced(i) for i in range(100)]
        recs.append((0, 5000, [(1, M)] * (STAGE - 3 * len(recs) - 3 + extra) + [(20, M), (150, N), (20, M)]))
        recs += [_spliced(len(recs) + i) for i in range(30)]
        assert len(recs) < TILE
        cases.append(J.JCase("stage_edge_%d" % extra, [(L.reads_from(recs), 0)], filters, "a read across the stage's end"))
    # more ops than a lane looks through, with the only N op after them; and exactly SCAN ops with the N op last
    recs = [_plain(i) for i in range(100)]
    recs.append((0, 3000, [(2, M), (1, I)] * (SCAN // 2) + [(9, M), (120, N), (30, M)]))
    recs.append((0, 3100, [(2, M)] * (SCAN - 1) + [(120, N)]))
    recs.append((0, 3200, [(2, M)] * (SCAN - 2) + [(120, N), (9, M)]))
    cases.append(J.JCase("scan_limit", [(L.reads_from(recs), 0)], filters, "the N op behind the ops a lane looks through"))
    # N as the first and as the last op, alone and next to clips
    recs = [_plain(0), (0, 1200, [(90, N), (30, M)]), (16, 1300, [(30, M), (90, N)]), (0, 1400, [(5, S), (90, N), (30, M)]), (0, 1500, [(30, M), (90, N), (4, S)]),
            (0, 1600, [(90, N)]), (0, 1700, [(90, N), (80, N)]), (0, 1, [(90, N), (10, M)]), (0, 0, [(90, N), (10, M)])]
    cases.append(J.JCase("n_first_last", [(L.reads_from(recs), 0)], filters, "N first / last"))
    # segments with shifts that begin at any index of the arrays (not on a chunk or tile boundary), some of them tiny
    segs = []
    for k, n in enumerate((1, TILE - 1, 3, J.CHUNK + 5, 2, TILE + 1)):
        recs = [(_spliced(i, 147) if (i + k) % 5 == 0 else _plain(i)) for i in range(n)]
        segs.append((L.reads_from(recs), 1000 * k + 7))
    cases.append(J.JCase("segments_anywhere", segs, filters, "segments that begin at any index"))
    return cases


@pytest.mark.parametrize("k", range(15))
def test_limits_of_the_fused_kernel(k, ctx, oracle_lib, monkeypatch):
    cases = _limit_cases()
    assert len(cases) == 15
    case = cases[k]
    assert any(len(case.want(0, *f)) > 0 for f in case.filters)
    for chunk in CHUNKS:
        monkeypatch.setenv("SPL_FORCE_CHUNK", str(chunk))
        _fused_check(ctx, oracle_lib, case, (case.name, chunk), count=case.name in ("wide_beyond_stage", "segments_anywhere", "one_op_chunk"))


def test_walk_past_coord_max_is_refused_and_the_context_recovers(ctx, oracle_lib):
    bad = J.beyond_coord_max()
    good = J.filter_boundaries_case()
    for stranded, knobs in ((0, (0, 0, 0)), (1, J.DEFAULTS)):
        with _Fused(ctx, [(bad, 0)]) as dr:
            with pytest.raises(native.SpliserNativeError) as err:
                dr.junctions(stranded, *knobs)
            assert err.value.code == -6
            assert dr.layout_bytes()[1] == 0
        _fused_check(ctx, oracle_lib, good, ("after the range error", stranded))
    top = J.coordinates_case()
    _fused_check(ctx, oracle_lib, top, ("ends at SPL_COORD_MAX",), count=False)


def test_table_is_sized_by_the_junction_ops(ctx):
    """The fused set's table follows the N ops that pass the intron filter, not all ops: 40 bytes a slot, the smallest table for
    a set of many ops and few junctions."""
    recs = [_plain(i) for i in range(50000)] + [_spliced(i) for i in range(50000, 50100)]
    rs = L.reads_from(recs)
    with _Fused(ctx, [(rs, 0)]) as dr:
        got = dr.junctions(0, 0, 0, 0)
        assert J.rows(got) == oracle.junction_table(rs.pos, rs.flag, rs.cig_off, rs.cigar, 0)
        assert dr.junctions_stats()[0] == J.MIN_SLOTS * 40 + 256
    dr = ctx.upload_reads(native.ReadArrays(rs.pos, rs.flag, rs.cig_off, rs.cigar))
    try:
        dr.junctions(0, 0, 0, 0)
        assert dr.junctions_stats()[0] == J.n_slots(int(rs.cig_off[-1])) * 40 + 256 > J.MIN_SLOTS * 40 + 256
    finally:
        dr.free()


def test_collisions_and_the_wrap_at_the_fused_tables_own_size(ctx):
    """junctioncases' hash case collides for the packed path's table (a slot per op).  The fused set's table follows 2 x the N
    ops: 1024 reads of one distinct junction each give exactly 2048 slots, HALF full -- the highest load the sizing allows -- with
    60 keys whose home is slot mask - 9 (the probe runs past the last slot to slot 0 and on) and 4 whose home is slot 1 (they
    meet the wrapped run).  One more N op and the table doubles."""
    slots = 2 * J.MIN_SLOTS
    mask = slots - 1
    hot = J._colliding(60, mask - 9, mask, 400000)
    low = J._colliding(4, 1, mask, max(hot)[0] + 5000)
    placed = J.place([J.key_of(l, r) for l, r in sorted(hot + low)], slots)
    assert max(placed.values()) == mask and min(placed.values()) == 0           # the run does wrap
    rest = [(20_000_000 + 1000 * i, 20_000_000 + 1000 * i + 200) for i in range(J.MIN_SLOTS - 64)]
    recs = [(0, l + 1 - 30, [(30, M), (r - l, N), (20 + k % 9, M)]) for k, (l, r) in enumerate(sorted(hot + low + rest))]
    assert len(recs) == J.MIN_SLOTS
    for extra, want_slots in ((0, slots), (1, 2 * slots)):
        rs = L.reads_from(recs + [recs[-1]] * extra)
        case = J.JCase("fused_hash", [(rs, 0)], J.NO_FILTER, "collisions at the fused table's mask")
        with _Fused(ctx, case.segments) as dr:
            _check_all(dr, case, Wants(case), ("fused_hash", extra))
            assert len(dr.junctions(0)["left"]) == J.MIN_SLOTS
            assert dr.junctions_stats()[0] == want_slots * 40 + 256


# ---- the command, end to end --------------------------------------------------------------------------------------------------------

def _two_commands(bam, tmp_path, jflags, pflags, tag):
    """`junctions` + `process -b` against `process` alone: the .SpliSER.tsv files and the kept junction file, byte for byte."""
    bed, one, two = str(tmp_path / (tag + ".j.bed")), str(tmp_path / (tag + ".one")), str(tmp_path / (tag + ".two"))
    assert cli.main(["junctions", "-B", bam, "-o", bed] + jflags) == 0
    assert cli.main(["process", "-B", bam, "-b", bed, "-o", two] + pflags) == 0
    knobs = []
    for short, long in (("-a", "--minAnchor"), ("-m", "--minIntron"), ("-M", "--maxIntron")):
        if short in jflags:
            knobs += [long, jflags[jflags.index(short) + 1]]
    assert cli.main(["process", "-B", bam, "-o", one, "--keepJunctions"] + knobs + pflags) == 0
    got, want = open(one + ".SpliSER.tsv", "rb").read(), open(two + ".SpliSER.tsv", "rb").read()
    assert got == want, tag
    if "-c" in pflags:      # (the kept file is the one `junctions -c` writes)
        bed = bed + ".c"
        assert cli.main(["junctions", "-B", bam, "-o", bed, "-c", pflags[pflags.index("-c") + 1]] + jflags) == 0
    assert open(one + ".junctions.bed", "rb").read() == open(bed, "rb").read(), tag
    return got


@pytest.fixture(scope="module")
def arab(tmp_path_factory):
    wl = synth.Workload("arabidopsis", scale=0.01, seed=31, workers=4)
    for r in wl.reads:
        r.flag[:] = np.random.default_rng(5).choice(np.array([99, 147, 83, 163, 0, 16], np.uint16), size=r.n)
    prefix = str(tmp_path_factory.mktemp("arab") / "a")
    _files(wl, prefix, seq_mode=1)
    return wl, prefix


@pytest.mark.parametrize("tag,jflags,pflags", [
    ("unstranded", [], []),
    ("fr", ["--isStranded", "-s", "fr"], ["--isStranded", "-s", "fr"]),
    ("rf", ["--isStranded", "-s", "rf"], ["--isStranded", "-s", "rf"]),
    ("cryptic", [], ["--beta2Cryptic"]),
    ("chrom", [], ["-c", "Chr3"]),
    ("every_n_op", ["-a", "0", "-m", "0", "-M", "0"], []),
    ("host_decode", [], ["--hostDecode"]),
    ("annotated_shares", [], ["-A", "GFF", "--devices", "0,0,0"]),
    ("fr_cryptic_shares", ["--isStranded", "-s", "fr"], ["--isStranded", "-s", "fr", "--beta2Cryptic", "--devices", "0,0,0"]),
])
def test_one_command_writes_what_the_two_write(tag, jflags, pflags, arab, tmp_path):
    wl, prefix = arab
    pflags = [prefix + ".gff" if f == "GFF" else f for f in pflags]
    if "--devices" in pflags:
        bam, held = _share_holdings(prefix + ".bam", wl.genome.chrom_names)
        bam.close()
        assert any(sum(1 for k in range(len(held)) if held[k][j] > 0) > 1 for j in range(len(wl.genome.chrom_names)))   # a chromosome is cut
    text = _two_commands(prefix + ".bam", tmp_path, jflags, pflags, tag)
    assert text.count(b"\n") > 100


def test_one_command_on_the_limit_cases_in_shares(bam_file, tmp_path):
    path, names, cases, sets = bam_file
    bam, held = _share_holdings(path, names)
    bam.close()
    assert any(sum(1 for k in range(len(held)) if held[k][j] > 0) > 1 for j in range(len(names)))
    for tag, jflags, pflags in (("u", [], []), ("fr", ["--isStranded", "-s", "fr", "-a", "1", "-m", "0", "-M", "0"], ["--isStranded", "-s", "fr"])):
        _two_commands(path, tmp_path, jflags, pflags + ["--devices", "0,0,0"], "limits_" + tag)
        # ... and the kept file is the restated one
        stranded, knobs = (1, (1, 0, 0)) if jflags else (0, J.DEFAULTS)
        assert open(str(tmp_path / ("limits_" + tag + ".one.junctions.bed"))).read() == _expected_bed(names, sets, stranded, *knobs)


def test_gene_query_on_the_single_gene_golden(tmp_path):
    d = os.path.join(helpers.GOLDEN, "single_gene")
    names, sets = samio.read_sam(os.path.join(d, "reads.sam"))
    bam = str(tmp_path / "g.bam")
    samio.write_bam(bam, names, [10 ** 8] * len(names), [(c, sets[c]) for c in names if c in sets])
    flags = ["-A", os.path.join(d, "genes.gff"), "-g", "AT1G01060", "-c", "Chr1", "-m", "6000"]
    for tag, jf, pf in (("gene", ["-a", "1", "-m", "1", "-M", "0"], flags), ("gene_fr", ["-a", "1", "-m", "1", "-M", "0", "--isStranded", "-s", "fr"],
                                                                             flags + ["--isStranded", "-s", "fr", "--beta2Cryptic"])):
        bed, one, two = str(tmp_path / (tag + ".bed")), str(tmp_path / (tag + ".one")), str(tmp_path / (tag + ".two"))
        assert cli.main(["junctions", "-B", bam, "-o", bed] + jf) == 0
        assert cli.main(["process", "-B", bam, "-b", bed, "-o", two] + pf) == 0
        assert cli.main(["process", "-B", bam, "-o", one, "--minAnchor", "1", "--minIntron", "1", "--maxIntron", "0"] + pf) == 0
        got = open(one + ".SpliSER.tsv", "rb").read()
        assert got == open(two + ".SpliSER.tsv", "rb").read() and got.count(b"\n") > 3, tag


def test_the_real_references_output_on_the_golden_junction_cases(tmp_path):
    """tests/golden/junctions_*: expected.*.tsv is what the unmodified reference wrote from junctions.bed, which `junctions` wrote
    from reads.sam.  `process` without -b on reads.sam, with the knobs and options make_golden.py records, writes those files."""
    sys.path.insert(0, helpers.GOLDEN)
    from make_golden import JUNCTION_CASES, JUNCTION_KNOBS
    n = 0
    for name, case in JUNCTION_CASES.items():
        sam = os.path.join(helpers.GOLDEN, name, "reads.sam")
        for variant, opts in case["variants"].items():
            out = str(tmp_path / (name + "." + variant))
            proc.process(sam, None, out, isStranded=bool(opts.get("stranded")), strandedType=opts.get("stranded"),
                         isbeta2Cryptic=bool(opts.get("cryptic")), log=lambda m: None, keepJunctions=True, **JUNCTION_KNOBS)
            assert open(out + ".SpliSER.tsv").read() == open(os.path.join(helpers.GOLDEN, name, "expected.%s.tsv" % variant)).read(), (name, variant)
            assert open(out + ".junctions.bed").read() == open(os.path.join(helpers.GOLDEN, name, "junctions.bed")).read(), (name, variant)
            n += 1
    assert n == 4


@pytest.mark.parametrize("preset,stranded,knobs", [("arabidopsis", None, J.DEFAULTS), ("mouse_stranded", "fr", (3, 50, 0))])
def test_against_the_oracle_with_a_bed_from_its_own_junction_table(preset, stranded, knobs, tmp_path, oracle_lib):
    wl = synth.Workload(preset, scale=0.01, seed=41, workers=4)
    prefix = str(tmp_path / "o")
    _files(wl, prefix, seq_mode=1)
    scode = native.STRANDED_CODE[stranded]
    bed = prefix + ".oracle.bed"
    with open(bed, "w") as fh:
        fh.write(_expected_bed(wl.genome.chrom_names, wl.reads, scode, *knobs))
    argv = ["process", "-B", prefix + ".bam", "-o", prefix, "--minAnchor", str(knobs[0]), "--minIntron", str(knobs[1]), "--maxIntron", str(knobs[2])]
    argv += ["--isStranded", "-s", stranded, "--beta2Cryptic"] if stranded else []
    assert cli.main(argv) == 0
    want = _oracle_tsv(oracle_lib, bed, wl, stranded, bool(stranded))
    assert want.count("\n") > 100
    assert open(prefix + ".SpliSER.tsv").read() == want


def test_a_bam_without_a_spliced_read(tmp_path):
    recs = [_plain(i) for i in range(5000)]
    path = str(tmp_path / "plain.bam")
    native.write_bam(path, ["c1", "c2"], [1 << 20] * 2, [L.reads_from(recs), L.reads_from(recs[:100])], level=1, threads=2, seq_mode=1)
    empty = str(tmp_path / "empty.bed")
    open(empty, "w").close()
    one, two = str(tmp_path / "one"), str(tmp_path / "two")
    assert cli.main(["process", "-B", path, "-o", one, "--keepJunctions"]) == 0
    assert cli.main(["process", "-B", path, "-b", empty, "-o", two]) == 0
    from spliser_amd import tsv
    assert open(one + ".SpliSER.tsv").read() == open(two + ".SpliSER.tsv").read() == tsv.HEADER
    assert open(one + ".junctions.bed").read() == jn.track_line(*J.DEFAULTS)
