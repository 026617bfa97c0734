"""``coverage`` on the device: ``spl_coverage`` on fused sets against the yardstick of ``covcases.py`` -- exactly, the sums being
integers -- at the sizes where the kernels' geometry changes, on reads of every kind in any order, stranded and not; its refusals;
the three decodes and the command line, whose files are compared byte for byte."""
import numpy as np
import pytest

import covcases as C
import ordercases as O
import xscases as X
from spliser_amd import cli, coverage as cov, native, samio

pytestmark = pytest.mark.gpu

# The kernels' geometry (csrc/spl_coverage.h).  mark: a workgroup takes SPL_COV_TILE = 256 reads a grid-stride step, a read a lane,
# and a launch has at most SPL_COV_GRID_MAX = 1024 workgroups: EVERY workgroup takes a second step from 524 033 reads on, and
# 2 * 1024 * 256 + 1 gives the first one a third.  compact: a workgroup takes SPL_COV_POS_TILE = 1024 positions a step, four a lane,
# and a launch has at most SPL_COV_POS_GRID_MAX = 4096 workgroups.  The scans (csrc/spl_sort_wave.h) cut their input into parts of
# whole tiles of SCAN_TILE = 1024 words: more than 1024 boundaries, or more than 1024 position tiles, are more than one part.
TILE, GRID_MAX = 256, 1024
LARGE = 2 * GRID_MAX * TILE + 1
POS_TILE, POS_GRID_MAX = 1024, 4096
SCAN_TILE = 1024


@pytest.fixture(scope="module")
def ctx():
    with native.Context(0) as c:
        yield c


def _device(ctx, rs, length, stranded=0, strand=0, shift=0):
    with ctx.upload_soa([native.ReadArrays(rs.pos, rs.flag, rs.cig_off, rs.cigar)]) as soa:
        with ctx.begin_reads() as dr:
            dr.add_soa(soa, 0, shift)
            dr.finish()
            got = dr.coverage(length, stranded, strand)
            if rs.n:
                assert dr.layout_bytes()[1] == 0          # (the set stays fused)
            return got


def _boundaries(depth):
    """Positions of [0, length) at which the depth changes."""
    return int(np.count_nonzero(np.diff(np.concatenate(([0], depth)))))


def _same(got, depth, totals):
    """The library's (start, end, depth, totals) against the yardstick's per-base depth and its four counts."""
    want = C.runs_of(depth)
    start, end, d, t = got
    assert start.dtype == np.int32 and end.dtype == np.int32 and d.dtype == np.uint32
    assert C.same_runs(got, want)
    assert [t["reads_seen"], t["contributed"], t["past_end"], t["covered_bases"]] == totals and t["runs"] == want[0].shape[0]
    assert int(((end.astype(np.int64) - start) * d).sum()) == t["covered_bases"] == int(depth.sum())
    assert 0 <= t["contributed"] <= t["reads_seen"] and t["past_end"] <= t["reads_seen"]
    return want


def _check(ctx, rs, length, stranded=0, strand=0, shift=0):
    depth, totals = C.depth_of(rs, length, shift, stranded, strand)
    return depth, totals, _same(_device(ctx, rs, length, stranded, strand, shift), depth, totals)


def _concat(a, b):
    off = np.concatenate((a.cig_off.astype(np.int64), b.cig_off[1:].astype(np.int64) + int(a.cig_off[-1])))
    return samio.ReadSet(np.concatenate((a.pos, b.pos)), np.concatenate((a.flag, b.flag)), off, np.concatenate((a.cigar, b.cigar)))


def _permuted(rs, perm):
    n_ops = np.diff(rs.cig_off.astype(np.int64))[perm]
    off = np.concatenate(([0], np.cumsum(n_ops)))
    take = np.repeat(rs.cig_off.astype(np.int64)[perm] - off[:-1], n_ops) + np.arange(int(off[-1]))
    return samio.ReadSet(rs.pos[perm], rs.flag[perm], off, rs.cigar[take])


def _reads(records):
    """records: (flag, pos, cigar text), any order."""
    return samio.ReadSet.from_records(sorted(records, key=lambda r: r[1]))


# ---- reads --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, TILE - 1, TILE, TILE + 1])
def test_read_counts_around_a_wave_and_a_tile(ctx, n):
    rng = np.random.default_rng(200 + n)
    rs = X.make_reads(rng, n) if n else samio.ReadSet.empty()
    _, totals, _ = _check(ctx, rs, 140000)           # (make_reads places reads up to 150 000: where there are enough, some run past the end)
    assert totals[0] == n


def test_a_set_that_gives_every_workgroup_more_than_one_step(ctx):
    """LARGE reads, built as arrays: six in seven one aligned op, every seventh spliced; a tenth of them unmapped."""
    rng = np.random.default_rng(7)
    n, length = LARGE, 3000000
    pos = np.sort(rng.integers(1, length + 30, n)).astype(np.int32)
    flag = rng.choice(np.array([0, 16, 99, 147, 83, 163, 256, 1024, 512, 4], np.uint16), n)
    spliced = np.arange(n) % 7 == 3
    n_ops = np.where(spliced, 3, 1)
    off = np.concatenate(([0], np.cumsum(n_ops)))
    cigar = np.full(int(off[-1]), (50 << 4) | 0, np.uint32)
    cigar[off[:-1][spliced] + 1] = (rng.integers(70, 5000, int(spliced.sum())).astype(np.uint32) << 4) | 3
    rs = samio.ReadSet(pos, flag, off, cigar)
    _, totals, want = _check(ctx, rs, length)
    assert totals[0] == n and 0 < totals[2] < totals[1] < n and want[0].shape[0] > SCAN_TILE * 100


# ---- positions ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("length", [1, 2, POS_TILE - 1, POS_TILE, POS_TILE + 1, 4 * POS_TILE])
def test_lengths_around_a_tile_of_positions(ctx, length):
    """The first base, a block that ends on the last base, one clipped there, the last base alone, a read wholly beyond."""
    rs = _reads([(0, 1, "1M"), (0, max(1, length - 4), "5M"), (16, max(1, length - 2), "10M"), (0, length, "1M"), (256, length + 1, "3M"), (0, max(1, length // 2), "2M3N2M")])
    depth, totals, want = _check(ctx, rs, length)
    assert totals[0] == 6 and totals[2] >= 2 and int(want[1][-1]) == length and depth[0] > 0


def test_blocks_at_the_edges_of_a_tile(ctx):
    length = 4 * POS_TILE + 7
    edge = [(0, POS_TILE - 9, "10M"),            # ends exactly on the edge of tile 0: [1014, 1024)
            (0, 2 * POS_TILE, "5M"),             # starts on the last base of tile 1: [2047, 2052)
            (0, 3 * POS_TILE + 1, "1024M"),      # a whole tile: [3072, 4096)
            (0, 4 * POS_TILE + 1, "7M")]         # the tail behind the last whole tile, to the last base
    depth, _, want = _check(ctx, _reads(edge), length)
    assert want[0].tolist() == [POS_TILE - 10, 2 * POS_TILE - 1, 3 * POS_TILE] and want[1].tolist() == [POS_TILE, 2 * POS_TILE + 4, length]
    # tiles without a boundary between two that have some: nothing there at all, and a block that lies over them
    _, _, want = _check(ctx, _reads([(0, 5, "20M"), (16, 3 * POS_TILE + 50, "20M")]), length)
    assert want[0].shape[0] == 2
    _, _, want = _check(ctx, _reads([(0, 5, "20M"), (0, 10, "%dM" % (3 * POS_TILE + 100)), (16, 3 * POS_TILE + 50, "20M")]), length)
    assert want[2].tolist() == [1, 2, 1, 2, 1]
    # every boundary in the last tile
    _, _, want = _check(ctx, _reads([(0, 4 * POS_TILE + 2, "3M"), (0, 4 * POS_TILE + 3, "1M1D9M")]), length)
    assert int(want[0][0]) == 4 * POS_TILE + 1 and int(want[1][-1]) == length


def test_more_position_tiles_than_a_launch_has_workgroups(ctx):
    """Every workgroup of the compact kernels takes a second tile, the first a third; the tile counts are more than one part of the scan."""
    length = (2 * POS_GRID_MAX + 1) * POS_TILE + 3
    rng = np.random.default_rng(11)
    pos = np.sort(np.concatenate((rng.integers(1, length, 3000), [1, POS_GRID_MAX * POS_TILE, 2 * POS_GRID_MAX * POS_TILE + 1, length - 30, length])))
    rs = samio.ReadSet.from_records([(16 * (i & 1), int(p), "40M200N35M" if i % 3 == 0 else "60M") for i, p in enumerate(pos.tolist())])
    _, totals, want = _check(ctx, rs, length)
    assert totals[2] >= 2 and int(want[1][-1]) == length and int(want[0][0]) == 0


# ---- boundary counts ----------------------------------------------------------------------------------------------------------
def test_no_boundary_at_all(ctx):
    rs = _reads([(4, 10, "30M"), (0, 20, "30S"), (0, 5000, "30M"), (0, 40, "12I"), (0, 0, "30M")])      # unmapped, clips only, beyond the end, an insertion, no POS
    depth, totals, want = _check(ctx, rs, 2000)
    assert want[0].shape[0] == 0 and totals == [5, 0, 1, 0] and _boundaries(depth) == 0


@pytest.mark.parametrize("n_bound", [1, 2, 64, 65, SCAN_TILE, SCAN_TILE + 1, 2 * SCAN_TILE + 1, 5 * SCAN_TILE + 64])
def test_boundary_counts_around_a_wave_and_the_parts_of_the_scan(ctx, n_bound):
    """Disjoint reads of 15 bases 30 apart, two boundaries each; an odd count's last read is clipped by the length, which leaves it one."""
    n = (n_bound + 1) // 2
    length = 30 * n - (20 if n_bound % 2 else 0)
    rs = samio.ReadSet.from_records([(0, 1 + 30 * i, "15M") for i in range(n)])
    depth, totals, want = _check(ctx, rs, length)
    assert _boundaries(depth) == n_bound and want[0].shape[0] == n and totals[2] == n_bound % 2


def test_events_that_cancel(ctx):
    """A ends where B starts with equal depth either side: no boundary there.  C is clipped at the length: the last run ends there."""
    rs = _reads([(0, 11, "10M"), (16, 21, "10M"), (0, 91, "20M")])
    depth, totals, want = _check(ctx, rs, 100)
    assert [w.tolist() for w in want] == [[10, 90], [30, 100], [1, 1]] and totals == [3, 3, 1, 30] and _boundaries(depth) == 3
    # ... and the same under a deeper cover, where the sums at the shared position cancel to zero among four events
    rs = _reads([(0, 1, "60M"), (0, 11, "10M"), (16, 21, "10M"), (0, 11, "10M"), (16, 21, "10M")])
    _, _, want = _check(ctx, rs, 100)
    assert [w.tolist() for w in want] == [[0, 10, 30], [10, 30, 60], [1, 3, 1]]


def test_a_hot_locus(ctx):
    """100 000 reads with one POS and one CIGAR: every atomic of theirs lands on four words, and the depth leaves 16 bits."""
    n = 100000
    ops = np.array([(30 << 4) | 0, (100 << 4) | 3, (20 << 4) | 0], np.uint32)
    hot = samio.ReadSet(np.full(n, 501, np.int32), np.where(np.arange(n) % 2, 16, 0).astype(np.uint16), 3 * np.arange(n + 1), np.tile(ops, n))
    rs = _concat(_reads([(0, 480, "40M"), (16, 495, "10M5D10M")]), _concat(hot, _reads([(0, 640, "20M")])))
    depth, totals, want = _check(ctx, rs, 5000)
    assert int(want[2].max()) == n + 2 > 65535 and totals[1] == n + 3 and totals[3] == 50 * n + 40 + 20 + 20


# ---- CIGAR content ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def content():
    """Reads of every kind (``xscases.make_reads``: flags 0, 16, 99, 147, 83, 163, 256, 4; soft clips, one or two N ops, CIGARs of
    80 ops and more) and two reads of 2 203 ops; the yardstick's unstranded answer, computed once."""
    rng = np.random.default_rng(20261019)
    a = X.make_reads(rng, 3000, long_cigar_every=97)
    b = samio.ReadSet.from_records([(0, 20000, "1M1I" * 1100 + "5M300N7M"), (147, 90000, "1M1D" * 1100 + "5M300N7M")])
    rs = _concat(a, b)
    assert set(rs.flag.tolist()) == {0, 16, 99, 147, 83, 163, 256, 4} and int(np.diff(rs.cig_off.astype(np.int64)).max()) == 2203
    length = 149000                      # (the reads end at 149 969: a few of them run past the end)
    depth, totals = C.depth_of(rs, length)
    assert 0 < totals[2] < totals[1] < totals[0] == rs.n
    return rs, length, depth, totals


def test_reads_of_every_kind(ctx, content):
    rs, length, depth, totals = content
    want = _same(_device(ctx, rs, length), depth, totals)
    assert want[0].shape[0] > 2 * SCAN_TILE


def test_the_reads_in_any_order(ctx, content):
    rs, length, depth, totals = content
    prs = _permuted(rs, np.random.default_rng(5).permutation(rs.n))
    assert not np.array_equal(prs.pos, rs.pos)
    _same(_device(ctx, prs, length), depth, totals)


@pytest.mark.parametrize("shift", [5000000, -1000])
def test_a_set_added_with_a_shift(ctx, content, shift):
    """The runs lie where the segment was moved to; a shift below zero loses the bases in front of 0."""
    rs, length, depth, totals = content
    if shift > 0:
        _same(_device(ctx, rs, length + shift, shift=shift), np.concatenate((np.zeros(shift, np.int64), depth)), totals)
    else:
        _, moved, _ = _check(ctx, rs, length, shift=shift)
        assert moved[2] > totals[2]


def test_a_set_at_the_top_of_the_coordinate_space(ctx):
    """length = 2^31 - 2, the longest there is, and a segment moved up against the last coordinate a read set takes (2^31 - 67): the
    difference array is 8.6 GB, its words' byte offsets leave 32 bits.  Compared where the reads lie, not over 2^31 counters."""
    rs = _reads([(0, 1, "50M"), (16, 20, "40M"), (0, 900, "30M40N31M")])
    shift, length = 2147483581 - 1000, 2 ** 31 - 2
    start, end, d, t = _device(ctx, rs, length, shift=shift)
    depth, totals = C.depth_of(rs, 1000)
    w = C.runs_of(depth)
    assert np.array_equal(start.astype(np.int64) - shift, w[0]) and np.array_equal(end.astype(np.int64) - shift, w[1]) and np.array_equal(d, w[2])
    assert [t["reads_seen"], t["contributed"], t["past_end"], t["covered_bases"]] == totals == [3, 3, 0, 151]


# ---- stranded -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stranded", [1, 2])
def test_stranded_tracks(ctx, content, stranded):
    rs, length, depth, totals = content
    halves = []
    for strand in ("+", "-"):
        d, t, _ = _check(ctx, rs, length, stranded, strand)
        assert 0 < t[1] < totals[1] and t[0] == rs.n
        halves.append((d, t, _device(ctx, rs, length, stranded, strand)))
    plus, minus = (C.expand(h[2][0], h[2][1], h[2][2], length) for h in halves)
    assert np.array_equal(plus + minus, depth)                                         # per base, the two tracks add up to the unstranded depth
    assert halves[0][1][1] + halves[1][1][1] == totals[1] and halves[0][1][3] + halves[1][1][3] == totals[3]
    other = _device(ctx, rs, length, 3 - stranded, "-")                                  # rf's '-' track is fr's '+' track
    assert C.same_runs(other, halves[0][2])


# ---- errors -------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_working(ctx, content):
    rs, length, depth, totals = content
    arrays = native.ReadArrays(rs.pos, rs.flag, rs.cig_off, rs.cigar)
    dr = ctx.upload_reads(arrays)                  # (packed on the host: records, not arrays)
    try:
        with pytest.raises(native.SpliserNativeError, match="fused") as err:
            dr.coverage(length)
        assert err.value.code == -1
    finally:
        dr.free()
    with ctx.upload_soa([arrays]) as soa:
        with ctx.begin_reads() as dr:
            dr.add_soa(soa, 0)
            dr.finish()
            for bad in (0, -5, 2 ** 31 - 1, 2 ** 31, 2 ** 40):
                with pytest.raises(native.SpliserNativeError, match="length") as err:
                    dr.coverage(bad)
                assert err.value.code == -1
            for stranded in (-1, 3, 7):
                with pytest.raises(native.SpliserNativeError, match="stranded") as err:
                    dr.coverage(length, stranded, "+")
                assert err.value.code == -1
            for stranded, strand in ((0, "+"), (0, "-"), (1, 0), (2, 0), (1, "?"), (2, 1)):
                with pytest.raises(native.SpliserNativeError, match="strand") as err:
                    dr.coverage(length, stranded, strand)
                assert err.value.code == -1
            _same(dr.coverage(length), depth, totals)
    _same(_device(ctx, rs, length), depth, totals)


# ---- the decodes --------------------------------------------------------------------------------------------------------------
NAMES, LENGTHS = ["c1", "c2", "c3"], [10 ** 6, 400000, 10 ** 6]


@pytest.fixture(scope="module")
def decode_files(tmp_path_factory):
    d = tmp_path_factory.mktemp("cdec")
    rng = np.random.default_rng(31)
    sets = [(c, X.make_reads(rng, 1500, long_cigar_every=211)) for c in NAMES]
    bam, sam, mixed, bare = str(d / "d.bam"), str(d / "d.sam"), str(d / "mixed.bam"), str(d / "bare.sam")
    samio.write_bam(bam, NAMES, LENGTHS, sets, with_seq=True, unplaced=3)
    O.write_bam(mixed, NAMES, LENGTHS, O.shuffled(O.records_of([rs for _, rs in sets]), 9))

    def lines(chrom, rs):
        return ["\t".join(["r", str(rs.flag[k]), chrom, str(rs.pos[k]), "60", samio.cigar_string(rs.cigar[rs.cig_off[k]:rs.cig_off[k + 1]]), "*", "0", "0", "*", "*"]) + "\n"
                for k in range(rs.n)]
    with open(sam, "w") as fh:
        fh.write("@HD\tVN:1.6\tSO:coordinate\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % (n, ln) for n, ln in zip(NAMES, LENGTHS)))
        for chrom, rs in sets:
            fh.writelines(lines(chrom, rs))
    with open(bare, "w") as fh:          # no header: the Python reader's, and no lengths
        fh.writelines(lines(*sets[1]))
    return dict(dir=str(d), bam=bam, sam=sam, mixed=mixed, bare=bare, sets=sets)


_TEXTS = {}


def _want_text(sets, chroms=NAMES, exclude=0, stranded=0, strand=0, per_million_of=0, lengths=None):
    key = (tuple(chroms), exclude, stranded, strand, per_million_of, lengths is None)
    if key not in _TEXTS:
        text = ""
        for (chrom, rs), ln in zip(sets, lengths or LENGTHS):
            if chrom in chroms:
                depth, _ = C.depth_of(rs, ln, 0, stranded, strand, keep=(rs.flag & exclude) == 0)
                text += C.bedgraph_text(chrom, *C.runs_of(depth), per_million_of=per_million_of)
        _TEXTS[key] = text
    return _TEXTS[key]


@pytest.mark.parametrize("exclude", [0, 0x110])
def test_every_decode_writes_the_same_bytes(decode_files, exclude, capsys):
    f = decode_files
    got = {}
    for how, path, gpu in (("device", f["bam"], True), ("host", f["bam"], False), ("sam", f["sam"], None)):
        prefix = "%s/%s.%x" % (f["dir"], how, exclude)
        written = cov.coverage(path, prefix, gpuDecode=gpu, excludeFlags=exclude, log=lambda m: None)
        got[how] = open(prefix + ".bedgraph").read()
        assert written == {prefix + ".bedgraph": got[how].count("\n")}
    want = _want_text(f["sets"], exclude=exclude)
    assert want.count("\n") > 3000 and {line.split("\t")[0] for line in want.splitlines()} == set(NAMES)
    assert got["device"] == want and got["host"] == want and got["sam"] == want
    if exclude:
        assert want != _want_text(f["sets"])


def test_a_source_without_lengths_is_covered_up_to_its_last_base(decode_files, capsys):
    f = decode_files
    chrom, rs = f["sets"][1]
    prefix = f["dir"] + "/bare"
    assert cli.main(["coverage", "-B", f["bare"], "-o", prefix]) == 0
    depth, totals = C.depth_of(rs, int(rs.max_end))
    assert totals[2] == 0 and depth[-1] > 0
    assert open(prefix + ".bedgraph").read() == C.bedgraph_text(chrom, *C.runs_of(depth))
    with pytest.raises(native.SpliserNativeError, match="flagstat counters are counted while a BAM file is decoded"):
        cli.main(["coverage", "-B", f["bare"], "-o", prefix + ".pm", "--perMillion"])


# ---- the command line ---------------------------------------------------------------------------------------------------------
def test_command_plain_one_chromosome_and_stranded(decode_files, capsys):
    f = decode_files
    d = f["dir"]
    assert cli.main(["coverage", "-B", f["bam"], "-o", d + "/plain"]) == 0
    log = capsys.readouterr().out
    assert open(d + "/plain.bedgraph").read() == _want_text(f["sets"])
    assert all("  %s: " % c in log for c in NAMES) and "covered bases" in log and not open(d + "/plain.bedgraph").read().startswith("track")
    assert cli.main(["coverage", "-B", f["bam"], "-o", d + "/one", "-c", "c2"]) == 0
    assert open(d + "/one.bedgraph").read() == _want_text(f["sets"], chroms=["c2"])
    assert cli.main(["coverage", "-B", f["bam"], "-o", d + "/fr", "--isStranded", "-s", "fr"]) == 0
    plus, minus = open(d + "/fr.plus.bedgraph").read(), open(d + "/fr.minus.bedgraph").read()
    assert plus == _want_text(f["sets"], stranded=1, strand="+") and minus == _want_text(f["sets"], stranded=1, strand="-") and plus != minus
    assert cli.main(["coverage", "-B", f["sam"], "-o", d + "/rf", "--isStranded", "-s", "rf", "-c", "c3"]) == 0
    assert open(d + "/rf.plus.bedgraph").read() == _want_text(f["sets"], chroms=["c3"], stranded=2, strand="+")
    assert open(d + "/rf.minus.bedgraph").read() == _want_text(f["sets"], chroms=["c3"], stranded=1, strand="+")


def test_command_per_million(decode_files, capsys):
    f = decode_files
    d = f["dir"]
    mapped = sum(int(((rs.flag & 4) == 0).sum()) for _, rs in f["sets"])
    assert cli.main(["coverage", "-B", f["bam"], "-o", d + "/pm", "--perMillion"]) == 0
    assert ("Library size: %d mapped reads" % mapped) in capsys.readouterr().out
    assert open(d + "/pm.bedgraph").read() == _want_text(f["sets"], per_million_of=mapped)
    kept = sum(int(((rs.flag & (4 | 0x110)) == 0).sum()) for _, rs in f["sets"])          # the library size is the filtered file's
    assert cli.main(["coverage", "-B", f["sam"], "-o", d + "/pmx", "--perMillion", "--excludeFlags", "0x110"]) == 0
    assert 0 < kept < mapped and open(d + "/pmx.bedgraph").read() == _want_text(f["sets"], exclude=0x110, per_million_of=kept)


def test_command_on_a_file_in_any_order(decode_files, capsys):
    f = decode_files
    d = f["dir"]
    assert cli.main(["coverage", "-B", f["mixed"], "-o", d + "/mixed", "--anyOrder"]) == 0
    assert "not in coordinate order" in capsys.readouterr().out
    assert open(d + "/mixed.bedgraph").read() == _want_text(f["sets"])
