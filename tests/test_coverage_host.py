"""``coverage`` without a GPU: the per-read rule on the host (``spl_coverage_rule_host``) against the yardstick of ``covcases.py``,
the bedGraph writer (``spl_bedgraph_append``) against Python's own formatting, and the command line's refusals."""
import numpy as np
import pytest

import covcases as C
from spliser_amd import cli, native

PLUS, MINUS = C.PLUS, C.MINUS
LENGTH_MAX = 2 ** 31 - 2


def op(n, code):
    return (n << 4) | code


def _check(flag, pos, ops, length, shift=0, stranded=0, strand=0):
    want = C.blocks_of(flag, pos, ops, length, shift, stranded, strand)
    got = native.coverage_rule_host(flag, pos, ops, length, shift, stranded, strand)
    assert got == want, (flag, pos, ops, length, shift, stranded, strand)
    return want


@pytest.mark.parametrize("code", range(16))
def test_every_op_code(code):
    """Between two aligned stretches: M, = and X make one block of three, D and N a gap, everything else nothing at all."""
    blocks, past = _check(0, 101, [op(10, 0), op(7, code), op(5, 0)], 1000)
    assert not past
    if code in (0, 7, 8):
        assert blocks == [(100, 122)]
    elif code in (2, 3):
        assert blocks == [(100, 110), (117, 122)]
    else:
        assert blocks == [(100, 115)]
    alone, _ = _check(0, 101, [op(7, code)], 1000)
    assert alone == ([(100, 107)] if code in (0, 7, 8) else [])


def test_abutting_inserted_and_zero_length_ops():
    assert _check(0, 1, [op(10, 0), op(2, 1), op(5, 0)], 100)[0] == [(0, 15)]                     # 10M2I5M: one block
    assert _check(0, 1, [op(10, 0), op(0, 3), op(5, 0)], 100)[0] == [(0, 15)]                     # 10M0N5M: an op of no length does nothing
    assert _check(0, 1, [op(10, 0), op(0, 2), op(5, 7), op(0, 0), op(3, 8)], 100)[0] == [(0, 18)]
    assert _check(0, 1, [op(10, 0), op(1, 2), op(5, 0)], 100)[0] == [(0, 10), (11, 16)]           # a deletion of one base is a gap
    assert _check(0, 1, [op(0, 0)], 100) == ([], False)                                           # nothing covered: no block, nothing lost
    assert _check(0, 1, [op(3, 4), op(4, 0), op(2, 1), op(6, 3), op(2, 6), op(4, 0), op(3, 5)], 100)[0] == [(0, 4), (10, 14)]
    assert _check(0, 1, [op(5, 3), op(4, 0)], 100)[0] == [(5, 9)]                                  # a gap in front


def test_reads_that_cover_nothing():
    for ops in ([op(20, 4)], [op(5, 5), op(20, 4)], [op(3, 1)], [op(9, 2)], [op(9, 3), op(2, 1)], []):
        assert _check(0, 50, ops, 100) == ([], False)


def test_unmapped_and_unplaced_reads():
    ops = [op(30, 0)]
    assert _check(0x4, 10, ops, 100) == ([], False)
    assert _check(0x4 | 0x10 | 0x1, 10, ops, 100) == ([], False)
    assert _check(0, 0, ops, 100) == ([], False)
    assert _check(0, -1, ops, 100) == ([], False)
    for flag in (0x100, 0x200, 0x400, 0x800, 0x100 | 0x400 | 0x800 | 0x200):       # secondary, QC-failed, duplicate, supplementary: they count
        assert _check(flag, 10, ops, 100) == ([(9, 39)], False)


@pytest.mark.parametrize("length", [1, 39, 40, 41, 60, 61, 100])
def test_clipping_at_and_beyond_the_length(length):
    """30M10N20M at POS 11: blocks [10, 40) and [50, 70)."""
    blocks, past = _check(0, 11, [op(30, 0), op(10, 3), op(20, 0)], length)
    assert past == (length < 70)
    assert blocks == [(s, min(e, length)) for s, e in ((10, 40), (50, 70)) if s < length]


def test_clipping_with_a_shift():
    ops = [op(30, 0)]
    assert _check(0, 11, ops, 100, shift=60) == ([(70, 100)], False)
    assert _check(0, 11, ops, 100, shift=61) == ([(71, 100)], True)
    assert _check(0, 11, ops, 100, shift=90) == ([], True)
    assert _check(0, 11, ops, 100, shift=-10) == ([(0, 30)], False)
    assert _check(0, 11, ops, 100, shift=-25) == ([(0, 15)], True)          # a base lost below 0 is a base lost
    assert _check(0, 11, ops, 100, shift=-40) == ([], True)


def test_positions_near_the_end_of_the_coordinate_space():
    top = 2 ** 31 - 1
    ops = [op(100, 0), op(2 ** 28 - 1, 3), op(50, 0)]
    assert _check(0, top, ops, LENGTH_MAX) == ([], True)
    assert _check(0, top - 1, ops, LENGTH_MAX) == ([(LENGTH_MAX - 1, LENGTH_MAX)], True)      # (POS 2^31 - 2 is the last base there is)
    assert _check(0, top - 2, ops, LENGTH_MAX) == ([(LENGTH_MAX - 2, LENGTH_MAX)], True)
    assert _check(0, top - 100, [op(100, 0)], LENGTH_MAX) == ([(LENGTH_MAX - 100, LENGTH_MAX)], False)
    assert _check(0, top - 99, [op(100, 0)], LENGTH_MAX) == ([(LENGTH_MAX - 99, LENGTH_MAX)], True)
    assert _check(0, top, ops, LENGTH_MAX, shift=2 ** 31 - 1) == ([], True)         # 2^32 - 3 and beyond: int64 arithmetic
    many = [op(2 ** 28 - 1, 0)] * 20                                                # 20 abutting ops of the longest length: one block of 5.4e9 bases
    assert _check(0, 1, many, LENGTH_MAX) == ([(0, LENGTH_MAX)], True)
    assert _check(0, 1, many, LENGTH_MAX, shift=-(2 ** 31)) == ([(0, LENGTH_MAX)], True)


PAIRED = (99, 147, 83, 163, 65, 129, 81, 161, 97, 145, 113, 177)


@pytest.mark.parametrize("stranded", [1, 2])
def test_tracks_of_single_and_paired_flags(stranded):
    """Unpaired forward / reverse and the paired flags, all six of a proper pair's among them: each read is on exactly one track."""
    ops = [op(25, 0)]
    for flag in (0, 16) + PAIRED:
        on = [native.coverage_rule_host(flag, 5, ops, 100, 0, stranded, s)[0] for s in ("+", "-")]
        assert sorted(on) == [[], [(4, 29)]]
        mine = PLUS if on[0] else MINUS
        assert C.read_strand(flag, stranded) == mine and C.read_strand(flag, 3 - stranded) != mine
        for s in (PLUS, MINUS):
            _check(flag, 5, ops, 100, 0, stranded, s)
    assert native.coverage_rule_host(99, 5, ops, 100, 0, 1, "+")[0] and native.coverage_rule_host(147, 5, ops, 100, 0, 1, "+")[0]      # fr: a pair on one track
    assert native.coverage_rule_host(83, 5, ops, 100, 0, 1, "-")[0] and native.coverage_rule_host(163, 5, ops, 100, 0, 1, "-")[0]
    assert native.coverage_rule_host(0x4 | 99, 5, ops, 100, 0, stranded, "+") == ([], False)


def test_random_reads_against_the_yardstick():
    rng = np.random.default_rng(20261019)
    for _ in range(3000):
        n_ops = int(rng.integers(0, 9))
        ops = [op(int(rng.choice([0, 0, 1, 2, 5, 40])), int(rng.integers(0, 16) if rng.random() < 0.3 else rng.choice([0, 0, 1, 2, 3, 4, 7, 8]))) for _ in range(n_ops)]
        flag = int(rng.choice([0, 16, 99, 147, 83, 163, 256, 4, 1024]))
        stranded = int(rng.integers(0, 3))
        strand = 0 if stranded == 0 else int(rng.choice([PLUS, MINUS]))
        _check(flag, int(rng.integers(0, 140)), ops, int(rng.choice([1, 50, 100, 150])), int(rng.integers(-20, 20)), stranded, strand)


def test_rule_refusals():
    ops = [op(10, 0)]
    for length in (0, -1, 2 ** 31 - 1, 2 ** 40):
        with pytest.raises(native.SpliserNativeError, match="length") as err:
            native.coverage_rule_host(0, 1, ops, length)
        assert err.value.code == -1
    for stranded, strand in ((0, "+"), (1, 0), (2, 0), (1, "?"), (3, "+"), (-1, 0)):
        with pytest.raises(native.SpliserNativeError, match="strand") as err:
            native.coverage_rule_host(0, 1, ops, 100, 0, stranded, strand)
        assert err.value.code == -1


# ---- the bedGraph writer ------------------------------------------------------------------------------------------------------
DEPTHS = [1, 2, 3, 7, 999, 65535, 65536, 1000000, 2 ** 31, 2 ** 32 - 1]
AWKWARD_N = [1, 3, 7, 10, 999983, 1000000, 1000003, 33333333, 123456789, 2 ** 31 - 1, 2 ** 32 + 1, 10 ** 12 + 39]


def _lines(n):
    start = np.arange(n, dtype=np.int64) * 3
    start[-1] = 2 ** 31 - 12
    return start.astype(np.int32), (start + 2).astype(np.int32)


def test_bedgraph_integers(tmp_path):
    path = str(tmp_path / "a.bedgraph")
    start, end = _lines(len(DEPTHS))
    native.bedgraph_append(path, "chr1", start, end, DEPTHS)
    native.bedgraph_append(path, "scaffold_2|x", start[:2], end[:2], DEPTHS[-2:])          # appended, not rewritten
    native.bedgraph_append(path, "empty", [], [], [])
    want = C.bedgraph_text("chr1", start, end, DEPTHS) + C.bedgraph_text("scaffold_2|x", start[:2], end[:2], DEPTHS[-2:])
    assert open(path).read() == want
    assert want.splitlines()[-1] == "scaffold_2|x\t3\t5\t4294967295" and "\t2147483636\t2147483638\t" in want


@pytest.mark.parametrize("n", AWKWARD_N)
def test_bedgraph_per_million(tmp_path, n):
    path = str(tmp_path / "b.bedgraph")
    start, end = _lines(len(DEPTHS))
    native.bedgraph_append(path, "c", start, end, DEPTHS, per_million_of=n)
    want = C.bedgraph_text("c", start, end, DEPTHS, per_million_of=n)
    assert open(path).read() == want
    assert all("." in line.split("\t")[3] or "e" in line.split("\t")[3] for line in want.splitlines())      # floats, as Python writes them


def test_bedgraph_per_million_on_random_pairs(tmp_path):
    rng = np.random.default_rng(5)
    path = str(tmp_path / "c.bedgraph")
    want = ""
    for n in rng.integers(1, 2 ** 33, 40).tolist():
        depth = rng.integers(1, 2 ** 32, 50)
        start, end = _lines(50)
        native.bedgraph_append(path, "c", start, end, depth, per_million_of=n)
        want += C.bedgraph_text("c", start, end, depth, per_million_of=n)
    assert open(path).read() == want


def test_bedgraph_refusals(tmp_path):
    with pytest.raises(ValueError):
        native.bedgraph_append(str(tmp_path / "x"), "c", [1, 2], [3], [1, 1])
    with pytest.raises(native.SpliserNativeError) as err:
        native.bedgraph_append(str(tmp_path / "x"), "c", [1], [3], [1], per_million_of=-5)
    assert err.value.code == -1
    with pytest.raises(native.SpliserNativeError) as err:
        native.bedgraph_append(str(tmp_path / "no" / "such" / "dir"), "c", [1], [3], [1])
    assert err.value.code != 0


# ---- the command line ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("argv, match", [
    (["coverage", "-B", "x.bam", "-o", "p", "-s", "auto"], "strandedness"),
    (["coverage", "-B", "x.bam", "-o", "p", "--isStranded", "-s", "auto"], "strandedness"),
    (["coverage", "-B", "x.bam", "-o", "p", "--isStranded"], "--isStranded requires parameter --strandedType/-s as fr or rf"),
    (["coverage", "-B", "x.bam", "-o", "p", "--isStranded", "-s", "ff"], "fr or rf"),
    (["coverage", "-B", "x.bam", "-o", "p", "--minMapQ", "256"], "--minMapQ must be in 0..255"),
    (["coverage", "-B", "x.bam", "-o", "p", "--excludeFlags", "65536"], "must be in 0..65535"),
    (["coverage", "-B", "x.bam", "-o", "p", "--requireFlags", "0x10", "--excludeFlags", "0x110"], "share a bit"),
    (["coverage", "-B", "x.bam"], "-o/--outputPath"),
    (["coverage", "-o", "p"], "-B/--BAMFile"),
])
def test_parser_errors(argv, match, capsys):
    with pytest.raises(SystemExit) as err:
        cli.main(argv)
    assert err.value.code == 2
    assert match in capsys.readouterr().err


def test_the_parser_takes_what_the_issue_lists():
    args = vars(cli.build_parser().parse_args(["coverage", "-B", "x.sam.gz", "-o", "p", "-c", "chr2", "--isStranded", "-s", "rf", "--perMillion", "--anyOrder",
                                               "--hostDecode", "--minMapQ", "10", "--excludeFlags", "0x704", "--gpus", "2", "--threads", "3"]))
    assert (args["command"], args["qChrom"], args["isStranded"], args["strandedType"], args["perMillion"], args["anyOrder"], args["gpuDecode"]) == \
        ("coverage", "chr2", True, "rf", True, True, False)
    assert (args["minMapQ"], args["excludeFlags"], args["gpus"], args["threads"]) == (10, 0x704, 2, 3)
    assert native.COVERAGE_TOTALS == ("runs", "reads_seen", "contributed", "past_end", "covered_bases")
