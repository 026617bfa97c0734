"""``coverage --fragments`` and ``intronretention --fragments`` on the device: ``coverage(fragments=True)``
(``spl_coverage_fragments`` on the mate table of ``spl_mate_table``), ``junctions(fragments=True)`` (``spl_junctions_fragments``) and
``intron_depth(fragments=True)`` against the yardstick of ``covfragcases.py`` -- exactly, the sums being integers -- on generated
paired sets whose coverage is asserted, unstranded, fr, rf and moved by a shift; at the sizes where the kernels' geometry changes;
on hand cases with the mates in one wave, in other waves, in other workgroups and further apart than a launch has lanes; on reads in
any order, on a segment that does not begin the arrays and on two segments; at the edges of ``length``; on a hot locus; their
refusals; and through every decode, where one paired file goes in as BAM on the device, BAM on the host threads, SAM text, BGZF SAM
text and the BAM shuffled, and each command writes one and the same file."""
import os
import re

import numpy as np
import pytest

import covcases as C
import covfragcases as F
import genecases as G
import introncases as I
import junctioncases as J
import matecases as M
import samzcases as Z
from spliser_amd import cli, native, samio

pytestmark = pytest.mark.gpu


def _constant(header, name):
    """A geometry constant of csrc, read from its header."""
    text = open(os.path.join(os.path.dirname(os.path.abspath(native.__file__)), "csrc", header)).read()
    return int(re.search(r"#define %s (\d+)" % name, text).group(1))


TILE, GRID_MAX = _constant("spl_coverage.h", "SPL_COV_TILE"), _constant("spl_coverage.h", "SPL_COV_GRID_MAX")
JTILE, JSTAGE = _constant("spl_junction_fused.h", "SPL_JTILE"), _constant("spl_junction_fused.h", "SPL_JSTAGE")
LARGE = GRID_MAX * TILE + 2 * TILE + 1          # every workgroup gets a second grid-stride step
TRACKS = [(0, 0), (1, "+"), (1, "-"), (2, "+"), (2, "-")]
MODES = [(s, k) for s in (0, 1, 2, 3) for k in F.KNOBS]


@pytest.fixture(scope="module")
def ctx():
    with native.Context(0) as c:
        yield c


class _Set(object):
    """A finished, fused read set of segments [(ReadSet, keys or None)] with shifts, for the length of a ``with``."""

    def __init__(self, ctx, segs, shifts=None, xs=None, only=None):
        self.ctx, self.segs, self.shifts, self.xs, self.only = ctx, segs, shifts or [0] * len(segs), xs, only

    def __enter__(self):
        keyed = self.segs[0][1] is not None
        arrays = [native.ReadArrays(rs.pos, rs.flag, rs.cig_off, rs.cigar, xs=self.xs, name_key=None if k is None else np.asarray(k, np.uint64)) for rs, k in self.segs]
        self.soa = self.ctx.upload_soa(arrays, with_strand=self.xs is not None, with_keys=keyed)
        self.dr = self.ctx.begin_reads()
        for k in (range(len(self.segs)) if self.only is None else self.only):
            self.dr.add_soa(self.soa, k, self.shifts[k])
        self.dr.finish()
        return self.dr

    def __exit__(self, *exc):
        self.dr.free()
        self.soa.__exit__(*exc)


def _got(dr, length, stranded=0, strand=0, fragments=True):
    start, end, depth, totals = dr.coverage(length, stranded, strand, fragments=fragments)
    return (start, end, depth), [totals[k] for k in (native.COVERAGE_FRAGMENT_TOTALS if fragments else native.COVERAGE_TOTALS)]


def _check(dr, rs, keys, length, shift=0, stranded=0, strand=0, mate=None):
    """The device's runs and six totals are the yardstick's."""
    mate = M.mate_table_of(rs, keys)[0] if mate is None else mate
    runs, totals = F.want_of(rs, mate, length, shift, stranded, strand)
    got, got_totals = _got(dr, length, stranded, strand)
    assert C.same_runs(got, runs) and got_totals == totals
    assert totals[4] == int(((runs[1] - runs[0]) * runs[2]).sum())          # covered bases == sum((end - start) * depth)
    return runs, totals


@pytest.fixture(scope="module")
def content():
    """Generated paired content of every kind -- asserted --, more than eight tiles of it, its mate table by the yardstick and strand
    bytes for mode 3."""
    rs, keys, names = F.paired_content(np.random.default_rng(20261022), n_fragments=1000)
    seen = F.assert_covers(rs, keys)
    assert rs.n > 8 * TILE
    mate, counts = M.mate_table_of(rs, keys)
    xs = np.random.default_rng(3).choice(np.array([43, 45, 0], np.uint8), rs.n)
    return dict(rs=rs, keys=keys, mate=mate, counts=counts, seen=seen, xs=xs)


# ---- coverage: generated sets ---------------------------------------------------------------------------------------------------
def test_generated_pairs_on_every_track_and_per_read_as_before(ctx, content):
    rs, keys, mate = content["rs"], content["keys"], content["mate"]
    with _Set(ctx, [(rs, keys)]) as dr:
        per_read_before = {t: _got(dr, F.LENGTH, *t, fragments=False) for t in TRACKS[:3]}
        for stranded, strand in TRACKS:
            runs, totals = _check(dr, rs, keys, F.LENGTH, 0, stranded, strand, mate)
            assert totals[5] >= 10 and totals[3] >= (0 if stranded else 1)
            if not stranded:
                assert totals[5] == content["counts"]["paired"] // 2 and dr.mate_table(0)[1] == content["counts"]
        # the same set without the switch: spl_coverage's answer, before and after
        for (stranded, strand), (got, totals) in per_read_before.items():
            depth, want = C.depth_of(rs, F.LENGTH, 0, stranded, strand)
            runs = C.runs_of(depth)
            assert C.same_runs(got, runs) and totals == [runs[0].shape[0]] + want
            again, again_totals = _got(dr, F.LENGTH, stranded, strand, fragments=False)
            assert C.same_runs(again, got) and again_totals == totals
        assert dr.layout_bytes()[1] == 0          # (the set stays fused)
    with _Set(ctx, [(rs, None)]) as dr:          # ... and on a set without keys, as before
        depth, want = C.depth_of(rs, F.LENGTH)
        got, totals = _got(dr, F.LENGTH, fragments=False)
        assert C.same_runs(got, C.runs_of(depth)) and totals[1:] == want


def test_per_read_depth_minus_fragment_depth_is_the_pairs_overlap(ctx, content):
    rs, keys, mate = content["rs"], content["keys"], content["mate"]
    overlap = np.zeros(F.LENGTH, np.int64)
    pos, off, cig = rs.pos.tolist(), rs.cig_off.tolist(), rs.cigar.tolist()
    for i, m in enumerate(mate):
        if m == M.NONE or m < i:
            continue
        masks = []
        for k in (i, m):
            mask = np.zeros(F.LENGTH, bool)
            for a, b in C.covered_stretches(pos[k], cig[off[k]:off[k + 1]]):
                mask[max(a, 0):min(b, F.LENGTH)] = True
            masks.append(mask)
        overlap += masks[0] & masks[1]
    assert overlap.sum() > 0 and content["seen"]["mates overlapping partly"] >= 1
    with _Set(ctx, [(rs, keys)]) as dr:
        per_read = C.expand(*_got(dr, F.LENGTH, fragments=False)[0], F.LENGTH)
        per_fragment = C.expand(*_got(dr, F.LENGTH)[0], F.LENGTH)
    assert np.array_equal(per_read - per_fragment, overlap)


@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, TILE - 1, TILE, TILE + 1])
def test_sizes_around_a_wave_and_a_tile(ctx, content, n):
    """A slice of the content: mates fall off its ends and their reads cover alone."""
    rs, keys = content["rs"].take(700, 700 + n), content["keys"][700:700 + n]
    with _Set(ctx, [(rs, keys)]) as dr:
        for stranded, strand in TRACKS[:2]:
            _check(dr, rs, keys, F.LENGTH, 0, stranded, strand)


@pytest.mark.parametrize("shift,length", [(5000000, 5000000 + F.LENGTH), (-1000, F.LENGTH)])
def test_a_set_added_with_a_shift(ctx, content, shift, length):
    rs, keys, mate = content["rs"], content["keys"], content["mate"]
    with _Set(ctx, [(rs, keys)], [shift]) as dr:
        for stranded, strand in TRACKS[:2]:
            runs, totals = _check(dr, rs, keys, length, shift, stranded, strand, mate)
        assert totals[3] >= 1
        wanted = F.junction_tables(rs, mate, 1, F.KNOBS[1], shift)[0]
        if shift > 0:
            assert J.rows(dr.junctions(1, *F.KNOBS[1], fragments=True)) == F.table_rows(wanted) and len(wanted) > 20


def test_a_permuted_set_gives_the_same_runs_and_the_same_junction_table(ctx, content):
    """Leaders lie right of their mates as often as left.  (Of the content, the reads whose names name one first and one second read
    at most: who pairs with whom in a larger group is a matter of the order.)"""
    rs, keys = content["rs"], content["keys"]
    n_ops = np.diff(rs.cig_off.astype(np.int64))
    groups = {}
    for i in range(rs.n):
        if M.pairable(int(rs.flag[i]), int(rs.pos[i]), int(n_ops[i]), int(keys[i])):
            groups.setdefault((int(keys[i]) >> 1, int(rs.flag[i]) & 0x80), []).append(i)
    drop = {i for members in groups.values() if len(members) > 1 for i in members}
    keep = np.array([i for i in range(rs.n) if i not in drop])
    srs, skeys = F.permuted(rs, keys, keep)
    prs, pkeys = F.permuted(srs, skeys, np.random.default_rng(5).permutation(srs.n))
    pmate = M.mate_table_of(prs, pkeys)[0]
    assert sum(1 for i, m in enumerate(pmate) if m != M.NONE and m > i and prs.pos[m] < prs.pos[i]) > 100
    with _Set(ctx, [(srs, skeys)]) as a, _Set(ctx, [(prs, pkeys)]) as b:
        for stranded, strand in TRACKS[:3]:
            runs, totals = _check(a, srs, skeys, F.LENGTH, 0, stranded, strand)
            assert _check(b, prs, pkeys, F.LENGTH, 0, stranded, strand, pmate)[1] == totals and totals[5] > 50
        for stranded, knobs in MODES[:6]:
            table = J.rows(a.junctions(stranded, *knobs, fragments=True))
            want = F.junction_tables(srs, M.mate_table_of(srs, skeys)[0], stranded, knobs)[0]
            # counts and keys do not depend on the order; the anchors are the inserted reads', which does: they are the yardstick's of each order
            assert table == F.table_rows(want)
            permuted = J.rows(b.junctions(stranded, *knobs, fragments=True))
            assert permuted == F.table_rows(F.junction_tables(prs, pmate, stranded, knobs)[0]) and [r[:4] for r in permuted] == [r[:4] for r in table]


def test_a_segment_that_does_not_begin_the_arrays_and_two_segments(ctx, content):
    """The mate table is the segment's own, its indexes relative to the segment's first read: pairs do not cross segments."""
    rs, keys = content["rs"], content["keys"]
    cut = 1111
    parts = [(rs.take(0, cut), keys[:cut]), (rs.take(cut, rs.n), keys[cut:])]
    mates = [M.mate_table_of(p, k)[0] for p, k in parts]
    depth = np.zeros(F.LENGTH, np.int64)
    totals = [0] * 5
    for (p, k), mate in zip(parts, mates):
        t = F.fragment_depth(p, mate, F.LENGTH, depth=depth)[1]
        totals = [x + y for x, y in zip(totals, t)]
    assert totals[4] < content["counts"]["paired"] // 2          # a pair cut by the border is two single reads
    runs = C.runs_of(depth)
    tables = [F.junction_tables(p, mate, 1, (0, 0, 0)) for (p, k), mate in zip(parts, mates)]
    merged = {}
    for frag, _, _ in tables:
        for key, row in frag.items():
            have = merged.setdefault(key, [0, 0, 0])
            merged[key] = [have[0] + row[0], max(have[1], row[1]), max(have[2], row[2])]
    with _Set(ctx, parts) as dr:
        got, got_totals = _got(dr, F.LENGTH)
        assert C.same_runs(got, runs) and got_totals == [runs[0].shape[0]] + totals
        assert [dr.mate_table(k)[1]["paired"] for k in (0, 1)] == [sum(1 for m in mate if m != M.NONE) for mate in mates]
        assert J.rows(dr.junctions(1, 0, 0, 0, fragments=True)) == F.table_rows(merged)
    with _Set(ctx, parts, only=[1]) as dr:          # the second segment alone: it begins at read `cut` of the arrays
        _check(dr, parts[1][0], parts[1][1], F.LENGTH, mate=mates[1])
        assert J.rows(dr.junctions(1, 0, 0, 0, fragments=True)) == F.table_rows(tables[1][0])


# ---- coverage: hand cases ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spread", [0, 70, 300])
def test_hand_cases_with_the_mates_adjacent_in_other_waves_and_in_other_workgroups(ctx, spread):
    names = sorted(F.HAND_CASES)
    for group in [names] + [[n] for n in names[:3]]:
        records, keys, where = F.hand_set(group, spread)
        rs = samio.ReadSet.from_records(records)
        mate = M.mate_table_of(rs, keys)[0]
        assert all(mate[w] == w + spread + 1 for w in where)
        depth = np.zeros(F.HAND_LENGTH, np.int64)
        for n in group:          # read off the rule by hand
            for s, e in F.HAND_CASES[n][2]:
                depth[s:e] += 1
        with _Set(ctx, [(rs, keys)]) as dr:
            runs, totals = _check(dr, rs, keys, F.HAND_LENGTH, mate=mate)
            assert C.same_runs(runs, C.runs_of(depth)) and totals[5] == len(group) and totals[2] == len(group)
            if len(group) > 1:
                for stranded, strand in TRACKS[1:3]:
                    _check(dr, rs, keys, F.HAND_LENGTH, 0, stranded, strand, mate)


@pytest.mark.parametrize("lead_at", [0, 63])
def test_70_blocks_on_each_mate_with_the_leader_at_lane_0_and_lane_63(ctx, lead_at):
    one = F.HAND_CASES["mates overlapping partly"][:2]
    records, keys = [F.FILLER] * (lead_at % 2), [0] * (lead_at % 2)
    for k in range(40):
        records += list(F.HAND_CASES["70 blocks each, interleaved"][:2] if len(records) == lead_at else one)
        keys += [2 * k + 2] * 2
    rs = samio.ReadSet.from_records(records)
    with _Set(ctx, [(rs, keys)]) as dr:
        runs, totals = _check(dr, rs, keys, F.HAND_LENGTH)
    assert totals[5] == 40 and totals[0] >= 2 * F.MANY + 1


def test_mates_further_apart_than_a_launch_has_lanes(ctx):
    """LARGE one-op reads of two bases, every workgroup on its second grid-stride step, and a few pairs planted whose mates overlap in
    a base: first and last read, across GRID_MAX * TILE and a little, and neighbours at the end.  (The yardstick takes the planted
    pairs; the unpaired reads' depth, which is per read, is a histogram.)"""
    rng = np.random.default_rng(7)
    length = 50000
    pos = np.sort(rng.integers(1, length - 10, LARGE)).astype(np.int64)
    flag, keys = np.zeros(LARGE, np.uint16), np.zeros(LARGE, np.uint64)
    planted = [(0, LARGE - 1), (5, GRID_MAX * TILE + 6), (300, GRID_MAX * TILE + 500), (LARGE - 3, LARGE - 2), (TILE + 1, TILE)]
    for k, (a, b) in enumerate(planted):
        flag[a], flag[b] = 99, 147
        keys[a] = keys[b] = 2 * k + 2
        pos[b] = pos[a] + 1
    rs = samio.ReadSet(pos, flag, np.arange(LARGE + 1), np.full(LARGE, (2 << 4), np.uint32))
    in_pair = np.zeros(LARGE, bool)
    in_pair[[i for p in planted for i in p]] = True
    depth = np.bincount(pos[~in_pair] - 1, minlength=length) + np.bincount(pos[~in_pair], minlength=length)[:length]
    small = samio.ReadSet.from_records([(int(flag[i]), int(pos[i]), "2M") for p in planted for i in p])
    small_mate = [1, 0, 3, 2, 5, 4, 7, 6, 9, 8]
    _, t, _ = F.fragment_depth(small, small_mate, length, depth=depth)
    assert t[1:] == [5, 0, 15, 5]
    with _Set(ctx, [(rs, keys)]) as dr:
        mate = dr.mate_table(0, LARGE)[0]
        assert all(mate[a] == b and mate[b] == a for a, b in planted) and int((mate != M.NONE).sum()) == 10
        got, totals = _got(dr, length)
        runs = C.runs_of(depth)
        assert C.same_runs(got, runs) and totals == [runs[0].shape[0], LARGE, LARGE - 5, 0, 2 * LARGE - 5, 5]


def test_length_edges(ctx):
    rs = samio.ReadSet.from_records([(99, 91, "10M"), (147, 96, "5M"), (99, 151, "10M"), (147, 301, "10M")])
    keys = [2, 2, 4, 4]
    with _Set(ctx, [(rs, keys)]) as dr:
        got, totals = _got(dr, 100)          # a union ending exactly at length; a mate wholly past it
        assert [a.tolist() for a in got] == [[90], [100], [1]] and totals == [1, 4, 1, 1, 10, 2]
        _check(dr, rs, keys, 100)
        got, totals = _got(dr, 1)
        assert got[0].shape[0] == 0 and totals == [0, 4, 0, 2, 0, 2]
    rs = samio.ReadSet.from_records([(99, 1, "10M"), (147, 1, "5M")])
    with _Set(ctx, [(rs, [2, 2])]) as dr:
        got, totals = _got(dr, 1)          # length 1
        assert [a.tolist() for a in got] == [[0], [1], [1]] and totals == [1, 2, 1, 1, 1, 1]


def test_a_hot_locus_of_100000_identical_pairs(ctx):
    n = 100000
    flag = np.tile(np.array([99, 147], np.uint16), n)
    pos = np.tile(np.array([1001, 1031], np.int64), n)
    keys = np.repeat(np.arange(1, n + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15) & np.uint64(0xFFFFFFFFFFFFFFFE), 2)
    rs = samio.ReadSet(pos, flag, np.arange(2 * n + 1), np.full(2 * n, (50 << 4), np.uint32))
    with _Set(ctx, [(rs, keys)]) as dr:
        got, totals = _got(dr, 5000)
        assert [a.tolist() for a in got] == [[1000], [1080], [n]] and totals == [1, 2 * n, n, 0, 80 * n, n]
        got, totals = _got(dr, 5000, fragments=False)
        assert [a.tolist() for a in got] == [[1000, 1030, 1050], [1030, 1050, 1080], [n, 2 * n, n]] and totals == [3, 2 * n, 2 * n, 0, 100 * n]


# ---- the junction table ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stranded,knobs", MODES)
def test_the_junction_table_against_the_yardstick(ctx, content, stranded, knobs):
    rs, keys, mate, xs = content["rs"], content["keys"], content["mate"], content["xs"]
    want_frag, want_read, _ = F.junction_tables(rs, mate, stranded, knobs, xs=xs if stranded == 3 else None)
    assert len(want_frag) > 20 and set(want_frag) == set(want_read)
    with _Set(ctx, [(rs, keys)], xs=xs if stranded == 3 else None) as dr:
        before = J.rows(dr.junctions(stranded, *knobs))
        assert before == F.table_rows(want_read)
        assert J.rows(dr.junctions(stranded, *knobs, fragments=True)) == F.table_rows(want_frag)
        assert J.rows(dr.junctions(stranded, *knobs)) == before          # the per-read table is unchanged after the fragment call
        assert J.rows(dr.junctions(stranded, *knobs, fragments=True)) == F.table_rows(want_frag)          # ... and the reverse
    if stranded != 3:
        assert sum(r[0] for r in want_frag.values()) < sum(r[0] for r in want_read.values())


@pytest.mark.parametrize("n", [63, 64, 65, JTILE - 1, JTILE, JTILE + 1])
def test_junction_sizes_around_a_wave_and_a_tile(ctx, content, n):
    full = content["rs"]
    rs, keys = full.take(full.n - 15 - n, full.n - 15), content["keys"][full.n - 15 - n:full.n - 15]          # (the planted spliced pairs lie here)
    mate = M.mate_table_of(rs, keys)[0]
    with _Set(ctx, [(rs, keys)]) as dr:
        for stranded, knobs in ((0, F.KNOBS[0]), (1, F.KNOBS[1])):
            assert J.rows(dr.junctions(stranded, *knobs, fragments=True)) == F.table_rows(F.junction_tables(rs, mate, stranded, knobs)[0])


def test_64_lanes_of_one_key_half_of_them_duplicate_carries(ctx):
    """A wave whose 64 lanes all hold one junction: 32 pairs, mates neighbours, the later one of each a duplicate carry with the
    larger anchors.  Then the same with the mates 70 apart."""
    for spread in (0, 70):
        records, keys = [], []
        for k in range(32):
            records += [(99, 1001 - k, "%dM100N30M" % (30 + k))] + [F.FILLER] * spread + [(147, 1001 - 40, "70M100N%dM" % (40 + k))]
            keys += [2 * k + 2] + [0] * spread + [2 * k + 2]
        rs = samio.ReadSet.from_records(records)
        mate = M.mate_table_of(rs, keys)[0]
        want = F.junction_tables(rs, mate, 0, (0, 0, 0))
        assert F.table_rows(want[0]) == [(1030, 1130, 63, 32, 61, 30)] and F.table_rows(want[1]) == [(1030, 1130, 63, 64, 70, 71)]
        with _Set(ctx, [(rs, keys)]) as dr:
            assert J.rows(dr.junctions(0, 0, 0, 0, fragments=True)) == F.table_rows(want[0])
            assert J.rows(dr.junctions(0, 0, 0, 0)) == F.table_rows(want[1])


def test_a_read_of_more_ops_than_the_stage_holds_with_an_earlier_mate(ctx):
    long_cigar = "1M1I" * (JSTAGE // 2 + 30) + "20M100N30M"
    lead = JSTAGE // 2 + 30
    records = [(99, 1001, "%dM100N20M" % (lead + 20)), (147, 1001, long_cigar), (99, 5001, long_cigar), (147, 5001 + lead, "20M100N30M"), (0, 9001, "10M80N10M")]
    keys = [2, 2, 4, 4, 0]
    rs = samio.ReadSet.from_records(records)
    mate = M.mate_table_of(rs, keys)[0]
    assert mate[:4] == [1, 0, 3, 2] and int(np.diff(rs.cig_off.astype(np.int64)).max()) > JSTAGE
    for knobs in F.KNOBS:
        want = F.junction_tables(rs, mate, 0, knobs)
        assert [r[3] for r in F.table_rows(want[0])] == [1, 1, 1] and [r[3] for r in F.table_rows(want[1])] == [2, 2, 1]
        with _Set(ctx, [(rs, keys)]) as dr:
            assert J.rows(dr.junctions(0, *knobs, fragments=True)) == F.table_rows(want[0])
            assert J.rows(dr.junctions(0, *knobs)) == F.table_rows(want[1])


# ---- intron depth ---------------------------------------------------------------------------------------------------------------
def _tables(introns):
    off = np.concatenate(([0], np.cumsum([len(p) for p in introns]))).astype(np.int64)
    flat = [piece for p in introns for piece in p]
    return off, np.array([s for s, _ in flat], np.int32), np.array([e for _, e in flat], np.int32)


@pytest.mark.parametrize("stranded", [0, 1, 2])
def test_intron_depth_fragments_is_the_host_rule_over_the_yardsticks_fragment_depth(ctx, content, stranded):
    rs, keys, mate = content["rs"], content["keys"], content["mate"]
    features = G.random_features(np.random.default_rng(20261021), F.LENGTH - 700, 9, 30)
    length = F.LENGTH - 900
    with _Set(ctx, [(rs, keys)]) as dr:
        for track in (".",) if not stranded else ("+", "-"):
            introns = [x[3] for x in I.introns_of(features, track, length)]
            strand = 0 if not stranded else track
            depth = F.fragment_depth(rs, mate, length, 0, stranded, strand)[0]
            start, end, value = C.runs_of(depth)
            pos, dep = [], []
            for s, e, d in zip(start.tolist(), end.tolist(), value.tolist()):
                if pos and pos[-1] == s:
                    pos.pop(), dep.pop()
                pos += [s, e]
                dep += [d, 0]
            if pos and pos[-1] >= length:
                pos.pop(), dep.pop()
            for trim in (0, 30):
                got = dr.intron_depth(length, *_tables(introns), trim_percent=trim, stranded=stranded, strand=strand, fragments=True)
                want = [native.intron_depth_host(pos, dep, [s for s, _ in p], [e for _, e in p], trim) for p in introns]
                assert got.tolist() == want and [tuple(w) for w in want] == [I.stats_of(depth, p, trim) for p in introns]
                per_read = dr.intron_depth(length, *_tables(introns), trim_percent=trim, stranded=stranded, strand=strand)
                assert (per_read[:, 3] >= got[:, 3]).all()
            assert int(got[:, 1].sum()) > 0 and int(per_read[:, 3].sum()) > int(got[:, 3].sum())


# ---- refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_working(ctx, content):
    rs, keys, mate = content["rs"], content["keys"], content["mate"]
    pieces = _tables([[(0, 10), (20, 30)]])

    def every_call(dr, match):
        for call in (lambda: dr.coverage(F.LENGTH, fragments=True), lambda: dr.junctions(0, 0, 0, 0, fragments=True), lambda: dr.intron_depth(F.LENGTH, *pieces, fragments=True)):
            with pytest.raises(native.SpliserNativeError, match=match) as err:
                call()
            assert err.value.code == -1

    def works():
        with _Set(ctx, [(rs, keys)]) as dr:
            _check(dr, rs, keys, F.LENGTH, mate=mate)

    dr = ctx.upload_reads(native.ReadArrays(rs.pos, rs.flag, rs.cig_off, rs.cigar))          # (packed on the host: records, not arrays)
    try:
        every_call(dr, "fused")
    finally:
        dr.free()
    works()
    with _Set(ctx, [(rs, None)]) as dr:          # a set without keys
        every_call(dr, "name keys")
        assert C.same_runs(_got(dr, F.LENGTH, fragments=False)[0], C.runs_of(C.depth_of(rs, F.LENGTH)[0]))
    works()
    with ctx.upload_soa([native.ReadArrays(rs.pos, rs.flag, rs.cig_off, rs.cigar, name_key=keys)], with_keys=True) as soa:
        with ctx.begin_reads() as dr:
            dr.add_soa(soa, 0)
            every_call(dr, "not finished")
            dr.finish()
            for kw, match in ((dict(stranded=3), "stranded"), (dict(stranded=0, strand="+"), "strand must be"), (dict(stranded=1, strand=0), "strand must be")):
                with pytest.raises(native.SpliserNativeError, match=match) as err:
                    dr.coverage(F.LENGTH, fragments=True, **kw)
                assert err.value.code == -1
                with pytest.raises(native.SpliserNativeError, match=match):
                    dr.intron_depth(F.LENGTH, *pieces, fragments=True, **kw)
            for bad_length in (0, 2 ** 31 - 1):
                with pytest.raises(native.SpliserNativeError, match="length") as err:
                    dr.coverage(bad_length, fragments=True)
                assert err.value.code == -1
            with pytest.raises(native.SpliserNativeError, match="stranded"):
                dr.junctions(4, 0, 0, 0, fragments=True)
            with pytest.raises(native.SpliserNativeError, match="strand bytes"):
                dr.junctions(3, 0, 0, 0, fragments=True)
            _check(dr, rs, keys, F.LENGTH, mate=mate)          # the next call on the same set works
    with ctx.begin_reads() as dr:          # a set without a read: nothing, not an error
        dr.finish()
        got, totals = _got(dr, 100)
        assert got[0].shape[0] == 0 and totals == [0] * 6 and dr.junctions(0, 0, 0, 0, fragments=True)["left"].shape[0] == 0
    works()


# ---- the decodes and the commands -------------------------------------------------------------------------------------------------
NAMES, LENGTHS = ["c1", "c2", "c3"], [9000, 8070, 10 ** 6]
IDS = ["gene%02d" % k for k in range(8)]
SPAN = 8000
PER_CHROM = 100000


def _paired_chromosome(rng, k, n):
    """About n reads of one chromosome, made with numpy: pairs of every flag kind whose mates overlap, abut, lie apart or cross the same
    intron, single reads, a secondary copy now and then.  -> (ReadSet sorted by POS, names, MAPQs)."""
    n_pairs = n // 2 - 50
    lead = rng.integers(1, SPAN - 400, n_pairs)
    gap = rng.choice(np.array([0, 10, 30, 50, 80, 120]), n_pairs)
    kind = rng.integers(0, 10, n_pairs)
    cigars = ["50M", "20M100N30M", "30M100N20M", "25M5D25M"]
    rows = []
    flags = M.PAIR_FLAGS
    for j in range(n_pairs):
        f = flags[j % 3]
        name = b"p%d:%d" % (k, j)
        if kind[j] < 6:
            rows.append((f[0], int(lead[j]), "50M", name, 60))
            rows.append((f[1], int(lead[j] + gap[j]), "50M", name, 60))
        elif kind[j] < 8:          # both mates across the intron that begins 20 + lead .. : the same junction
            rows.append((f[0], int(lead[j]), "20M100N30M", name, 60))
            rows.append((f[1], int(lead[j] + 10), "10M100N40M", name, 60))
        elif kind[j] == 8:
            rows.append((f[0], int(lead[j]), cigars[j % 4], name, 60))
            rows.append((f[1], int(lead[j] + gap[j]), cigars[(j // 4) % 4], name, 60))
        else:
            rows.append((f[0], int(lead[j]), "50M", name, 60))
            rows.append((f[1], int(lead[j] + 20), "50M", name, 60))
            rows.append((f[1] | 256, int(lead[j] + 25), "50M", name, 60))
    for j in range(100):
        rows.append(((73, 137, 0, 16)[j % 4], int(rng.integers(1, SPAN)), "50M", b"s%d:%d" % (k, j), 60))
    rows += [(99, SPAN + 45, "20M", b"lowq%d" % k, 60), ((99, 147)[k % 2], SPAN + 50, "30M", b"split/pair", 60), (147, SPAN + 60, "30M", b"lowq%d" % k, 3)]
    rows.sort(key=lambda r: r[1])
    return samio.ReadSet.from_records([r[:3] for r in rows]), [r[3] for r in rows], np.array([r[4] for r in rows], np.int64)


@pytest.fixture(scope="module")
def paired_files(tmp_path_factory):
    """Three chromosomes of about 100 000 paired reads each with names and MAPQs (c2's LN cuts its reads), one pair split over two of
    them, one pair a chromosome whose second mate has MAPQ 3; genes on c1 and c2.  The one content as BAM, the BAM shuffled, SAM text
    and BGZF SAM text."""
    d = tmp_path_factory.mktemp("cfdec")
    rng = np.random.default_rng(47)
    sets, names, mapq, features = [], [], [], {}
    for k, chrom in enumerate(NAMES):
        rs, nm, q = _paired_chromosome(rng, k, PER_CHROM)
        sets.append((chrom, rs))
        names.append(nm)
        mapq.append(q)
        if k < 2:
            features[chrom] = [(l, r, s, g) for l, r, s, g in G.random_features(rng, SPAN - 1000, 8, 30)]
    bam, shuffled, sam, samz, gtf = str(d / "p.bam"), str(d / "s.bam"), str(d / "p.sam"), str(d / "p.sam.gz"), str(d / "genes.gtf")
    samio.write_bam(bam, NAMES, LENGTHS, sets, with_seq=False, unplaced=3, names=names, mapq=mapq)
    samio.write_sam(sam, NAMES, LENGTHS, sets, names=names, mapq=mapq)
    records, flat_names = [], []
    for tid, ((chrom, rs), nm, q) in enumerate(zip(sets, names, mapq)):
        off = rs.cig_off.tolist()
        for j in range(rs.n):
            records.append((tid, int(rs.pos[j]) - 1, int(rs.flag[j]), int(q[j]), rs.cigar[off[j]:off[j + 1]], nm[j]))
    order = rng.permutation(len(records))
    _write_named_bam(shuffled, [records[j] for j in order])
    with open(sam, "rb") as fh, open(samz, "wb") as out:
        out.write(Z.bgzf(fh.read(), block=0xff00))
    text = "##gtf of the tests\n"
    for chrom in NAMES[:2]:
        for j, (left, right, strand, gene) in enumerate(features[chrom]):
            text += "%s\tsynth\texon\t%d\t%d\t.\t%s\t.\tgene_id \"%s\"; transcript_id \"t%d\";\n" % (chrom, left + 1, right, strand, IDS[gene], j)
    open(gtf, "w").write(text)
    ids, by_chrom = G.features_of_text(text)
    keys = [np.array([M.name_key(n) for n in nm], np.uint64) for nm in names]
    return dict(dir=str(d), bam=bam, shuffled=shuffled, sam=sam, samz=samz, gtf=gtf, sets=sets, keys=keys, mapq=mapq, ids=ids, by_chrom=by_chrom, kept={})


def _write_named_bam(path, records):
    """An unsorted BAM of (tid, 0-based pos, flag, mapq, ops, name) records, in the order given."""
    import struct
    body = bytearray(b"BAM\x01")
    text = "@HD\tVN:1.6\tSO:unsorted\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % (n, ln) for n, ln in zip(NAMES, LENGTHS))
    body += struct.pack("<i", len(text)) + text.encode() + struct.pack("<i", len(NAMES))
    for n, ln in zip(NAMES, LENGTHS):
        body += struct.pack("<i", len(n) + 1) + n.encode() + b"\0" + struct.pack("<i", ln)
    parts = [bytes(body)]
    for tid, pos, flag, mapq, ops, name in records:
        ops = np.asarray(ops, "<u4")
        rec = struct.pack("<iiBBHHHiiii", tid, pos, len(name) + 1, mapq, 4680, ops.shape[0], flag, 0, -1, -1, 0) + name + b"\0" + ops.tobytes()
        parts.append(struct.pack("<i", len(rec)) + rec)
    with open(path, "wb") as out:
        out.write(Z.bgzf(b"".join(parts), block=0xff00))


def _kept(f, min_mapq=0):
    """Per chromosome the reads the decode keeps under ``min_mapq``, their keys and the yardstick's mate table (made once)."""
    if min_mapq not in f["kept"]:
        out = []
        for (chrom, rs), keys, q in zip(f["sets"], f["keys"], f["mapq"]):
            keep = np.flatnonzero(q >= min_mapq)
            krs, kkeys = F.permuted(rs, keys, keep)
            out.append((chrom, krs, kkeys, M.mate_table_of(krs, kkeys)[0]))
        f["kept"][min_mapq] = out
    return f["kept"][min_mapq]


def _depth(f, k, stranded, strand, fragments=True, min_mapq=0):
    """The yardstick's depth of chromosome k on one track, and the pairs whose union was taken (made once)."""
    key = ("depth", k, stranded, strand, fragments, min_mapq)
    if key not in f["kept"]:
        chrom, rs, keys, mate = _kept(f, min_mapq)[k]
        if fragments:
            depth, totals, _ = F.fragment_depth(rs, mate, LENGTHS[k], 0, stranded, strand)
            f["kept"][key] = (depth, totals[4])
        else:
            f["kept"][key] = (C.depth_of(rs, LENGTHS[k], 0, stranded, strand)[0], 0)
    return f["kept"][key]


def _bedgraphs(f, stranded=0, fragments=True, min_mapq=0, only=None):
    """The yardstick's bedGraph text per track, and the pairs whose union was taken per track."""
    texts, pairs = [], []
    for strand in (("+", "-") if stranded else (0,)):
        text, taken = "", 0
        for k, chrom in enumerate(NAMES):
            if only is not None and chrom != only:
                continue
            depth, n = _depth(f, k, stranded, strand, fragments, min_mapq)
            taken += n
            text += C.bedgraph_text(chrom, *C.runs_of(depth))
        texts.append(text)
        pairs.append(taken)
    return texts, pairs


FIVE = [("bam", lambda f: ["-B", f["bam"]]), ("host", lambda f: ["-B", f["bam"], "--hostDecode"]), ("sam", lambda f: ["-B", f["sam"]]), ("samz", lambda f: ["-B", f["samz"]]),
        ("shuffled", lambda f: ["-B", f["shuffled"], "--anyOrder"])]


def _read(prefix, stranded):
    return [open(prefix + s).read() for s in ((".plus.bedgraph", ".minus.bedgraph") if stranded else (".bedgraph",))]


@pytest.mark.parametrize("stranded", [0, 1])
def test_coverage_fragments_writes_the_same_bytes_for_five_inputs(paired_files, capsys, stranded):
    f, d = paired_files, paired_files["dir"]
    want, pairs = _bedgraphs(f, stranded)
    assert all(want) and min(pairs) > 10000 and want != _bedgraphs(f, stranded, fragments=False)[0]
    extra = ["--isStranded", "-s", "fr"] if stranded else []
    for tag, args in FIVE:
        prefix = "%s/cov_%s_%d" % (d, tag, stranded)
        assert cli.main(["coverage", "-o", prefix, "--fragments"] + args(f) + extra) == 0
        log = capsys.readouterr().out
        assert _read(prefix, stranded) == want, tag
        assert "pairable reads" in log and "pairs found" in log and "union was taken" in log and all("  %s: " % c in log for c in NAMES)
        assert all(str(p) in log for p in pairs) and "Mates: " in log


def test_coverage_fragments_of_one_chromosome_and_with_min_mapq(paired_files, capsys):
    f, d = paired_files, paired_files["dir"]
    assert cli.main(["coverage", "-o", d + "/cov_c2", "--fragments", "-B", f["bam"], "-c", "c2"]) == 0
    assert _read(d + "/cov_c2", 0) == _bedgraphs(f, only="c2")[0]
    want, pairs = _bedgraphs(f, min_mapq=10)          # --minMapQ turns the low-quality pair of every chromosome into two single reads
    all_want, all_pairs = _bedgraphs(f)
    assert pairs[0] == all_pairs[0] - len(NAMES) and want != all_want
    for tag, args in FIVE[:3:2]:
        assert cli.main(["coverage", "-o", "%s/cov_q_%s" % (d, tag), "--fragments", "--minMapQ", "10"] + args(f)) == 0
        assert _read("%s/cov_q_%s" % (d, tag), 0) == want, tag
    capsys.readouterr()


def _introns_text(f, stranded=0, fragments=True):
    depths, junctions = {}, {}
    for k, (chrom, rs, keys, mate) in enumerate(_kept(f)):
        for track in I.tracks_of(stranded):
            depths[(chrom, track)] = _depth(f, k, stranded, 0 if not stranded else track, fragments)[0]
        if fragments:
            table = F.junction_tables(rs, mate, stranded, (0, 0, 0))[0]
            junctions[chrom] = sorted((l, r, chr(s), row[0]) for (l, r, s), row in table.items())
        else:
            junctions[chrom] = I.junction_rows(rs, stranded)
    return I.file_text(I.rows_of(f["ids"], list(f["by_chrom"]), f["by_chrom"], stranded, 30, dict(zip(NAMES, LENGTHS)), depths, junctions, None))


@pytest.mark.parametrize("stranded", [0, 1])
def test_intronretention_fragments_writes_the_yardsticks_rows_for_five_inputs(paired_files, capsys, stranded):
    f, d = paired_files, paired_files["dir"]
    want = _introns_text(f, stranded)
    assert want != _introns_text(f, stranded, fragments=False) and want.count("\n") > 10
    extra = ["--isStranded", "-s", "fr"] if stranded else []
    for tag, args in FIVE:
        prefix = "%s/ir_%s_%d" % (d, tag, stranded)
        assert cli.main(["intronretention", "-A", f["gtf"], "-o", prefix, "--fragments"] + args(f) + extra) == 0
        log = capsys.readouterr().out
        assert open(prefix + ".introns.tsv").read() == want, tag
        assert "per fragment" in log and "pairs found" in log and "Mates: " in log


def test_without_the_switch_both_commands_write_what_they_wrote(paired_files, capsys):
    f, d = paired_files, paired_files["dir"]
    for stranded, extra in ((0, []), (1, ["--isStranded", "-s", "fr"])):
        want = _bedgraphs(f, stranded, fragments=False)[0]
        for tag, args in FIVE[:3]:
            prefix = "%s/plain_%s_%d" % (d, tag, stranded)
            assert cli.main(["coverage", "-o", prefix] + args(f) + extra) == 0
            assert _read(prefix, stranded) == want, tag
    log = capsys.readouterr().out
    assert "pairs" not in log and "fragments" not in log and "reads contributed" in log
    want = _introns_text(f, 0, fragments=False)
    for tag, args in FIVE[:3]:
        assert cli.main(["intronretention", "-A", f["gtf"], "-o", "%s/plainir_%s" % (d, tag)] + args(f)) == 0
        assert open("%s/plainir_%s.introns.tsv" % (d, tag)).read() == want, tag
    log = capsys.readouterr().out
    assert "pairs" not in log and "per fragment" not in log
