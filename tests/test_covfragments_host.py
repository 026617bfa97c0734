"""``coverage --fragments`` and ``intronretention --fragments`` on the host: the coverage fragment rule
(``spl_coverage_fragment_rule_host``, the kernel's own header compiled for the host) against the yardstick of ``covfragcases.py`` on
generated paired content whose coverage is asserted and on the hand cases, unstranded and on both tracks of fr and rf; the rule's
block cursor against ``spl_cov_walk``, block for block; the junction fragment rule (``spl_junction_fragment_rule_host``) against the
yardstick's sets of keys, and the three identities that tie the fragment table to the per-read one; both headers in a stand-alone
program under AddressSanitizer and UBSan (tests/hostsim/covfragment_rule_asan.cpp); the command line.  No GPU."""
import os
import subprocess
import types

import numpy as np
import pytest

import covcases as C
import covfragcases as F
import junctioncases as J
import matecases as M
from spliser_amd import cli, coverage as cov, intronretention as ir, native, samio

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRACKS = [(0, 0), (1, "+"), (1, "-"), (2, "+"), (2, "-")]
MODES = [(s, k) for s in (0, 1, 2, 3) for k in F.KNOBS]


@pytest.fixture(scope="module")
def built():
    native.build()
    return native.lib()


@pytest.fixture(scope="module")
def content():
    """Generated paired content of every kind -- asserted --, its mate table by the yardstick, and strand bytes for mode 3."""
    rs, keys, names = F.paired_content(np.random.default_rng(20261022))
    seen = F.assert_covers(rs, keys)
    mate, counts = M.mate_table_of(rs, keys)
    xs = np.random.default_rng(3).choice(np.array([43, 45, 0], np.uint8), rs.n)
    return dict(rs=rs, keys=keys, mate=mate, counts=counts, seen=seen, xs=xs)


def _arrays(rs):
    return native.ReadArrays(rs.pos, rs.flag, rs.cig_off, rs.cigar)


def _hook(rs, mate, length, shift=0, stranded=0, strand=0, cap=1 << 16):
    return native.coverage_fragment_rule_host(_arrays(rs), np.asarray(mate, np.uint32), length, shift, stranded, strand, cap)


def _split(n_iv, intervals):
    out, at = [], 0
    for n in n_iv.tolist():
        out.append(intervals[at:at + n])
        at += n
    assert at == len(intervals)
    return out


def _same_as_yardstick(rs, mate, length, shift, stranded, strand):
    status, n_iv, past, intervals, totals = _hook(rs, mate, length, shift, stranded, strand)
    depth, want_totals, per_read = F.fragment_depth(rs, mate, length, shift, stranded, strand)
    assert status.tolist() == [p[0] for p in per_read]
    assert _split(n_iv, intervals) == [p[1] for p in per_read]
    assert past.tolist() == [p[2] for p in per_read]
    assert [totals[k] for k in native.COVERAGE_FRAGMENT_TOTALS[1:]] == want_totals and totals["runs"] == sum(len(p[1]) for p in per_read)
    # the intervals summed are the depth: covered bases == sum((end - start) * depth)
    got = np.zeros(length, np.int64)
    for s, e in intervals:
        got[s:e] += 1
    assert np.array_equal(got, depth) and int(depth.sum()) == totals["covered_bases"]
    return status, per_read, totals


# ---- coverage: the rule -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stranded,strand", TRACKS)
def test_the_hook_against_the_yardstick(built, content, stranded, strand):
    rs, mate = content["rs"], content["mate"]
    status, per_read, totals = _same_as_yardstick(rs, mate, F.LENGTH, 0, stranded, strand)
    assert {F.CONTRIBUTED, F.SILENT, F.NOT_PARTICIPATING} <= set(status.tolist()) and totals["pairs"] >= 10
    assert stranded or (totals["past_end"] >= 1 and totals["pairs"] > 100)
    silent = [i for i, s in enumerate(status.tolist()) if s == F.SILENT]
    assert len(silent) == totals["pairs"] and all(mate[i] != M.NONE and mate[i] < i for i in silent)
    if stranded == 0:
        assert totals["pairs"] == content["counts"]["paired"] // 2
    else:          # a pair with its mates on different tracks is no pair on either
        assert totals["pairs"] < content["counts"]["paired"] // 2 and content["seen"]["mates on different tracks under fr"] >= 1
    # every interval, also beyond cap; the list as far as cap reaches
    full = _hook(rs, mate, F.LENGTH, 0, stranded, strand)
    for cap in (0, 1, 7):
        part = _hook(rs, mate, F.LENGTH, 0, stranded, strand, cap=cap)
        assert part[0].tolist() == full[0].tolist() and part[1].tolist() == full[1].tolist() and part[3] == full[3][:cap] and part[4] == full[4]


@pytest.mark.parametrize("shift,length", [(5000000, 5000000 + F.LENGTH), (-1000, F.LENGTH), (0, 5000), (0, 1)])
def test_shifts_and_lengths(built, content, shift, length):
    for stranded, strand in TRACKS[:3]:
        _same_as_yardstick(content["rs"], content["mate"], length, shift, stranded, strand)


def test_fragment_depth_is_read_depth_minus_the_pairs_overlap(built, content):
    rs, mate = content["rs"], content["mate"]
    per_fragment = F.fragment_depth(rs, mate, F.LENGTH)[0]
    per_read = C.depth_of(rs, F.LENGTH)[0]
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
    assert np.array_equal(per_read - per_fragment, overlap)


def test_the_union_does_not_depend_on_the_order(built, content):
    """Which mate leads does; runs and the order-independent counters do not.  (Of the content, the reads whose names name one first
    and one second read at most: who pairs with whom in a larger group is a matter of the order.)"""
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
    for stranded, strand in TRACKS[:3]:
        a = _hook(srs, M.mate_table_of(srs, skeys)[0], F.LENGTH, 0, stranded, strand)
        b = _hook(prs, M.mate_table_of(prs, pkeys)[0], F.LENGTH, 0, stranded, strand)
        assert a[4] == b[4] and a[4]["pairs"] > 50

        def depth_of(intervals):
            d = np.zeros(F.LENGTH, np.int64)
            for s, e in intervals:
                d[s:e] += 1
            return d
        assert np.array_equal(depth_of(a[3]), depth_of(b[3]))


def test_a_set_without_a_pair_gives_the_per_read_blocks(built, content):
    rs = content["rs"]
    none = np.full(rs.n, M.NONE, np.uint32)
    off, cig = rs.cig_off.tolist(), rs.cigar
    for stranded, strand in TRACKS[:3]:
        status, n_iv, past, intervals, totals = _hook(rs, none, F.LENGTH, 0, stranded, strand)
        per_read = _split(n_iv, intervals)
        assert totals["pairs"] == 0 and F.SILENT not in status.tolist()
        for i in range(rs.n):
            blocks, lost = native.coverage_rule_host(int(rs.flag[i]), int(rs.pos[i]), cig[off[i]:off[i + 1]], F.LENGTH, 0, stranded, strand)
            assert per_read[i] == blocks and bool(past[i]) == lost
        want = C.depth_of(rs, F.LENGTH, 0, stranded, strand)[1]
        assert [totals[k] for k in native.COVERAGE_TOTALS[1:]] == want


def test_the_cursor_against_the_walk(built, content):
    """``spl_cov_cursor`` gives ``spl_cov_walk``'s blocks, block for block, on covcases' reads: the content's, and CIGARs of every op."""
    rs = content["rs"]
    off, cig = rs.cig_off.tolist(), rs.cigar
    cases = [(int(rs.flag[i]), int(rs.pos[i]), cig[off[i]:off[i + 1]]) for i in range(rs.n)]
    for text in ("10M2I5M", "10M0N5M", "5S10M5D0M10M3N2M4H", "3N10M", "10M3N", "0M", "5I", "10M5P5M", "2=3X4M", "1M1D1M1N1M1D1M", "100N", "5M100N5M100N5M"):
        for pos in (1, 40, 95):
            cases.append((0, pos, samio.ReadSet.from_records([(0, pos, text)]).cigar))
    n_blocks = 0
    for flag, pos, ops in cases:
        for length, shift in ((F.LENGTH, 0), (100, 0), (60, -50), (1, 0)):
            walk = native.coverage_rule_host(flag, pos, ops, length, shift)
            assert native.coverage_cursor_host(flag, pos, ops, length, shift) == walk
            assert walk == C.blocks_of(flag, pos, list(np.asarray(ops).tolist()), length, shift)
            n_blocks += len(walk[0])
    assert n_blocks > 1000


@pytest.mark.parametrize("spread", [0, 70, 300])
def test_the_hand_cases(built, spread):
    names = sorted(F.HAND_CASES)
    for group in [names] + [[n] for n in names]:
        records, keys, where = F.hand_set(group, spread)
        rs = samio.ReadSet.from_records(records)
        mate = M.mate_table_of(rs, keys)[0]
        assert all(mate[w] == w + spread + 1 for w in where)
        status, n_iv, past, intervals, totals = _hook(rs, mate, F.HAND_LENGTH)
        per_read = _split(n_iv, intervals)
        assert [per_read[w] for w in where] == [F.HAND_CASES[n][2] for n in group]          # read off the rule by hand
        assert all(status[w + spread + 1] == F.SILENT for w in where) and totals["pairs"] == len(group)
        _same_as_yardstick(rs, mate, F.HAND_LENGTH, 0, 0, 0)
    assert len(F.HAND_CASES["70 blocks each, interleaved"][2]) == 2 * F.MANY
    # 99 / 131 under fr: each mate alone on its own track
    records, keys, where = F.hand_set(["99 / 131: two tracks of a stranded run"], spread)
    rs = samio.ReadSet.from_records(records)
    mate = M.mate_table_of(rs, keys)[0]
    plus, minus = _hook(rs, mate, F.HAND_LENGTH, 0, 1, "+"), _hook(rs, mate, F.HAND_LENGTH, 0, 1, "-")
    assert plus[3] == [(1700, 1750)] and minus[3] == [(1720, 1770)] and plus[4]["pairs"] == minus[4]["pairs"] == 0
    assert F.SILENT not in plus[0].tolist() + minus[0].tolist()


def test_length_edges(built):
    rs = samio.ReadSet.from_records([(99, 91, "10M"), (147, 96, "5M"), (99, 151, "10M"), (147, 301, "10M")])
    mate = [1, 0, 3, 2]
    status, n_iv, past, intervals, totals = _hook(rs, mate, 100)          # a union ending exactly at length; a mate wholly past it
    assert intervals == [(90, 100)] and status.tolist() == [1, F.SILENT, F.NOTHING, F.SILENT] and past.tolist() == [False, False, True, False]
    assert totals == dict(runs=1, reads_seen=4, contributed=1, past_end=1, covered_bases=10, pairs=2)
    status, n_iv, past, intervals, totals = _hook(samio.ReadSet.from_records([(99, 1, "10M"), (147, 1, "5M")]), [1, 0], 1)
    assert intervals == [(0, 1)] and totals["covered_bases"] == 1 and totals["past_end"] == 1 and totals["pairs"] == 1


def test_mate_indexes_the_rule_does_not_believe(built):
    """At or beyond n, or the read itself: no partner."""
    rs = samio.ReadSet.from_records([(99, 101, "50M"), (147, 131, "50M")])
    for mate in ([2, 0], [0, 0], [0xFFFFFFF0, 0xFFFFFFFF], [7, 1]):
        status, n_iv, past, intervals, totals = _hook(rs, mate, 1000)
        if mate[1] == 0:
            assert status.tolist() == [1, F.SILENT] and intervals == [(100, 150)]
        else:
            assert status.tolist() == [1, 1] and intervals == [(100, 150), (130, 180)] and totals["pairs"] == 0


def test_hook_refusals(built):
    rs = samio.ReadSet.from_records([(99, 101, "50M"), (147, 131, "50M")])
    for kwargs, match in ((dict(length=0), "length"), (dict(length=100, stranded=1, strand=0), "strand"), (dict(length=100, stranded=3, strand="+"), "strand")):
        with pytest.raises(native.SpliserNativeError, match=match) as err:
            _hook(rs, [1, 0], **kwargs)
        assert err.value.code == -1
    with pytest.raises(ValueError):
        _hook(rs, [1], 100)


# ---- junctions: the rule ----------------------------------------------------------------------------------------------------------
def _jhook(rs, mate, stranded, knobs, shift=0, xs=None):
    counted, dup, rows = native.junction_fragment_rule_host(_arrays(rs), np.asarray(mate, np.uint32), stranded, *knobs, shift=shift, xs=xs if stranded == 3 else None)
    frag, read = {}, {}
    for l, r, st, al, ar, d in rows.tolist():
        for table in ([read] if d else [read, frag]):
            row = table.setdefault((l, r, st), [0, 0, 0])
            row[0], row[1], row[2] = row[0] + 1, max(row[1], al), max(row[2], ar)
    return counted.tolist(), dup.tolist(), frag, read, rows


@pytest.mark.parametrize("stranded,knobs", MODES)
def test_the_junction_hook_against_the_yardstick_and_the_three_identities(built, content, stranded, knobs):
    rs, mate, xs = content["rs"], content["mate"], content["xs"]
    counted, dup, frag, read, rows = _jhook(rs, mate, stranded, knobs, xs=xs)
    want_frag, want_read, per_read = F.junction_tables(rs, mate, stranded, knobs, xs=xs if stranded == 3 else None)
    assert F.table_rows(frag) == F.table_rows(want_frag) and F.table_rows(read) == F.table_rows(want_read)
    assert [(c, d) for c, d in zip(counted, dup)] == [p for p in per_read]
    # the three identities
    assert set(frag) == set(read) and len(frag) > 20
    duplicates = {}
    for l, r, st, al, ar, d in rows.tolist():
        if d:
            duplicates[(l, r, st)] = duplicates.get((l, r, st), 0) + 1
    assert all(frag[k][0] == read[k][0] - duplicates.get(k, 0) for k in read) and (sum(duplicates.values()) >= 1 or stranded == 3)
    assert all(frag[k][1] <= read[k][1] and frag[k][2] <= read[k][2] for k in read)
    # a duplicate carry only at a read whose mate lies in front of it
    assert all(d == 0 or (mate[i] != M.NONE and mate[i] < i) for i, d in enumerate(dup))
    if knobs == F.KNOBS[1] and stranded == 0:
        assert content["seen"]["the same intron with only one mate passing min_anchor"] >= 1
    # the per-read table is the walk's: spl_junction_walk_host's rule, by junctioncases
    if stranded != 3:
        assert F.table_rows(read) == F.table_rows(F.junction_tables(rs, [M.NONE] * rs.n, stranded, knobs)[0])


def test_junction_hand_cases(built):
    """Both mates across one intron: once.  Only one of them passing min_anchor: that one's.  Mates on two strands of fr: twice."""
    rs = samio.ReadSet.from_records([(99, 101, "30M100N30M"), (147, 111, "20M100N40M"), (99, 1001, "30M100N30M"), (147, 1026, "5M100N40M"),
                                     (65, 2001, "30M100N30M"), (129, 2011, "20M100N40M"), (0, 3001, "30M100N30M"), (0, 3001, "30M100N30M")])
    mate = [1, 0, 3, 2, 5, 4, M.NONE, M.NONE]
    counted, dup, frag, read, _ = _jhook(rs, mate, 0, (0, 0, 0))
    assert counted == [1, 0, 1, 0, 1, 0, 1, 1] and dup == [0, 1, 0, 1, 0, 1, 0, 0]
    assert F.table_rows(frag) == [(130, 230, 63, 1, 30, 30), (1030, 1130, 63, 1, 30, 30), (2030, 2130, 63, 1, 30, 30), (3030, 3130, 63, 2, 30, 30)]
    assert [row[3:] for row in F.table_rows(read)] == [(2, 30, 40)] * 3 + [(2, 30, 30)]
    counted, dup, frag, read, _ = _jhook(rs, mate, 0, F.KNOBS[1])          # the second pair's later mate has a left anchor of 5: it supports nothing
    assert counted == [1, 0, 1, 0, 1, 0, 1, 1] and dup == [0, 1, 0, 0, 0, 1, 0, 0]
    counted, dup, frag, read, _ = _jhook(rs, mate, 1, (0, 0, 0))          # 65 / 129: '+' and '-' under fr, two rows
    assert counted == [1, 0, 1, 0, 1, 1, 1, 1] and (2030, 2130, 43) in frag and (2030, 2130, 45) in frag
    for bad in ([2, 0] + mate[2:], [0, 1] + mate[2:], [0xFFFFFFF0, 8] + mate[2:]):          # no earlier mate: counted as before
        counted, dup, _, _, _ = _jhook(rs, bad, 0, (0, 0, 0))
        assert counted[:2] == ([1, 0] if bad[1] == 0 else [1, 1])


# ---- both headers under the sanitizers ---------------------------------------------------------------------------------------------
def test_headers_under_the_sanitizers(tmp_path, built, content):
    """The two rule headers alone in a program of its own: every array in a heap block of exactly its size; mate indexes at and
    beyond n, a read that is its own mate, CIGAR offsets that descend or point beyond the ops, and a mate without an op."""
    exe = str(tmp_path / "covfragment_asan")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "hostsim", "covfragment_rule_asan.cpp"), "-o", exe])
    text_of = lambda v: " ".join(str(int(x)) for x in v)
    rs, mate, xs = content["rs"], content["mate"], content["xs"]
    lines, want = [], []

    def cov_case(rs, mate, shift, length, stranded, strand, cap, expect=None):
        strand = ord(strand) if isinstance(strand, str) else strand
        lines.append("|".join(["C", "%d %d %d %d %d" % (shift, length, stranded, strand, cap), text_of(rs.pos), text_of(rs.flag), text_of(rs.cig_off), text_of(rs.cigar), text_of(mate)]))
        if expect is None:
            _, totals, per_read = F.fragment_depth(rs, mate, length, shift, stranded, strand)
            flat = [v for p in per_read for iv in p[1] for v in iv]
            expect = [[p[0] for p in per_read], [len(p[1]) for p in per_read], [int(p[2]) for p in per_read], flat[:2 * cap], [len(flat) // 2] + totals]
        want.extend(expect)

    def junction_case(rs, mate, shift, stranded, knobs, cap, xs=None, expect=None, symmetric=True):
        lines.append("|".join(["J", "%d %d %d %d %d %d" % ((shift, stranded) + tuple(knobs) + (cap,)), text_of(rs.pos), text_of(rs.flag), text_of(rs.cig_off), text_of(rs.cigar),
                               text_of(mate), text_of(xs) if stranded == 3 else ""]))
        if expect is None:
            counted, dup, rows = native.junction_fragment_rule_host(_arrays(rs), np.asarray(mate, np.uint32), stranded, *knobs, shift=shift, xs=xs if stranded == 3 else None, cap=cap)
            per_read = F.junction_tables(rs, mate, stranded, knobs, shift, xs if stranded == 3 else None)[2] if symmetric else list(zip(counted.tolist(), dup.tolist()))
            assert [(c, d) for c, d in zip(counted.tolist(), dup.tolist())] == per_read          # (the library's rows are the yardstick's: the test above)
            expect = [counted.tolist(), dup.tolist(), rows.reshape(-1).tolist()]
        want.extend(expect)

    for stranded, strand in TRACKS:
        for cap in (0, 5, 1 << 16):
            cov_case(rs, mate, 0, F.LENGTH, stranded, strand, cap)
    cov_case(rs, mate, -1000, 3000, 0, 0, 1 << 16)
    cov_case(rs, mate, 2147480000, 2147483646, 0, 0, 1 << 16)
    records, keys, where = F.hand_set(sorted(F.HAND_CASES), 3)
    hand = samio.ReadSet.from_records(records)
    cov_case(hand, M.mate_table_of(hand, keys)[0], 0, F.HAND_LENGTH, 0, 0, 1 << 16)
    for stranded, knobs in MODES:
        junction_case(rs, mate, 0, stranded, knobs, 1 << 16, xs)
    junction_case(rs, mate, 5000000, 1, (0, 0, 0), 7, xs)
    # mate tables the rules do not believe: at and beyond n, the read itself (the program's answer is held against the library's)
    two = samio.ReadSet.from_records([(99, 101, "30M100N30M"), (147, 111, "20M100N40M"), (99, 2001, "5M5N" * 69 + "5M")])
    for bad in ([3, 0, 2], [0xFFFFFFF0, 1, 0xFFFFFFFE], [2, 1, 0], [1, 2, 0], [2, 2, 2]):
        s, n_iv, past, intervals, totals = _hook(two, bad, 3000, cap=100)
        cov_case(two, bad, 0, 3000, 0, 0, 100, [s.tolist(), n_iv.tolist(), past.astype(int).tolist(), [v for iv in intervals for v in iv], [totals[k] for k in native.COVERAGE_FRAGMENT_TOTALS]])
        junction_case(two, bad, 0, 0, (0, 0, 0), 100, symmetric=False)          # (the yardstick knows symmetric tables)
    # CIGAR offsets that go down, and one beyond the ops: such a read has no op; a mate of no op is no partner, and carries nothing
    down = types.SimpleNamespace(pos=[101, 111, 161, 171], flag=[99, 147, 99, 147], cig_off=[2, 1, 9, 3, 4], cigar=[(30 << 4), (100 << 4) | 3, (30 << 4), (30 << 4)])
    cov_case(down, [1, 0, 3, 2], 0, 1000, 0, 0, 10, [[-3, -3, -3, 1], [0, 0, 0, 1], [0, 0, 0, 0], [170, 200], [1, 4, 1, 0, 30, 0]])
    junction_case(down, [1, 0, 3, 2], 0, 0, (0, 0, 0), 10, expect=[[0, 0, 0, 0], [0, 0, 0, 0], []])
    noop = types.SimpleNamespace(pos=[101, 111], flag=[99, 147], cig_off=[0, 0, 3], cigar=[(20 << 4), (100 << 4) | 3, (40 << 4)])          # the EARLIER mate has no op
    cov_case(noop, [1, 0], 0, 1000, 0, 0, 10, [[-3, 1], [0, 2], [0, 0], [110, 130, 230, 270], [2, 2, 1, 0, 60, 0]])
    junction_case(noop, [1, 0], 0, 0, (0, 0, 0), 10, expect=[[0, 1], [0, 0], [130, 230, 63, 20, 40, 0]])
    empty = types.SimpleNamespace(pos=[], flag=[], cig_off=[0], cigar=[])
    cov_case(empty, [], 0, 10, 0, 0, 0, [[], [], [], [], [0] * 6])
    junction_case(empty, [], 0, 0, (0, 0, 0), 0, expect=[[], [], []])
    path = tmp_path / "cases.txt"
    path.write_text("\n".join(lines) + "\n")
    out = subprocess.run([exe, str(path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0"))
    assert out.returncode == 0, out.stderr
    got = out.stdout.split("\n")
    assert len(got) >= len(want)
    for k, line in enumerate(want):
        assert [int(v) for v in got[k].split()] == [int(v) for v in line], k


# ---- the command line ---------------------------------------------------------------------------------------------------------
def test_the_switches(capsys):
    p = cli.build_parser(fragment_switches=True)          # (the parser `main` builds; without the argument it is the parser of before, which refuses both)
    for command, extra in (("coverage", []), ("intronretention", ["-A", "g"])):
        with pytest.raises(SystemExit):
            cli.build_parser().parse_args([command, "-B", "x", "-o", "o", "--fragments"] + extra)
        assert "fragments" not in vars(p.parse_args([command, "-B", "x", "-o", "o"] + extra))          # without it, the arguments are what they were
        assert vars(p.parse_args([command, "-B", "x", "-o", "o", "--fragments"] + extra))["fragments"] is True
    for command in ("junctions", "process", "strandedness", "flagstat"):          # alpha stays per read: no such option
        with pytest.raises(SystemExit):
            p.parse_args([command, "-B", "x", "-o", "o", "--fragments"])
    capsys.readouterr()
    with pytest.raises(SystemExit) as err:
        cli.main(["coverage", "-B", "x.bam", "-o", "o", "--perMillion", "--fragments"])
    text = capsys.readouterr().err
    assert err.value.code == 2 and "--perMillion --fragments" in text and "library size" in text
    with pytest.raises(ValueError, match="perMillion"):
        cov.coverage("x.bam", "o", perMillion=True, fragments=True)


def test_the_functions_take_the_switch_and_refuse_a_source_without_keys():
    import inspect
    assert inspect.signature(cov.coverage).parameters["fragments"].default is False
    assert inspect.signature(ir.intronretention).parameters["fragments"].default is False
    assert inspect.signature(native.DeviceReads.coverage).parameters["fragments"].default is False
    assert inspect.signature(native.DeviceReads.junctions).parameters["fragments"].default is False
    assert inspect.signature(native.DeviceReads.intron_depth).parameters["fragments"].default is False

    class NoKeys(object):
        mate_keys = False
        ref_names = []
    with pytest.raises(native.SpliserNativeError, match="name keys"):
        list(cov.sets_of_source(NoKeys(), 0, [], with_keys=True))
    with pytest.raises(native.SpliserNativeError, match="name keys"):
        list(cov.runs_of_source(NoKeys(), 0, [], fragments=True))
