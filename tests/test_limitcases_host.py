"""CPU checks that the cases of limitcases.py reach the limits they are built for (test_gpu_kernel_limits.py runs them on the
GPU): a change to a case or to a kernel constant that made a case miss its limit would otherwise leave its GPU test passing
without testing anything."""
import numpy as np
import pytest

import limitcases as L


def test_the_limits_come_from_the_headers():
    assert L.WIN_STRANDED_FUSED < L.WIN_STRANDED <= L.WIN
    assert L.WAVE_READS_FUSED <= L.WAVE_READS
    assert L.CHUNK_BIG == 2 * L.CHUNK and L.CHUNK % L.TILE == 0
    assert L.SCAN_BLOCK % 256 == 0
    assert 0 < L.RIV_ONCE < L.RIV_TWICE


@pytest.mark.parametrize("win", [L.WIN, L.WIN_STRANDED, L.WIN_STRANDED_FUSED])
def test_window_cases_put_range_ends_on_the_window_edge(win, oracle_lib):
    case = L.window_case(win)
    t = case.table
    recs = L.records(case.reads)
    first = recs[0][1]
    wbase = L.window_base(t, first)
    assert wbase == case.meta["wbase"] == L.pair_window_base(t, first)
    assert len(t.dpos()) == t.n                               # (one row per position: rows and dpos share their indexes)
    edge = wbase + win
    seen = set()
    for rec in recs:
        for kind, lo, ub in L.read_ranges(t, rec) or []:
            for d in (-1, 0, 1):
                if ub == edge + d and lo <= edge:
                    seen.add((kind, "end", d))
            if lo <= edge < ub:
                seen.add((kind, "one end outside"))
            if lo > edge:
                seen.add((kind, "both ends outside"))
    for kind in ("b1", "me"):
        for d in (-1, 0, 1):
            assert (kind, "end", d) in seen
        assert (kind, "one end outside") in seen and (kind, "both ends outside") in seen
    # rivals of both junctions on the edge (their keys t, t + 1 straddle it), few enough to be resolved in the range kernel
    rival_rows = set()
    for rec in recs:
        juncs = [(a, b) for a, b in _junctions(rec)]
        for j in juncs:
            rival_rows.update(t.rivals(*j))
    assert {edge - 1, edge, edge + 1} <= rival_rows
    assert any(rec[1] < first for rec in recs[1:])            # a POS before the chunk's first one
    assert any(rec[1] > t.pos[-1] for rec in recs)            # a read past the last site
    for stranded in (0, 1):
        b1, b2, _ = oracle_lib.check_bam(t.pos, t.strand, t.part_off, t.part_pos, t.comp_off, t.comp_pos, case.reads.pos,
                                         case.reads.flag, case.reads.cig_off, case.reads.cigar, stranded, 0)
        for row in (edge - 1, edge, edge + 1):
            assert b1[row] > 0 and b2[row] > 0, (stranded, row)


def _junctions(rec):
    _, p, ops = rec
    out, cur = [], p
    for ln, code in ops:
        if code == L.N:
            out.append((cur - 1, cur + ln - 1))
        cur += ln if code in (L.M, L.N, L.D, L.EQ, L.X) else 0
    return out


@pytest.mark.parametrize("which,fused", [("twice", False), ("once", False), ("once", True), ("front_first", True), ("back_first", False)])
def test_overflow_cases_fill_the_lists(which, fused):
    case = L.overflow_case(which)
    seg = L.WAVE_READS_FUSED if fused else L.WAVE_READS
    demand, extra = L.simulate_lists(case, fused, L.CHUNK_BIG)
    assert demand > seg
    if which in ("twice", "front_first"):
        assert extra > 0                                     # twice-spliced entries that only the literal queue takes
    listed = L.listed_reads(case, 0)
    assert all(x is not None for x in listed)                # every read of the chunk is listed
    if which in ("twice", "front_first", "back_first"):
        twice = [x for x, f in zip(listed, case.reads.flag) if not f & 4]
        assert twice and all(x == "back" for x in twice)     # ... and the spliced ones would not be queued if the lists had room
        assert L.simulate_lists(case, True, L.CHUNK)[1] == 0
    if which == "front_first":
        assert all(case.reads.flag[:L.CHUNK] & 4) and not any(case.reads.flag[L.CHUNK:] & 4)
    if which == "back_first":
        assert not any(case.reads.flag[:L.CHUNK] & 4) and all(case.reads.flag[L.CHUNK:] & 4)


@pytest.mark.parametrize("which", L.RIVAL_CASES)
def test_rival_cases_have_the_rivals_they_claim(which):
    case = L.rival_case(which)
    t = case.table
    l, r = case.meta["junction"]
    riv = t.rivals(l, r)
    kind, _, num = which.partition("_")
    recs = L.records(case.reads)
    classes = {L.read_class(ops, f) for f, _, ops in recs} - {0}   # (besides unspliced reads over the sites)
    if kind in ("once", "twice"):
        assert len(riv) == int(num)
        assert int(num) in (L.RIV_ONCE, L.RIV_ONCE + 1) if kind == "once" else int(num) in (L.RIV_TWICE, L.RIV_TWICE + 1)
        assert classes == ({1} if kind == "once" else {2})
        # rivals inside the intron, and rivals on a read's last aligned base (covered without t + 1)
        assert any(l < t.pos[x] < r for x in riv)
        last_bases = {sum(ln for ln, c in ops) + p - 1 for _, p, ops in recs}
        assert any(t.pos[x] in last_bases for x in riv if t.pos[x] > r)
    elif kind == "multirow":
        assert classes == {1}
        assert any(len(set(t.strand[t.rows_at(t.pos[x])].tolist())) == 2 for x in riv)
    elif kind == "complex":
        assert classes == {1}
        assert any(t.pos[x] in (l, r) for x in riv)
        assert any(len(t.rows_at(t.pos[x])) == 2 and len(set(t.strand[t.rows_at(t.pos[x])].tolist())) == 1 for x in riv)
    else:
        assert classes == {2}
        j1 = _junctions(recs[0])[0]
        assert _junctions(recs[0])[1] == (l, r)
        assert any(t.pos[x] == l for x in t.rivals(*j1))     # a rival of junction 1 is an end of junction 2
        assert len(t.rows_at(l)) == 1


@pytest.mark.parametrize("which", L.TILE_CASES)
def test_tile_cases_change_where_they_say(which):
    case = L.tile_case(which)
    recs = L.records(case.reads)
    classes = [L.read_class(ops, f) for f, _, ops in recs]
    if which.startswith("class_change_"):
        k = case.meta["change_at"]
        for c0 in range(0, len(recs), L.CHUNK):
            assert set(classes[c0:c0 + k]) == {0} and classes[c0 + k] == 1
    elif which == "all_wide":
        assert set(classes) == {3} and all(len(ops) > L.C["SPL_INLINE_OPS"] for _, _, ops in recs)
        assert len(recs) >= 2 * L.TILE
    elif which.startswith("last_tile_"):
        assert len(recs) % L.TILE == 1 and len(recs) % L.CHUNK in (1, L.TILE + 1)
    else:
        (s0, sh0), (s1, sh1) = case.segments
        assert sh0 and sh1 and sh0 != sh1
        late = s1.flag[L.TILE + 200:]
        assert np.count_nonzero(late & 4) > 100                # queued reads in the later tiles of the second segment
        assert s0.n % L.TILE and s1.n > L.CHUNK               # (it begins inside a cell and fills more than one)


@pytest.mark.parametrize("n_dpos", L.SCAN_SIZES)
def test_scan_cases_have_their_sizes(n_dpos, oracle_lib):
    for shared in (False, True):
        if shared and n_dpos > 4 * L.SCAN_BLOCK:
            continue
        case = L.scan_case(n_dpos, shared)
        t = case.table
        assert len(t.dpos()) == n_dpos
        if shared and n_dpos > 1:
            pos, counts = np.unique(t.pos, return_counts=True)
            assert counts.max() >= 3 and 0 in t.strand.tolist()
        b1, b2, _ = oracle_lib.check_bam(t.pos, t.strand, t.part_off, t.part_pos, t.comp_off, t.comp_pos, case.reads.pos,
                                         case.reads.flag, case.reads.cig_off, case.reads.cigar, 1, 0)
        if n_dpos > 1:
            zero = (t.alpha == 0) & (b1 == 0) & (b2 == 0)
            assert zero.any()                                  # a zero denominator
            assert (b1 > 0).any()
