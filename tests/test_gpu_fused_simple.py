"""The fused range kernel counts a read of run 0 (one aligned op, mapped, placed, in range) where it classifies it, from the
thread's registers: such a read has no record, no rank and no place in LDS.  The record area then holds the tile's other reads
only -- SPL_REC_BYTES_FUSED - 64 bytes of records -- and a tile that needs more is laid out and counted in two halves.  Cases
built to the edges of both, each a few thousand reads: the fused pass against the oracle and against the same shard through
layout + range (SPL_FUSED=0), bit for bit -- beta1, beta2Simple's reads and the double counts (which is where the literal queue's
reads end up: a queue entry that named the wrong read would count the wrong read), and the beta2 / SSE doubles."""
import numpy as np
import pytest

import limitcases as L
from limitcases import M, N, D, S, H
from spliser_amd import native

pytestmark = pytest.mark.gpu

TILE = L.TILE
REC_ROOM = L.C["SPL_REC_BYTES_FUSED"] - 64      # bytes of records a tile's runs 1 .. 3 may take (spl_kernels.hip: REC_ROOM)
REC_MNM, REC_M2, REC_OTHER = L.C["SPL_REC_MNM"], L.C["SPL_REC_M2"], L.C["SPL_REC_OTHER"]
MODES = [(0, 0), (1, 0), (2, 1)]                # unstranded; fr; rf in combine mode


@pytest.fixture(scope="module")
def ctx():
    with native.Context(0) as c:
        yield c


def _check(ctx, oracle_lib, monkeypatch, case, modes=MODES, queued=None):
    """fused == layout + range == oracle, counters and SSE, in every mode; the fused run really was the fused kernel."""
    sites = case.table.sites()
    t, r = case.table, case.reads
    monkeypatch.setenv("SPL_FORCE_CHUNK", str(L.CHUNK))
    for stranded, combine in modes:
        want = oracle_lib.check_bam(t.pos, t.strand, t.part_off, t.part_pos, t.comp_off, t.comp_pos, r.pos, r.flag, r.cig_off, r.cigar,
                                    stranded, combine)
        cryptic = (stranded + combine) % 2 == 0
        want_sse = oracle_lib.beta2_sse(t.pos, t.part_off, t.part_pos, t.part_site, t.alpha, t.edge_cnt, want[0], want[1], want[2], cryptic)
        got = {}
        for fused in (False, True):
            monkeypatch.setenv("SPL_FUSED", "1" if fused else "0")
            got[fused] = L.count_device(ctx, sites, case.segments, stranded, combine, cryptic)
            tag = (case.name, "stranded", stranded, "combine", combine, "fused", fused)
            assert got[fused].fused == fused, tag
            for w, g in zip(want, got[fused].counters):
                assert np.array_equal(w, g), tag
            for w, g in zip(want_sse, got[fused].sse):
                assert np.array_equal(np.asarray(g), np.asarray(w), equal_nan=w.dtype.kind == "f"), tag
        for a, b in zip(got[False].counters, got[True].counters):
            assert np.array_equal(a, b), (case.name, stranded, combine)
        for a, b in zip(got[False].sse, got[True].sse):
            assert np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True), (case.name, stranded, combine)
        if queued is not None and not combine:
            assert got[True].queued >= queued, (case.name, got[True].queued, queued)
    return want


def _mixed(rng, classes):
    return [L._mixed_read(rng, int(c)) for c in classes]


def _case(name, recs, limit):
    return L.Case("simple_" + name, L._tile_table(), [(L.reads_from(recs), 0)], limit)


# ---- what a tile is made of ---------------------------------------------------------------------------------------------------

def test_tile_without_a_simple_read(ctx, oracle_lib, monkeypatch):
    rng = np.random.default_rng(1)
    want = _check(ctx, oracle_lib, monkeypatch, _case("none", _mixed(rng, rng.integers(1, 6, 1500)), "no read of run 0 in either tile"))
    assert int(want[0].sum()) > 0


def test_tiles_of_simple_reads_only(ctx, oracle_lib, monkeypatch):
    """Runs 1 .. 3 see no record at all, in full tiles and in a partial one."""
    rng = np.random.default_rng(2)
    want = _check(ctx, oracle_lib, monkeypatch, _case("only", _mixed(rng, [0] * (2 * TILE + 301)), "reads of run 0 only"))
    assert int(want[0].sum()) > 0


@pytest.mark.parametrize("cls", [0, 1])
def test_single_read(cls, ctx, oracle_lib, monkeypatch):
    recs = [(0, 30000 - 10, [(60, M)])] if cls == 0 else [(16, 30000 - 10, [(11, M), (7, N), (30, M)])]
    want = _check(ctx, oracle_lib, monkeypatch, _case("single_%d" % cls, recs, "one read"))
    assert int(want[0].sum()) + int(want[1].sum()) > 0


# ---- partial tiles ------------------------------------------------------------------------------------------------------------

def test_chunk_that_begins_inside_a_cell_and_ends_in_a_partial_tile(ctx, oracle_lib, monkeypatch):
    """Two segments end to end in one set of arrays: the second one's first chunk begins at index 701 -- inside a tile, inside a
    thread's four reads -- and its last tile holds 1503 + 701 - 2048 = 156 reads; neither count is a multiple of four."""
    rng = np.random.default_rng(3)
    sh0, sh1 = 500, 7000
    s0 = [(f, p - sh0, ops) for f, p, ops in _mixed(rng, rng.choice([0, 0, 0, 1, 2, 3, 5], 701))]
    s1 = [(f, p - sh1, ops) for f, p, ops in _mixed(rng, rng.choice([0, 0, 0, 1, 2, 3, 5], 1503))]
    case = L.Case("simple_mid_cell", L._tile_table(), [(L.reads_from(s0), sh0), (L.reads_from(s1), sh1)], "a chunk from index 701 on")
    _check(ctx, oracle_lib, monkeypatch, case, queued=1)


# ---- the record area: exactly full, and one record more (the tile in two halves) ----------------------------------------------------

def _fill(kind, over):
    """A first tile whose records of runs 1 .. 3 take REC_ROOM bytes exactly (over = False) or one record more, simple reads making
    up the tile's 1024 where there is room for them, in an order that puts simple reads before, between and behind the others;
    then a second, ordinary tile."""
    rng = np.random.default_rng(len(kind) + over)
    if kind == "once":          # 16-byte records, two of 24 to land on the byte
        assert (TILE - 3) * REC_MNM + 2 * REC_M2 == REC_ROOM
        cls = [1] * (TILE - 3) + [2] * 2 + [1 if over else 0]
    elif kind == "twice":       # 24-byte records of twice-spliced and other reads, one of 16
        n24 = (REC_ROOM - REC_MNM) // REC_M2
        assert n24 * REC_M2 + REC_MNM == REC_ROOM and n24 + 2 < TILE
        cls = [2] * (n24 // 2) + [3] * (n24 - n24 // 2) + [1] + ([2] if over else []) + [0] * (TILE - n24 - 1 - over)
    else:                       # WIDE reads of nine ops: the tile's ops take more than one window of 4 TILE words as well
        n24 = (REC_ROOM - REC_MNM) // REC_OTHER
        cls = [4] * n24 + [1] + ([4] if over else []) + [0] * (TILE - n24 - 1 - over)
        assert 9 * n24 > 4 * TILE
    cls = list(rng.permutation(cls))
    assert len(cls) == TILE
    need = sum({1: REC_MNM, 2: REC_M2, 3: REC_OTHER, 4: REC_OTHER, 5: REC_OTHER}.get(int(c), 0) for c in cls)
    assert need == REC_ROOM + (0 if not over else (REC_MNM if kind == "once" else REC_M2)), need
    return _mixed(rng, cls) + _mixed(rng, rng.integers(0, 6, 333))


@pytest.mark.parametrize("over", [False, True])
@pytest.mark.parametrize("kind", ["once", "twice", "wide"])
def test_record_area_full_and_one_record_more(kind, over, ctx, oracle_lib, monkeypatch):
    _check(ctx, oracle_lib, monkeypatch, _case("fill_%s_%d" % (kind, over), _fill(kind, over), "records of %d bytes%s" % (REC_ROOM, " + 1 record" if over else "")))


def test_tiles_in_halves_in_partial_cells(ctx, oracle_lib, monkeypatch):
    """Segments end to end in one set of arrays.  700 twice-spliced reads: their tile goes in halves of 512 and 188 reads.  Then a
    chunk in the second half of that cell only (it fits: half a tile always does), then one whose first tile goes in halves with
    simple reads in the first of them, and a last partial tile."""
    rng = np.random.default_rng(5)
    s0 = _mixed(rng, [2] * 700)
    s1 = _mixed(rng, [3] * 300 + [0] * 24)
    s2 = _mixed(rng, [0] * 300 + [2] * 724 + [3] * 400 + [0] * 77)
    case = L.Case("simple_halves", L._tile_table(), [(L.reads_from(s0), 0), (L.reads_from(s1), 0), (L.reads_from(s2), 0)], "half tiles")
    _check(ctx, oracle_lib, monkeypatch, case)


# ---- where the commits go -----------------------------------------------------------------------------------------------------

def _dense_table(n=1500):
    tb = L.TableBuilder(17)
    rows = [tb.row(40000 + 3 * k, "+-"[(k // 3) % 2]) for k in range(n)]
    for k in range(0, n - 1, 2):
        tb.link(rows[k], rows[k + 1])
    return tb.build()


@pytest.mark.parametrize("win", [L.WIN, L.WIN_STRANDED_FUSED])
def test_simple_reads_left_of_across_and_right_of_the_window(win, ctx, oracle_lib, monkeypatch):
    """The chunk's window begins at the site of its first read, row `lead`, and ends win distinct positions further: simple reads
    wholly left of it, across its left edge, inside, across its right edge (ending at its last entry - 1, on it and behind it)
    and wholly right of it -- both ends in LDS, one end each, both ends global atomics -- on both strands."""
    lead, P0 = 100, 40000
    recs = [(0, P0 + 3 * lead, [(40, M)])]
    for f in (0, 16, 99, 147):
        for row, length in [(lead - 60, 100), (lead - 20, 90), (lead - 1, 3), (lead, 3), (lead + 5, 300),
                            (lead + win - 40, 3 * 38), (lead + win - 40, 3 * 39), (lead + win - 40, 3 * 40), (lead + win - 40, 3 * 41),
                            (lead + win - 1, 2), (lead + win, 2), (lead + win + 1, 2), (lead + win + 30, 200), (lead - 90, 3 * (win + 200))]:
            for d in (-1, 0, 1):
                recs.append((f, P0 + 3 * row + d, [(length, M)]))
    recs += [(16, P0 + 3 * lead + 10, [(20, M), (30, N), (25, M)])] * 5
    case = L.Case("simple_window_%d" % win, _dense_table(), [(L.reads_from(recs), 0)], "window of %d" % win, modes=[(0, 0), (1, 0), (2, 0), (2, 1)])
    want = _check(ctx, oracle_lib, monkeypatch, case, modes=case.modes)
    assert int(want[0].sum()) > 0


def test_simple_reads_that_end_at_a_site_and_one_behind_it(ctx, oracle_lib, monkeypatch):
    """beta1 needs both t and t + 1 under one op: reads ending at t - 1, t, t + 1, t + 2 and beginning at t - 1 .. t + 2."""
    t = 30000 + 7 * 50
    recs = []
    for f in (0, 16):
        for last in (t - 1, t, t + 1, t + 2):
            recs.append((f, last - 49, [(50, M)]))
        for first in (t - 1, t, t + 1, t + 2):
            recs.append((f, first, [(50, M)]))
        recs.append((f, t, [(1, M)]))
        recs.append((f, t, [(2, M)]))
    want = _check(ctx, oracle_lib, monkeypatch, _case("ends", recs, "ends at t, t + 1"))
    assert int(want[0].sum()) > 0


def test_many_identical_simple_reads_on_one_site(ctx, oracle_lib, monkeypatch):
    """Equal keys throughout a wave, and through all four reads of a thread."""
    t = 30000 + 7 * 80
    recs = [(0, t - 20, [(60, M)])] * 1500 + [(16, t - 20, [(60, M)])] * 700 + [(0, t - 30, [(31, M), (14, N), (20, M)])] * 3
    want = _check(ctx, oracle_lib, monkeypatch, _case("identical", recs, "2200 equal reads"))
    assert int(want[0].max()) >= 1500


# ---- clips, flags, modes ------------------------------------------------------------------------------------------------------

def test_clipped_reads_that_are_simple_ones_beside_plain_ones(ctx, oracle_lib, monkeypatch):
    t = 30000 + 7 * 30
    recs = []
    for k in range(300):
        p = t - 50 + (k % 9)
        recs += [(0, p, [(5, S), (95, M)]), (16, p, [(100, M)]), (99, p, [(95, M), (5, S)]), (147, p, [(3, H), (90, M), (4, S)]), (0, p, [(100, M)])]
    want = _check(ctx, oracle_lib, monkeypatch, _case("clips", recs, "5S95M beside 100M"))
    assert int(want[0].sum()) > 0


def test_reads_that_must_not_be_counted_in_place(ctx, oracle_lib, monkeypatch):
    """Flag 0x4 with a placed POS and a one-op CIGAR, '*' CIGARs, a block too long for a simple record (2^16 and more) and
    clips on clips -- each between simple reads, in one thread's four reads.
    (The 70000M block is outside what a simple record holds, the 16-bit length; a read outside the coordinate space is
    test_read_that_ends_past_the_coordinate_space_beside_simple_reads.)"""
    t = 30000 + 7 * 120
    odd = [(4, t - 20, [(60, M)]), (0, t - 20, []), (16, t - 5, [(70000, M)]), (0, t - 20, [(2, H), (3, S), (60, M)]), (20, t - 10, [(40, M)]),
           (0, t - 20, [(30, M), (2, D), (30, M)]), (0, t - 20, [(30, M), (1, L.I), (30, M)])]
    recs = []
    for k in range(400):
        recs.append((0, t - 30 + (k % 7), [(60, M)]))
        recs.append(odd[k % len(odd)])
        if k % 3 == 0:
            recs.append((16, t - 25, [(50, M)]))
    want = _check(ctx, oracle_lib, monkeypatch, _case("not_in_place", recs, "0x4, '*', long blocks"), queued=1)
    assert int(want[0].sum()) > 0


def test_read_that_ends_past_the_coordinate_space_beside_simple_reads(ctx, oracle_lib, monkeypatch):
    """One aligned op that ends exactly at SPL_COORD_MAX is a simple read like any other (its length equals the room behind its
    POS) and is counted in place; one base more and the read is out of range: not run 0, nothing is counted for it in place, and
    the count refuses the whole set (SPL_ERR_RANGE) -- there is nothing to hold against the oracle bit for bit then, so what is
    asserted is that the fused pass and layout + range (SPL_FUSED=0) both refuse it."""
    top = L.C["SPL_COORD_MAX"]
    t = 30000 + 7 * 60
    plain = [(f, t - 20 + k % 5, [(60, M)]) for k in range(300) for f in (0, 16)]
    _check(ctx, oracle_lib, monkeypatch, _case("at_coord_max", plain + [(0, top - 60, [(60, M)])] + plain[:7], "ends at SPL_COORD_MAX"))
    bad = _case("past_coord_max", plain + [(0, top - 60, [(61, M)])] + plain[:7], "ends one base past SPL_COORD_MAX")
    monkeypatch.setenv("SPL_FORCE_CHUNK", str(L.CHUNK))
    for fused in (False, True):
        monkeypatch.setenv("SPL_FUSED", "1" if fused else "0")
        with pytest.raises(native.SpliserNativeError):
            L.count_device(ctx, bad.table.sites(), bad.segments, 0, 0, False)


def test_stranded_modes_with_sites_on_both_strands(ctx, oracle_lib, monkeypatch):
    """fr and rf, with and without combine mode, more sites than the stranded fused window holds (508)."""
    rng = np.random.default_rng(9)
    P0 = 40000
    recs = [(0, P0, [(50, M)])]
    for _ in range(3000):
        f = int(rng.choice([0, 16, 99, 147, 83, 163]))
        p = P0 + int(rng.integers(0, 3 * 1400))
        recs.append((f, p, [(int(rng.integers(10, 120)), M)]) if rng.random() < 0.8 else
                    (f, p, [(int(rng.integers(5, 40)), M), (3 * int(rng.integers(2, 30)), N), (int(rng.integers(5, 40)), M)]))
    case = L.Case("simple_stranded", _dense_table(), [(L.reads_from(recs), 0)], "fr / rf / combine")
    _check(ctx, oracle_lib, monkeypatch, case, modes=[(1, 0), (2, 0), (1, 1), (2, 1), (0, 1)])


# ---- queue entries still name their reads -----------------------------------------------------------------------------------------

def test_once_spliced_reads_with_rivals_between_simple_reads(ctx, oracle_lib, monkeypatch):
    """The junction of rival_case: more rivals than the range kernel settles itself (the read goes to the literal queue, named by
    its place in the arrays) and fewer (the once-spliced run is streamed again for the marked reads) -- the spliced reads with
    simple reads before and behind them in array order, so that their slots among runs 1 .. 3 and their places in the arrays
    differ."""
    for which in ("once_%d" % (L.RIV_ONCE + 1), "once_%d" % L.RIV_ONCE):
        base = L.rival_case(which)
        l, r = base.meta["junction"]
        recs = []
        for i, rec in enumerate(L.records(base.reads)[:1200]):
            recs += [(0, l - 30 - (i % 5), [(45, M)])] * (i % 3)
            recs.append(rec)
            recs.append((16, r - 5, [(40 + (i % 4), M)]))
        case = L.Case("simple_queue_" + which, base.table, [(L.reads_from(recs), 0)], "queue entries")
        _check(ctx, oracle_lib, monkeypatch, case, queued=1 if which.endswith(str(L.RIV_ONCE + 1)) else None)
