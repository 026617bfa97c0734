"""The counting passes over BAM-native arrays resident on the device -- the fused range kernel (records made in LDS tile by tile)
and, with SPL_FUSED=0, the layout kernel + the range kernel -- held to the oracle on cases built to land on their limits
(limitcases.py): the LDS difference windows' last entry, full wave lists handing entries to the literal queue, the junction
table's rival thresholds and flags, the fused pass's tiles and segments, the scan's blocks and the SSE that rides on it.  Every
case runs at both chunk sizes, fused and not, in every strand mode, with and without combine mode; counters bit-equal, SSE
bit-equal.  A fused run that silently took layout + range fails."""
import numpy as np
import pytest

import limitcases as L
from spliser_amd import native

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    with native.Context(0) as c:
        yield c


def _want(oracle_lib, case, stranded, combine):
    t, r = case.table, case.reads
    return oracle_lib.check_bam(t.pos, t.strand, t.part_off, t.part_pos, t.comp_off, t.comp_pos, r.pos, r.flag, r.cig_off, r.cigar,
                                stranded, combine)


def _want_sse(oracle_lib, t, counts, cryptic):
    return oracle_lib.beta2_sse(t.pos, t.part_off, t.part_pos, t.part_site, t.alpha, t.edge_cnt, counts[0], counts[1], counts[2], cryptic)


def _assert_sse(got, want, tag):
    for g, w in zip(got, want):
        assert np.array_equal(np.asarray(g), np.asarray(w), equal_nan=w.dtype.kind == "f"), tag
    assert np.all(np.abs(np.asarray(got[3]) - want[3]) <= 1e-9), tag      # the tolerance BASELINE.json states


def run_device(ctx, oracle_lib, monkeypatch, case, check=None):
    """case on the device path: SPL_FORCE_CHUNK x {layout + range, fused} x the case's (stranded, combine) modes."""
    sites = case.table.sites()
    for stranded, combine in case.modes:
        want = _want(oracle_lib, case, stranded, combine)
        cryptic = (stranded + combine) % 2 == 0
        want_sse = _want_sse(oracle_lib, case.table, want, cryptic)
        for chunk in (L.CHUNK, L.CHUNK_BIG):
            lds_layout = None
            for fused in (False, True):
                monkeypatch.setenv("SPL_FORCE_CHUNK", str(chunk))
                monkeypatch.setenv("SPL_FUSED", "1" if fused else "0")
                got = L.count_device(ctx, sites, case.segments, stranded, combine, cryptic)
                tag = (case.name, "stranded", stranded, "combine", combine, "fused", fused, "chunk", chunk)
                for w, g in zip(want, got.counters):
                    assert np.array_equal(w, g), tag
                _assert_sse(got.sse, want_sse, tag)
                if fused:
                    # the fused kernel ran: no records were written, and its launch has the tile's records in LDS
                    assert got.fused and got.lds != lds_layout, tag
                else:
                    assert not got.fused, tag
                    lds_layout = got.lds
                if check:
                    check(got, stranded, combine, fused, chunk)
    return want


# ---- a. the hand-built cases of test_gpu_parity.py, through the device path -------------------------------------------------------

@pytest.mark.parametrize("name", ["non_consuming_ops", "twice_spliced_class_limits", "long_introns_and_hot_sites",
                                  "more_ops_than_the_packed_count", "star_and_unmapped_with_cigar"])
def test_hand_built_cases_on_the_device_path(name, ctx, oracle_lib, monkeypatch):
    case = {c.name: c for c in L.parity_cases()}[name]
    want = run_device(ctx, oracle_lib, monkeypatch, case)
    if name == "long_introns_and_hot_sites":
        assert int(want[0][case.meta["hot_row"]]) >= 50000


@pytest.mark.parametrize("seed", range(4))
def test_query_tables_like_combine_on_the_device_path(seed, ctx, oracle_lib, monkeypatch):
    """Tables as `combine` asks about them (no partner rows, partial lists, rows without strand)."""
    import randcase
    arr, rs = randcase.make_case(seed + 300, bool(seed % 2))
    q = randcase.query_table(arr, seed)
    assert len(q["pos"]) and rs.n
    n, n_part = len(q["pos"]), len(q["part_pos"])
    rng = np.random.default_rng(seed)
    table = L.Table(q["pos"], q["strand"], q["part_off"], q["part_pos"], np.full(n_part, -1, np.int32), q["comp_off"], q["comp_pos"],
                    rng.integers(0, 9, n), rng.integers(0, 5, n_part))
    run_device(ctx, oracle_lib, monkeypatch, L.Case("query_%d" % seed, table, [(L._repeat(rs, 23), 0)], "query table"))


# ---- b. window edges ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("win", [L.WIN, L.WIN_STRANDED, L.WIN_STRANDED_FUSED])
def test_window_edges(win, ctx, oracle_lib, monkeypatch):
    """Range ends and rival corrections at wbase + WIN - 1, WIN, WIN + 1 of every difference array; WIN = 1020 is the unstranded
    instantiations' window, 956 the stranded range kernel's, 508 the stranded fused pass's (all run in every mode)."""
    run_device(ctx, oracle_lib, monkeypatch, L.window_case(win))


def test_window_edges_pair_kernel(ctx, oracle_lib):
    """The pair kernel's window (SPL_WIN rows from the first row at or after the chunk's first POS), host-packed reads; the range
    kernel on the same host-packed reads beside it."""
    case = L.window_case(L.WIN)
    sites = case.table.sites()
    r = case.reads
    reads = native.ReadArrays(r.pos, r.flag, r.cig_off, r.cigar)
    for stranded, combine in case.modes:
        want = _want(oracle_lib, case, stranded, combine)
        for flags in (native.OPT_PAIR_KERNEL, 0):
            for w, g in zip(want, ctx.count(sites, reads, stranded, combine, flags)):
                assert np.array_equal(w, g), (stranded, combine, flags)


# ---- c. full lists -> push_direct ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("which", ["twice", "once", "front_first", "back_first"])
def test_list_overflow(which, ctx, oracle_lib, monkeypatch):
    """Chunks of nothing but listed reads.  Outside combine mode the twice-spliced ones are never queued while their wave's lists
    have room: the literal queue must hold the flag-0x4 reads plus exactly the back-list entries that limitcases.simulate_lists
    says did not fit -- which went through push_direct --; in `twice` (layout + range) and `front_first` (fused) there are such
    entries."""
    case = L.overflow_case(which)
    sim = {(f, c): L.simulate_lists(case, f, c) for f in (False, True) for c in (L.CHUNK, L.CHUNK_BIG)}
    overflowed = []

    def check(got, stranded, combine, fused, chunk):
        if combine or which == "once":
            return
        extra = sim[(fused, chunk)][1]
        assert got.queued == case.meta["n_literal"] + extra, (stranded, fused, chunk, got.queued, extra)
        if extra:
            overflowed.append((fused, chunk))
    run_device(ctx, oracle_lib, monkeypatch, case, check)
    if which in ("twice", "front_first"):       # (back_first: what overflows there is the front list, queued either way)
        assert overflowed


# ---- d. rival-table thresholds ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("which", L.RIVAL_CASES)
def test_rival_thresholds(which, ctx, oracle_lib, monkeypatch):
    want = run_device(ctx, oracle_lib, monkeypatch, L.rival_case(which))
    assert int(want[0].sum()) > 0 and int(want[1].sum()) > 0


# ---- e. tiles of the fused pass -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("which", L.TILE_CASES)
def test_tile_edges(which, ctx, oracle_lib, monkeypatch):
    run_device(ctx, oracle_lib, monkeypatch, L.tile_case(which))


# ---- f. scan / SSE edges ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_dpos,shared", [(n, False) for n in L.SCAN_SIZES] + [(n, True) for n in L.SCAN_SIZES if n <= 4 * L.SCAN_BLOCK])
def test_scan_and_sse_edges(n_dpos, shared, ctx, oracle_lib, monkeypatch):
    """The counting pass's scan with SSE (the table carries alpha, edge counts and partner rows) through run_device, and
    spl_sse_kernel (ctx.sse) on the oracle's counters, both with and without beta2Cryptic.  shared: rows of both strands and rows
    without strand at one position."""
    case = L.scan_case(n_dpos, shared)
    run_device(ctx, oracle_lib, monkeypatch, case)
    sites = case.table.sites()
    for stranded in (0, 1):
        want = _want(oracle_lib, case, stranded, 0)
        for cryptic in (False, True):
            _assert_sse(ctx.sse(sites, want[0], want[1], want[2], cryptic), _want_sse(oracle_lib, case.table, want, cryptic),
                        (n_dpos, stranded, cryptic))
