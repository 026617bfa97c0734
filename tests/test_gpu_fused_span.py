"""The fused range kernel's simple reads (run 0), round 14: a thread asks one pair of position-index entries for the span of all
its simple reads (spl_simple_span.h); the simple reads of the threads whose span holds a site (FLAGGED) go to a list of
SPL_SIMPLE_LIST_FUSED entries a wave and are counted from there one read a lane; a wave with more than SPL_SIMPLE_DENSE_FUSED
flagged threads takes them slot by slot instead.  Cases built to the edges of all three, a few thousand reads each, two tiles a
chunk: fused == layout + range (SPL_FUSED=0) == oracle, counters and SSE, unstranded, fr and rf in combine mode
(test_gpu_fused_simple.py: _check).  Which threads a case flags and how many reads a wave lists is worked out on the host, with the
rule the kernel includes (native.simple_span_host), so that every case is known to reach the edge it names.

A thread holds reads 4 t .. 4 t + 3 of its tile, a wave 256 consecutive reads, a tile 1024."""
import numpy as np
import pytest

import limitcases as L
from limitcases import M, N, D
from spliser_amd import native
from test_gpu_fused_simple import _check, _dense_table, ctx  # noqa: F401  (ctx: the module's device context, a fixture)

pytestmark = pytest.mark.gpu

TILE = L.TILE
CAP = L.C["SPL_SIMPLE_LIST_FUSED"]
DENSE = L.C["SPL_SIMPLE_DENSE_FUSED"]
REC_ROOM = L.C["SPL_REC_BYTES_FUSED"] - 64
P0, STEP = 30000, 1000


def _sparse_table(n=40):
    """Sites a thousand bases apart: a read of 100 bases holds one or none."""
    tb = L.TableBuilder(5)
    rows = [tb.row(P0 + STEP * k, "+-"[k % 2]) for k in range(n)]
    for k in range(0, n - 1, 2):
        tb.link(rows[k], rows[k + 1])
    return tb.build()


def on(k, f=0, d=0):
    """A simple read over site k."""
    return (f, P0 + STEP * k - 50 + d, [(100, M)])


def gap(k, i=0, f=0):
    """A simple read between sites k and k + 1."""
    return (f, P0 + STEP * k + 200 + i % 600, [(100, M)])


def once(k, f=0):
    return (f, P0 + STEP * k + 300, [(30, M), (900, N), (30, M)])


def twice(k, f=16):
    return (f, P0 + STEP * k + 300, [(30, M), (900, N), (30, M), (900, N), (30, M)])


def other(k, f=0):
    return (f, P0 + STEP * k - 20, [(30, M), (2, D), (30, M)])


def _case(name, recs, limit, table=None):
    return L.Case("span_" + name, table if table is not None else _sparse_table(), [(L.reads_from(recs), 0)], limit)


def _threads(case):
    """-> (flagged per thread, listed reads per wave): the kernel's rule on the host, for one segment laid from index 0 on."""
    recs = L.records(case.reads)
    n = (len(recs) + 3) // 4 * 4
    pos, length, simple = np.zeros(n, np.int64), np.ones(n, np.int64), np.zeros(n, bool)
    for i, (f, p, ops) in enumerate(recs):
        if L.read_class(ops, f) == 0:
            pos[i], length[i], simple[i] = p, ops[0][0], True
    flagged, _, _, _ = native.simple_span_host(case.table.dpos(), pos, length, simple)
    listed = (np.repeat(flagged, 4) & simple).astype(np.int64)
    listed = np.concatenate((listed, np.zeros(-n % 256, np.int64))).reshape(-1, 256).sum(axis=1)
    fl = np.concatenate((flagged, np.zeros(-len(flagged) % 64, bool))).reshape(-1, 64).sum(axis=1)
    return flagged, listed, fl


def _unstranded(oracle_lib, case):
    t, r = case.table, case.reads
    return oracle_lib.check_bam(t.pos, t.strand, t.part_off, t.part_pos, t.comp_off, t.comp_pos, r.pos, r.flag, r.cig_off, r.cigar, 0, 0)


def _counted(oracle_lib, case):
    """beta1 + beta2Simple reads over all rows, unstranded (the oracle alone: what a case is built to count or not to count)."""
    want = _unstranded(oracle_lib, case)
    return int(want[0].sum()) + int(want[1].sum())


def _run(ctx, oracle_lib, monkeypatch, case, **kw):
    """_check, -> what the oracle counts unstranded."""
    _check(ctx, oracle_lib, monkeypatch, case, **kw)
    return _counted(oracle_lib, case)


# ---- the span test ------------------------------------------------------------------------------------------------------------

def test_no_thread_flagged_and_then_one(ctx, oracle_lib, monkeypatch):
    """Simple reads only, every thread's four in one gap between sites: nothing is flagged, listed or counted -- until one read is
    moved onto a site."""
    recs = [gap((i // 4) % 38, 37 * i, (0, 16)[i % 2]) for i in range(2 * TILE + 301)]
    case = _case("none", recs, "no thread flagged")
    flagged, _, _ = _threads(case)
    assert not flagged.any()
    assert _run(ctx, oracle_lib, monkeypatch, case) == 0
    recs[TILE + 402] = on(7)
    case = _case("one", recs, "one thread flagged")
    assert _threads(case)[0].sum() == 1
    assert _run(ctx, oracle_lib, monkeypatch, case) > 0


def test_flagged_threads_without_an_emitting_read(ctx, oracle_lib, monkeypatch):
    """Two reads left of a site and two right of it, in both orders: the span holds the site, no read does."""
    recs = []
    for t in range(TILE // 4 + 77):
        k = t % 37
        recs += [gap(k, 9 * t), gap(k + 1, 5 * t, 16), gap(k, 3 * t, 16), gap(k + 1, t)] if t % 2 else [gap(k + 1, t), gap(k, 9 * t), gap(k + 1, 2 * t), gap(k, t, 16)]
    case = _case("gap", recs, "every thread flagged, nothing counted")
    flagged, listed, _ = _threads(case)
    assert flagged.all() and listed.max() == 256
    assert _run(ctx, oracle_lib, monkeypatch, case) == 0


@pytest.mark.parametrize("slot", [0, 1, 2, 3])
def test_emitting_read_in_each_slot_beside_other_classes(slot, ctx, oracle_lib, monkeypatch):
    """The thread's one simple read in slot `slot` -- over a site in every third thread, between sites in the others --, a
    once-spliced, a twice-spliced and another read in the other slots."""
    recs = []
    for t in range(TILE // 4 + 130):
        k = t % 36
        rest = [once(k, (0, 16)[t % 2]), twice(k), other(k + 1)]
        rest.insert(slot, on(k, (0, 16, 99, 147)[t % 4], t % 5 - 2) if t % 3 == 0 else gap(k, 11 * t))
        recs += rest
    case = _case("slot_%d" % slot, recs, "one simple read a thread, slot %d" % slot)
    flagged, listed, _ = _threads(case)
    assert 0 < flagged.sum() < len(flagged) and listed.max() <= CAP
    assert _run(ctx, oracle_lib, monkeypatch, case) > 0


def test_reads_in_descending_order_within_a_thread(ctx, oracle_lib, monkeypatch):
    """The least start and the greatest end anywhere among the four: descending, and with both in the middle slots."""
    recs = []
    for t in range(TILE // 4 + 50):
        k = t % 30
        four = [gap(k + 2, t), on(k + 1, 16) if t % 4 == 0 else gap(k + 1, t), gap(k, 7 * t), gap(k, 0)]        # descending
        if t % 2:
            four = [four[1], four[0], four[3], four[2]]                                                        # max, min in slots 1 and 2
        if t % 5 == 0:
            four = [gap(k, 500), gap(k, 300, 16), gap(k, 100), gap(k, 0)]                                       # descending, one gap: not flagged
        recs += four
    case = _case("descending", recs, "min / max not at the ends")
    flagged, _, _ = _threads(case)
    assert flagged.any() and not flagged.all()
    assert _run(ctx, oracle_lib, monkeypatch, case) > 0


# ---- the list -----------------------------------------------------------------------------------------------------------------

def _wave(n_flagged_threads, extra=0, seed=0):
    """256 reads: n_flagged_threads threads of four simple reads with one over a site (four listed reads each), `extra` threads
    whose only simple read lies over a site (one listed read each, in slot 0), the others four reads in one gap -- the flagged
    threads spread over the wave."""
    kinds = ["flag"] * n_flagged_threads + ["extra"] * extra + ["fill"] * (64 - n_flagged_threads - extra)
    kinds = list(np.random.default_rng(seed).permutation(kinds))
    recs = []
    for t, kind in enumerate(kinds):
        k = (t + seed) % 36
        if kind == "flag":
            four = [gap(k, t), gap(k, 3 * t, 16), gap(k, 5 * t), gap(k, 7 * t)]
            four[t % 4] = on(k + (t % 2), (0, 16)[t % 2], t % 7 - 3)
            recs += four
        elif kind == "extra":
            recs += [on(k, 16), once(k), other(k), twice(k)]
        else:
            recs += [gap(k, 13 * t + j, (0, 16)[j % 2]) for j in range(4)]
    return recs


@pytest.mark.parametrize("n_listed", sorted({CAP - 1, CAP, CAP + 1, 2 * CAP, 4 * DENSE}))
def test_list_capacity(n_listed, ctx, oracle_lib, monkeypatch):
    """A wave that lists exactly SPL_SIMPLE_LIST_FUSED reads, one fewer, one more (the list is drained and filled again in the
    middle of slot 3), two lists full, and as many as the flagged-thread threshold lets through the list -- in the first wave of
    the first tile and in the third wave of the second one, ordinary waves around them."""
    full, extra = divmod(n_listed, 4)
    assert full + extra <= DENSE
    special = _wave(full, extra, seed=n_listed)
    recs = special + _wave(3, 1, 1) + _wave(0, 0, 2) + _wave(5, 2, 3) + _wave(2, 0, 4) + _wave(1, 1, 5) + special + _wave(4, 0, 6)[:133]
    case = _case("list_%d" % n_listed, recs, "%d listed reads in a wave" % n_listed)
    _, listed, fl = _threads(case)
    assert listed[0] == n_listed and listed[6] == n_listed and fl.max() <= DENSE
    assert _run(ctx, oracle_lib, monkeypatch, case) > 0


@pytest.mark.parametrize("n_flagged", [DENSE, DENSE + 1, 64])
def test_flagged_thread_threshold(n_flagged, ctx, oracle_lib, monkeypatch):
    """SPL_SIMPLE_DENSE_FUSED flagged threads in a wave (the list), one more and all 64 (slot by slot)."""
    recs = _wave(n_flagged, 0, 7) + _wave(2, 1, 8) + _wave(n_flagged, 0, 9) + _wave(0, 0, 10) + _wave(n_flagged, 0, 11)[:201]
    case = _case("dense_%d" % n_flagged, recs, "%d flagged threads in a wave" % n_flagged)
    _, _, fl = _threads(case)
    assert fl[0] == n_flagged and fl[2] == n_flagged
    assert _run(ctx, oracle_lib, monkeypatch, case) > 0


def test_every_thread_flagged_over_dense_sites(ctx, oracle_lib, monkeypatch):
    """A tile of 1024 simple reads over sites every three bases, and a partial one."""
    rng = np.random.default_rng(4)
    recs = [(int(rng.choice([0, 16, 99, 147])), 40000 + int(rng.integers(0, 4200)), [(int(rng.integers(2, 150)), M)]) for _ in range(TILE + 300)]
    case = _case("all_flagged", recs, "every thread flagged", table=_dense_table())
    flagged, _, fl = _threads(case)
    assert flagged[:TILE // 4].all() and fl[0] == 64
    assert _run(ctx, oracle_lib, monkeypatch, case) > 0


@pytest.mark.parametrize("last", [1, 2, 3])
def test_partial_last_tile_whose_last_thread_holds_fewer_reads(last, ctx, oracle_lib, monkeypatch):
    recs = _wave(6, 1, 12) * 4 + _wave(3, 0, 13)[:4 * 17] + [on(9, 16), on(9, 0, 3), on(10)][:last]
    case = _case("last_%d" % last, recs, "a last thread of %d reads" % last)
    assert len(recs) % 4 == last and _threads(case)[0][-1]
    assert _run(ctx, oracle_lib, monkeypatch, case) == _counted(oracle_lib, _case("last_%d_without" % last, recs[:-last], "without them")) + last


def test_tile_in_halves_with_flagged_threads(ctx, oracle_lib, monkeypatch):
    """724 twice-spliced reads and 300 simple ones in one tile: its records do not fit, it is taken in halves -- the simple reads,
    flagged threads among them, were counted when it was looked at in one piece and are not counted again."""
    assert 724 * L.C["SPL_REC_M2"] > REC_ROOM
    simple = (_wave(10, 2, 14) + _wave(DENSE + 3, 0, 15))[:300]
    recs = simple[:150] + [twice(i % 30, (0, 16)[i % 2]) for i in range(724)] + simple[150:] + _wave(4, 1, 16) + [other(i % 30) for i in range(90)]
    case = _case("halves", recs, "a tile in halves")
    assert _threads(case)[0][:256].any()
    assert _run(ctx, oracle_lib, monkeypatch, case) > 0


@pytest.mark.parametrize("win", [L.WIN, L.WIN_STRANDED_FUSED])
def test_listed_reads_left_of_across_and_right_of_the_window(win, ctx, oracle_lib, monkeypatch):
    """test_gpu_fused_simple.py's window case with its reads coming out of the list: fewer threads a wave than the threshold hold them, the others
    reads far in front of the table (POS before the chunk's first one, nothing flagged).  Both ends in LDS, one end each, both
    ends global atomics, on both strands; the stranded fused window of 508 as well."""
    lead, Q0 = 100, 40000
    body = []
    for f in (0, 16, 99, 147):
        for row, length in [(lead - 60, 100), (lead - 20, 90), (lead - 1, 3), (lead, 3), (lead + 5, 300),
                            (lead + win - 40, 3 * 38), (lead + win - 40, 3 * 39), (lead + win - 40, 3 * 40), (lead + win - 40, 3 * 41),
                            (lead + win - 1, 2), (lead + win, 2), (lead + win + 1, 2), (lead + win + 30, 200), (lead - 90, 3 * (win + 200))]:
            for d in (-1, 0, 1):
                body.append((f, Q0 + 3 * row + d, [(length, M)]))
    far = lambda i: (0, 2000 + i % 900, [(80, M)])
    recs = [(0, Q0 + 3 * lead, [(40, M)]), far(1), far(2), far(3)]           # the chunk's first read: the window's base
    while body:
        recs += body[:4 * (DENSE - 4)]
        body = body[4 * (DENSE - 4):]
        recs += [far(len(recs) + i) for i in range(-len(recs) % 256)]
    case = _case("window_%d" % win, recs, "window of %d" % win, table=_dense_table())
    _, listed, fl = _threads(case)
    assert fl.max() <= DENSE and listed.sum() == 168 + 4     # (the first thread's span runs from its far reads to the first read: all four are listed)
    _check(ctx, oracle_lib, monkeypatch, case, modes=[(0, 0), (1, 0), (2, 0), (2, 1)])
    assert _counted(oracle_lib, case) > 0


def test_identical_simple_reads_on_one_site(ctx, oracle_lib, monkeypatch):
    """2000 equal reads in a row (every thread flagged: slot by slot), and 21 waves more of them through the list: as many threads a
    wave as the threshold allows, whole list passes of nothing but equal keys."""
    same = (0, P0 + STEP * 8 - 20, [(60, M)])
    recs = [same] * 2000 + [gap(3, i) for i in range(48)]
    for w in range(21):
        recs += [same] * (4 * DENSE) + [gap((w + i // 4) % 30, i) for i in range(256 - 4 * DENSE)]
    case = _case("identical", recs, "equal keys through whole list passes")
    _, listed, fl = _threads(case)
    assert (listed[8:] == 4 * DENSE).all() and fl[0] == 64
    _check(ctx, oracle_lib, monkeypatch, case)
    assert int(_unstranded(oracle_lib, case)[0].max()) == 2000 + 21 * 4 * DENSE
