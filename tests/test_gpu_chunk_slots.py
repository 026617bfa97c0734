"""One launch (spl_chunk_slots_kernel, spl_devpack.hip) gives a fused read set its chunks' descriptors, the range kernel's chunk
order and the fused pass's 64-byte descriptor of every slot.  What it leaves is read back (DeviceReads.slots) and held byte for
byte to a numpy restatement of the rule:
  * chunk j (a cell of the grid of `chunk` reads over the arrays' indexes, cut to its segment) goes to XCD share (j / 8) % 8;
  * its cost estimate is (3 ops + reads) / 2, its key cost / 16, at most 4095;
  * inside a share the chunks go by key, largest first, equal keys by chunk number -- the order kernel this one replaces left
    equal keys in the order its workgroup's LDS atomics were served, which nothing pinned: this order is one of those it could
    leave, and now the only one;
  * slots past a share's chunks are marked empty;
  * the descriptors' fields as spl_devpack.h names them.
Sets built to where the launch can go wrong: 1, 8, 9 chunks (a share with nothing, with one chunk, with two), 8 * 256 + 8 chunks (a
share of two workgroups), equal costs throughout, segments that begin in the middle of a cell and end in a partial chunk, long
CIGARs whose tile boundaries clamp, as many segments as the kernel looks up in LDS and more, and a share of more members than a
thread asks for at a time -- at the small chunk size, two of them at the large one as well.  Every set is also counted (count_launch + sse_launch: counters and doubles equal to the oracle's, unstranded
and in one stranded mode), and a relayout followed by a second count gives the same arrays and counters again."""
import numpy as np
import pytest

import limitcases as L
from limitcases import M, N
from spliser_amd import native, samio

TILE, CHUNK, CHUNK_BIG = L.TILE, L.CHUNK, L.CHUNK_BIG
MODES = [(0, 0), (2, 1)]                        # unstranded; rf in combine mode
NONE = 0xffffffff
SEGS_IN_LDS = 256                               # SPL_SLOTS_SEGS_LDS
ROUND = 4 * 256                                 # members of a share whose costs a workgroup asks for at a time

SLOT = np.dtype([("lo", "<i8"), ("chunk", "<u4"), ("n", "<u4"), ("shift", "<i4"), ("seg_op0", "<u4"), ("pos0", "<i4"), ("unused0", "<u4"),
                 ("ob", "<u4", (5,)), ("unused1", "<u4", (3,))])
CELL = np.dtype([("lo", "<i8"), ("n", "<u4"), ("o_lo", "<u4"), ("o_hi", "<u4"), ("seg_op0", "<u4"), ("shift", "<i4"), ("flat", "<u4")])
assert SLOT.itemsize == 64 and CELL.itemsize == 32


@pytest.fixture(scope="module")
def ctx():
    with native.Context(0) as c:
        yield c


# ---- the rule -------------------------------------------------------------------------------------------------------------------

def expected(segments, chunk):
    """[(ReadSet, shift)] laid end to end in one set of arrays -> (order uint32[8, per], slots SLOT[8, per], chunks CELL[n])."""
    pos = np.concatenate([rs.pos for rs, _ in segments]).astype(np.int32)
    off, first, ops = [np.zeros(1, np.int64)], [], 0
    at = 0
    for rs, _ in segments:
        first.append(at)
        off.append(rs.cig_off[1:rs.n + 1].astype(np.int64) + ops)
        at += rs.n
        ops += int(rs.cig_off[rs.n]) if rs.n else 0
    off = np.concatenate(off)
    cells = []
    for (rs, shift), f in zip(segments, first):
        if not rs.n:
            continue
        for cell in range(f // chunk, (f + rs.n - 1) // chunk + 1):
            lo, hi = max(f, cell * chunk), min(f + rs.n, (cell + 1) * chunk)
            cells.append((lo, hi - lo, off[lo], off[hi], off[f], shift, len(cells)))
    chunks = np.array(cells, CELL)
    n = len(chunks)
    per = ((n + 7) // 8 + 7) // 8 * 8
    slots = np.zeros(n, SLOT)
    for name in ("lo", "n", "shift", "seg_op0"):
        slots[name] = chunks[name]
    slots["chunk"] = chunks["flat"]
    slots["pos0"] = np.where(chunks["n"] > 0, pos[np.minimum(chunks["lo"], len(pos) - 1)], 0)
    hi = chunks["lo"] + chunks["n"]
    c0 = chunks["lo"] // chunk * chunk
    tiles = chunk // TILE
    for q in range(5):
        i = np.clip(c0 + q * TILE, chunks["lo"], hi)
        slots["ob"][:, q] = chunks["o_lo"] if q == 0 else (chunks["o_hi"] if q >= tiles else off[i])
    cost = (3 * (chunks["o_hi"].astype(np.int64) - chunks["o_lo"]) + chunks["n"]) // 2
    key = np.minimum(cost >> 4, 4095)
    j = np.arange(n)
    share = j // 8 % 8
    order = np.full((8, per), NONE, np.uint32)
    by_slot = np.zeros((8, per), SLOT)
    by_slot["chunk"] = NONE
    for x in range(8):
        mine = j[share == x]
        mine = mine[np.lexsort((mine, -key[mine]))]             # key, largest first; equal keys by chunk number
        order[x, :len(mine)] = mine
        by_slot[x, :len(mine)] = slots[mine]
    return order, by_slot, chunks


def test_the_restatement_on_a_set_small_enough_to_do_by_hand():
    """Nine chunks of 2048 one-op reads but for chunk 3 (three ops a read): chunk 3 leads share 0, chunk 8 is share 1's only one."""
    recs = [(0, 100 + i, [(50, M)] if i // CHUNK != 3 else [(20, M), (7, N), (20, M)]) for i in range(9 * CHUNK)]
    order, slots, chunks = expected([(L.reads_from(recs), 5)], CHUNK)
    assert order.shape == (8, 8) and list(order[0]) == [3, 0, 1, 2, 4, 5, 6, 7] and list(order[1]) == [8] + [NONE] * 7 and (order[2:] == NONE).all()
    assert slots["chunk"][0, 0] == 3 and slots["lo"][0, 0] == 3 * CHUNK and slots["pos0"][0, 0] == 100 + 3 * CHUNK and slots["shift"][0, 0] == 5
    assert list(slots["ob"][0, 0]) == [3 * CHUNK, 3 * CHUNK + 3 * TILE, 6 * CHUNK, 6 * CHUNK, 6 * CHUNK]
    assert chunks["o_hi"][8] == 11 * CHUNK and chunks["flat"][8] == 8


# ---- the sets -------------------------------------------------------------------------------------------------------------------

_POOL = {}


def _bulk(n, equal=False):
    """n simple, once- and twice-spliced reads over _tile_table's sites, made array by array; stretches of one class, so that the
    chunks' cost estimates differ (equal: every read 150M, every full chunk's cost the same)."""
    if equal:
        rng = np.random.default_rng(5)
        return samio.ReadSet(30000 + np.sort(rng.integers(-40, 2700, n)).astype(np.int64), rng.choice([0, 16, 99, 147], n).astype(np.uint16),
                             np.arange(n + 1, dtype=np.uint32), np.full(n, (150 << 4) | M, np.uint32))
    if "all" not in _POOL:
        rng = np.random.default_rng(66)
        big = (8 * 256 + 8) * CHUNK
        cls = rng.choice([0, 0, 0, 1, 1, 2], big)
        cls[(np.arange(big) // 3000) % 3 == 1] = 0
        off = np.concatenate(([0], np.cumsum(1 + 2 * cls))).astype(np.int64)
        at = off[:-1]
        m_len, n_len = rng.integers(5, 60, (big, 3)).astype(np.uint32), (7 * rng.integers(1, 9, (big, 2))).astype(np.uint32)
        cig = np.zeros(off[-1], np.uint32)
        cig[at] = (m_len[:, 0] << 4) | M
        for k in (1, 2):
            sel = cls >= k
            cig[at[sel] + 2 * k - 1] = (n_len[sel, k - 1] << 4) | N
            cig[at[sel] + 2 * k] = (m_len[sel, k] << 4) | M
        pos = 30000 + rng.integers(-40, 2700, big).astype(np.int64)
        pos[128 * CHUNK:] += 1000000                            # (the oracle's time goes with the reads over sites: the first 128 chunks')
        _POOL["all"] = (pos, rng.choice([0, 16, 99, 147], big).astype(np.uint16), off, cig)
    pos, flag, off, cig = _POOL["all"]
    return samio.ReadSet(pos[:n].copy(), flag[:n].copy(), off[:n + 1].astype(np.uint32), cig[:off[n]].copy())


def _take(rs, a, b):
    o = rs.cig_off.astype(np.int64)
    return samio.ReadSet(rs.pos[a:b].copy(), rs.flag[a:b].copy(), (o[a:b + 1] - o[a]).astype(np.uint32), rs.cigar[o[a]:o[b]].copy())


def _segments(which):
    if which == "chunks_1":
        return [(_bulk(CHUNK - 600), 0)]
    if which == "chunks_8":
        return [(_bulk(8 * CHUNK), 0)]
    if which == "chunks_9":
        return [(_bulk(8 * CHUNK + 1), 0)]                      # (share 1's only chunk is one read)
    if which == "chunks_2056":
        return [(_bulk((8 * 256 + 8) * CHUNK - 77), 0)]
    if which == "equal_costs":
        return [(_bulk(70 * CHUNK - 5, equal=True), 0)]
    if which == "segments":     # three references in one set of arrays: the second begins in the middle of a cell, the last chunk is partial
        rs = _bulk(11 * CHUNK)
        cuts = [0, 2 * CHUNK + 700, 2 * CHUNK + 700, 7 * CHUNK + TILE + 1, 10 * CHUNK + 333]
        return [(_take(rs, cuts[k], cuts[k + 1]), 900 * k) for k in range(4)]
    if which == "long_cigars":  # nine ops a read and soft clips: a tile's ops are more than a stage, the boundaries' offsets far apart
        rng = np.random.default_rng(9)
        cls = rng.choice([4, 4, 4, 0, 1], 3 * CHUNK_BIG + TILE + 9)
        cls[:TILE + 5] = 4
        return [(L.reads_from([L._mixed_read(rng, int(c)) for c in cls[:700]]), 0), (L.reads_from([L._mixed_read(rng, int(c)) for c in cls[700:]]), 0)]
    if which.startswith("many_segments_"):     # a few reads a segment, every one a chunk of its own: as many segments as are looked up in LDS, one
        n_segs = int(which.rsplit("_", 1)[1])   # more, many more; and enough of one read each that a thread has more members than it takes at a time
        each = 3 if n_segs < 1000 else 1
        rs = _bulk(each * n_segs)
        return [(_take(rs, each * k, each * k + each), 7 * (k % 5)) for k in range(n_segs)]
    raise KeyError(which)


CASES = [("chunks_1", CHUNK), ("chunks_8", CHUNK), ("chunks_9", CHUNK), ("chunks_9", CHUNK_BIG), ("chunks_2056", CHUNK), ("equal_costs", CHUNK),
         ("segments", CHUNK), ("segments", CHUNK_BIG), ("long_cigars", CHUNK)] + [("many_segments_%d" % k, CHUNK) for k in (SEGS_IN_LDS, SEGS_IN_LDS + 1, SEGS_IN_LDS + 44, ROUND * 8 + 1)]


def _same(got, want, tag):
    order, slots, chunks = want
    assert got["fused"], tag
    assert got["order"].shape == order.shape, tag
    assert np.array_equal(got["order"], order), tag
    assert got["chunks"].tobytes() == chunks.tobytes(), tag
    assert got["slots"].tobytes() == slots.tobytes(), tag


@pytest.mark.gpu
@pytest.mark.parametrize("which,chunk", CASES, ids=["%s-%d" % c for c in CASES])
def test_slots_order_and_descriptors_are_the_rule_s(which, chunk, ctx, oracle_lib, monkeypatch):
    segments = _segments(which)
    want = expected(segments, chunk)
    n_chunks = len(want[2])
    assert n_chunks == {"chunks_1": 1, "chunks_8": 8, "chunks_9": 9 if chunk == CHUNK else 5, "chunks_2056": 2056, "equal_costs": 70}.get(which, n_chunks)
    if which.startswith("many_segments_"):
        assert n_chunks == len(segments) and (n_chunks < 8 * ROUND or want[0].shape[1] > ROUND)
    if which == "equal_costs":      # (all full chunks of a share are one key: the order inside it is the chunk numbers')
        keys = (3 * (want[2]["o_hi"].astype(np.int64) - want[2]["o_lo"]) + want[2]["n"]) // 2 >> 4
        assert len(set(keys[:-1])) == 1 and all(list(row[row != NONE]) == sorted(row[row != NONE]) for row in want[0])
    if which == "segments":
        assert (want[2]["lo"] % chunk != 0).any() and want[2]["n"][-1] < chunk
    case = L.Case("slots_" + which, L._tile_table(), segments, which)
    t, r = case.table, case.reads
    sites = t.sites()
    monkeypatch.setenv("SPL_FORCE_CHUNK", str(chunk))
    monkeypatch.setenv("SPL_FUSED", "1")
    counted = 0
    with ctx.upload_soa([native.ReadArrays(rs.pos, rs.flag, rs.cig_off, rs.cigar) for rs, _ in segments]) as soa:
        for stranded, combine in MODES:
            tag = (which, chunk, "stranded", stranded, "combine", combine)
            counters = oracle_lib.check_bam(t.pos, t.strand, t.part_off, t.part_pos, t.comp_off, t.comp_pos, r.pos, r.flag, r.cig_off, r.cigar, stranded, combine)
            cryptic = (stranded + combine) % 2 == 0
            sse = oracle_lib.beta2_sse(t.pos, t.part_off, t.part_pos, t.part_site, t.alpha, t.edge_cnt, counters[0], counters[1], counters[2], cryptic)
            counted += int(counters[0].sum()) + int(counters[1].sum())
            with ctx.upload_sites(sites) as ds:
                dr = ctx.begin_reads(0)
                try:
                    for k, (_, shift) in enumerate(segments):
                        dr.add_soa(soa, k, shift)
                    dr.finish()
                    for again in (False, True):
                        if again:
                            dr.relayout()
                        _same(dr.slots(), want, tag + ("relayout", again))
                        ctx.count_launch(ds, dr, stranded, combine)
                        ctx.sse_launch(ds, cryptic)
                        for w, g in zip(counters, ds.counters()):
                            assert np.array_equal(w, g), tag + ("relayout", again)
                        for w, g in zip(sse, ds.sse_results()):
                            assert np.array_equal(np.asarray(g), np.asarray(w), equal_nan=w.dtype.kind == "f"), tag + ("relayout", again)
                finally:
                    dr.free()
    assert counted > 0, which
