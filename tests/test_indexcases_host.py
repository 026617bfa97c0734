"""CPU checks of indexcases.py: the yardstick of the position index (index_of / resolve) agrees with brute force over sets and
bisect at every coordinate around its tables, the tables are what their names claim -- sites and flagged positions on bit 0 and bit
31, a full bucket, every phase of dbase -- and the reads of the consumer cases look up every bit of a bucket in every class
(test_gpu_site_index.py reads the device's index back and runs these cases on the GPU): a change that made a case miss its edge
would otherwise leave its GPU test passing without testing anything."""
import bisect

import numpy as np
import pytest

import indexcases as X
import limitcases as L
from limitcases import I, D, N, S

ALL = set(range(32))
FLAGS_SIMPLE = (0, 16)


# ---- the yardstick against brute force ----------------------------------------------------------------------------------------------

def _coordinates(name, index):
    lo, hi = index.lo - 200, index.hi + 200
    if name not in ("wide", X.BIG):
        return np.arange(lo, hi + 1, dtype=np.int64)
    near = np.concatenate([np.arange(p - 200, p + 201, dtype=np.int64) for p in np.concatenate((index.D, index.F)).tolist()])
    return np.unique(np.concatenate((near, np.random.default_rng(5).integers(lo, hi + 1, 10000))))


@pytest.mark.parametrize("name", sorted(X.TABLES))
def test_resolve_agrees_with_sets_and_bisect(name):
    t, index, _ = X.table(name)
    sites = sorted(set(int(p) for p in t.pos))
    site_set, flagged = set(sites), set(int(p) for p in t.junction_ends())
    assert index.n_dpos == len(sites)
    xs = _coordinates(name, index)
    u, is_site, is_flagged = X.resolve(index, xs)
    for k, x in enumerate(xs.tolist()):
        want = (bisect.bisect_left(sites, x), x in site_set, x in flagged)
        assert (int(u[k]), bool(is_site[k]), bool(is_flagged[k])) == want, (name, x)


@pytest.mark.parametrize("name", sorted(set(X.TABLES) - {"wide", X.BIG}))
def test_entries_are_the_definition_bucket_by_bucket(name):
    """first / occ / rival of every bucket by a loop over its 32 positions."""
    t, index, _ = X.table(name)
    sites, flagged = set(int(p) for p in t.pos), set(int(p) for p in t.junction_ends())
    words = index.words()
    assert words.shape == (index.n_dbuckets, 3) and words.dtype == np.uint32
    buckets = range(index.n_dbuckets) if index.n_dbuckets < 100 else list(range(40)) + list(range(index.n_dbuckets - 40, index.n_dbuckets))
    for b in buckets:
        start = index.dbase + 32 * b
        want = (sum(1 for p in sites if p < start), sum(1 << k for k in range(32) if start + k in sites),
                sum(1 << k for k in range(32) if start + k in flagged))
        assert tuple(int(v) for v in words[b]) == want, (name, b)
    assert not words[0, 1] and not words[1 if index.lo >= 64 else 0, 1] and not words[-1, 1] and words[-1, 0] == index.n_dpos
    assert np.array_equal(index.words(3, 2), words[3:5])


# ---- the tables are what they claim ---------------------------------------------------------------------------------------------

def _known_words(name):
    """The entries of a table's buckets (of the large tables: those near a site or an end), in bucket order, with the bucket numbers."""
    _, index, _ = X.table(name)
    if name not in ("wide", X.BIG):
        return np.arange(index.n_dbuckets), index.words()
    b = np.unique(np.concatenate([np.arange(f, f + c) for f, c in X.ranges_to_read(index)]))
    return b, index.entries(b)


def test_the_case_list_holds_every_edge():
    seen = set()
    phases, bits = set(), set()
    for name in X.TABLES:
        t, index, _ = X.table(name)
        b, w = _known_words(name)
        occ, rival = w[:, 1].astype(np.int64), w[:, 2].astype(np.int64)
        if np.any(occ == 0xffffffff):
            seen.add("full")
        nxt = np.nonzero((occ[:-1] == 1 << 31) & (occ[1:] == 1) & (np.diff(b) == 1))[0]
        if len(nxt):
            seen.add("bit 31 then bit 0")
        lone = rival & ~occ
        if np.any(lone & 1):
            seen.add("flagged, no site, bit 0")
        if np.any(lone & (1 << 31)):
            seen.add("flagged, no site, bit 31")
        seen.add("dbase -64" if index.dbase == -64 else ("dbase > 0" if index.dbase > 0 else "dbase 0"))
        phases.add(index.dbase & 31)
        bits |= set(((index.D - index.dbase) & 31).tolist())
    assert {"full", "bit 31 then bit 0", "flagged, no site, bit 0", "flagged, no site, bit 31", "dbase -64", "dbase > 0"} <= seen
    assert {0, 1, 31} <= phases and len(phases) >= 4
    assert bits == ALL


@pytest.mark.parametrize("k", X.PHASES)
def test_phase_tables(k):
    t, index, _ = X.table("phase_%d" % k)
    assert index.lo == int(t.pos[0]) == X.PHASE_BASE + k and (index.lo - 64 - k) % 32 == 0
    assert index.dbase == index.lo - 64 and index.dbase & 31 == k and len(index.F)
    # the same pattern, moved: bucket for bucket the words of phase 0
    assert np.array_equal(index.words(), X.table("phase_0")[1].words())


@pytest.mark.parametrize("lo", X.LOW_LO)
def test_low_tables(lo):
    t, index, _ = X.table("low_lo_%d" % lo)
    assert index.lo == int(t.pos[0]) == lo and len(index.F)
    assert index.dbase == (-64 if lo < 64 else lo - 64)
    assert index.n_dbuckets == ((index.hi - index.dbase) >> 5) + 2


def test_full_bucket_table():
    t, index, _ = X.table("full_bucket")
    occ = index.words()[:, 1].astype(np.int64)
    full = np.nonzero(occ == 0xffffffff)[0]
    assert len(full) == 1 and occ[full[0] - 1] == 0 and occ[full[0] + 1] == 0           # 32 consecutive positions, one bucket exactly
    d = index.D
    runs = np.split(d, np.nonzero(np.diff(d) != 1)[0] + 1)
    straddle = [r for r in runs if len(r) == 33]
    assert len(straddle) == 1 and (straddle[0][0] - index.dbase) >> 5 == ((straddle[0][-1] - index.dbase) >> 5) - 1
    assert any(occ[b] == 1 << 31 and occ[b + 1] == 1 for b in range(len(occ) - 1))
    groups = np.nonzero(occ)[0]
    gaps = np.diff(groups) - 1
    assert np.all((gaps == 0) | (gaps >= 3)) and np.count_nonzero(gaps >= 3) >= 4
    assert len(index.F)


def test_multirow_table():
    t, index, _ = X.table("multirow")
    assert index.n_dpos < t.n
    counts = {}
    for p in index.D.tolist():
        rows = t.rows_at(p)
        counts.setdefault((p - index.dbase) & 31, set()).add(len(rows))
        assert len(set(t.strand[rows].tolist())) == len(rows)
    assert {2, 3} <= counts[0] and {2, 3} <= counts[31]
    assert index.words()[-1, 0] == index.n_dpos


def test_flag_not_site_table():
    t, index, _ = X.table("flag_not_site")
    loose = sorted(set(index.F.tolist()) - set(index.D.tolist()))
    assert index.lo == loose[0] < index.D[0] and index.hi == loose[-1] > index.D[-1]
    as_partner = set(int(p) for p, s in zip(t.part_pos, t.part_site) if s < 0)
    as_competitor = set(t.comp_pos.tolist())
    sites = set(index.D.tolist())
    for kind in (as_partner, as_competitor):
        assert {0, 31} <= set((p - index.dbase) & 31 for p in kind - sites if p in loose)
    w = index.words().astype(np.int64)
    lone = w[:, 2] & ~w[:, 1]
    assert np.any((lone & 1 != 0) & (w[:, 1] != 0)) and np.any((lone & 1 != 0) & (w[:, 1] == 0))      # beside sites, and in a bucket without any
    assert np.any((lone >> 31 != 0) & (w[:, 1] != 0)) and np.any((lone >> 31 != 0) & (w[:, 1] == 0))


def test_the_other_tables():
    t, index, _ = X.table("no_flags")
    assert len(index.F) == 0 and not index.words()[:, 2].any() and t.part_off[-1] > 0 and t.comp_off[-1] == 0
    t, index, _ = X.table("one_site")
    assert t.n == 1 and index.n_dpos == 1 and len(index.F) == 2
    t, index, _ = X.table("wide")
    assert index.n_dbuckets > 256 * 4096 and index.hi - index.lo >= 1 << 27 and len(index.F)
    t, index, _ = X.table("top")
    assert index.hi == int(t.pos[-1]) == X.COORD_MAX and 999000 < X.COORD_MAX - index.lo < 1001000 and index.dbase & 31 == (X.COORD_MAX - X.TOP_SPAN) & 31
    t, index, _ = X.table(X.BIG)
    assert index.lo == int(t.pos[0]) == 0 and index.hi == int(t.pos[-1]) == X.COORD_MAX and index.dbase == -64
    assert index.n_dbuckets * 12 > 800 * 10 ** 6
    covered = set()
    for f, c in X.ranges_to_read(index):
        assert 0 <= f and f + c <= index.n_dbuckets
        covered.update(range(f, f + c))
    assert {0, index.n_dbuckets - 1} <= covered and set(((np.concatenate((index.D, index.F)) - index.dbase) >> 5).tolist()) <= covered


# ---- the consumer cases look up what they name ------------------------------------------------------------------------------------

def _lookups(rec):
    """The coordinates a read of M / N ops looks up: pos - 1, then the last base of every block and intron."""
    _, p, ops = rec
    out, cur = [p - 1], p
    for ln, _ in ops:
        cur += ln
        out.append(cur - 1)
    return out


def _case(name):
    return X.consumer_case(name, X.TOP_SHIFT if name == "top" else 0)


@pytest.mark.parametrize("name", X.CONSUMER_CASES + ["top"])
def test_consumer_case_reaches_every_bit(name, oracle_lib):
    case = _case(name)
    t, index, juncs = X.table(name)
    recs = L.records(case.reads)
    assert 1000 < len(recs) < 9000
    assert all(p >= 1 and p + X._span(ops) <= X.COORD_MAX for _, p, ops in recs)
    occ = {b: int(w) for b, w in enumerate(index.words()[:, 1]) if w} if index.n_dbuckets < 100 else None
    if occ is None:                                                      # (`top`: the buckets of the pattern)
        b0 = int((index.D[1] - index.dbase) >> 5)
        occ = {b0 + b: int(w) for b, w in enumerate(index.words(b0, index.n_dbuckets - b0)[:, 1]) if w}
    full = [b for b, w in occ.items() if w == 0xffffffff]
    assert bool(full) == (name == "full_bucket")
    empty = [b for b in range(min(occ), max(occ)) if b not in occ]
    rel = lambda x: ((x - index.dbase) >> 5, (x - index.dbase) & 31)
    n_coords = {0: 2, 1: 4, 2: 6}
    for cls in (0, 1, 2):
        for f in (FLAGS_SIMPLE if cls == 0 else X.FLAGS):
            mine = [_lookups(r) for r in recs if r[0] == f and L.read_class(r[2], r[0]) == cls]
            assert mine, (name, cls, f)
            for k in range(n_coords[cls]):
                where = [rel(c[k]) for c in mine]
                assert set(bit for _, bit in where) == ALL, (name, cls, f, k)
                # bits 0 and 31 of an occupied bucket, of an empty one between sites, and of the full one
                for kind in (set(occ), set(empty), set(full)):
                    if kind:
                        assert {0, 31} <= set(bit for b, bit in where if b in kind), (name, cls, f, k)
    if full:
        s = index.start(full[0])
        simple = [(p, p + ops[0][0]) for fl, p, ops in recs if L.read_class(ops, fl) == 0]
        assert any(a > s and b <= s + 32 for a, b in simple)                                 # wholly inside the full bucket
        assert any(b - 1 == s + 31 for a, b in simple) and any(b - 1 == s + 32 for a, b in simple)
        assert any(a - 1 == s - 1 for a, b in simple) and any(a - 1 == s for a, b in simple)
    sites_, flagged = set(index.D.tolist()), set(index.F.tolist())
    spans = [(rel(p - 1)[0], rel(p + ops[0][0] - 1)[0]) for fl, p, ops in recs if L.read_class(ops, fl) == 0]
    gap = 4 if name in ("full_bucket", "phase_0", "phase_1", "phase_31", "top") else 2          # (three empty buckets in a row there)
    assert any(a in occ and b in occ and b - a >= gap and not any(x in occ for x in range(a + 1, b)) for a, b in spans)   # across the empty buckets
    # junction ends on flagged positions at bit 0 and bit 31, sites and (flag_not_site) not sites; one base off: not in the table
    table_juncs = set()
    for row in range(t.n):
        for p in t.part_pos[t.part_off[row]:t.part_off[row + 1]].tolist():
            for c in t.comp_pos[t.comp_off[row]:t.comp_off[row + 1]].tolist():
                table_juncs.add((min(p, c), max(p, c)))
    assert set(juncs) <= table_juncs
    for cls in (1, 2):
        for f in X.FLAGS:
            hit, off = set(), set()
            for r in recs:
                if r[0] != f or L.read_class(r[2], r[0]) != cls:
                    continue
                c = _lookups(r)
                for l, rr in zip(c[1::2], c[2::2]):
                    if (l, rr) in table_juncs:
                        hit.update((rel(e)[1], e in sites_) for e in (l, rr))
                    elif any((l + dl, rr + dr) in table_juncs for dl in (-1, 0, 1) for dr in (-1, 0, 1)):
                        off.update((rel(e + d)[1], e + d in sites_) for e in (l, rr) for d in (-1, 1) if e + d in flagged)
            want = {(0, True), (31, True)} | ({(0, False), (31, False)} if name == "flag_not_site" else set())
            assert want <= hit and want <= off, (name, cls, f, hit, off)
    # the general path: a soft clip, an insertion, a deletion, three introns; last blocks end on bits 0 and 31
    for need in (lambda ops: ops[0][1] == S, lambda ops: any(c == I for _, c in ops), lambda ops: any(c == D for _, c in ops),
                 lambda ops: sum(c == N for _, c in ops) == 3):
        ends = set(rel(p + X._span(ops) - 1)[1] for fl, p, ops in recs if L.read_class(ops, fl) == 3 and need(ops))
        assert {0, 31} <= ends, name
    # the clamp: a segment whose first read lies left of bucket 0, one whose first read lies right of the last bucket
    firsts = [int(rs.pos[0]) + sh for rs, sh in case.segments]
    assert any(p - 1 < index.dbase for p in firsts)
    if name != "top":
        assert any(p - 1 >= index.start(index.n_dbuckets) for p in firsts)
    else:
        assert case.segments[0][1] == X.TOP_SHIFT > (1 << 31) - (1 << 16) and case.segments[0][0].n > 1000
    X.assert_named_rows_count(oracle_lib, case)

