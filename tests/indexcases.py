"""The position index of an uploaded site table (spl_dbk: one entry per 32-base bucket counted from dbase, built on the device by
spl_build_dbuckets_kernel), written down from its definition, and site tables built to land on its edges: sites and flagged
positions on bit 0 and bit 31 of a bucket, a full bucket, every value of dbase mod 32, the switch between dbase = -64 and lo - 64,
tables of millions of buckets and tables that end at SPL_COORD_MAX.  With the reads that make every kind of consumer (the fused
range kernel's prologue, the simple-read span test, the once- and twice-spliced paths, the inline-op path) look those places up.

Shared by test_indexcases_host.py (CPU: the cases are what they claim, the yardstick agrees with brute force) and
test_gpu_site_index.py (GPU: the index read back, and the counting passes over these tables against the oracle).  No GPU and no
call into the library here."""
import numpy as np

import limitcases as L
from limitcases import M, I, D, N, S

COORD_MAX = L.C["SPL_COORD_MAX"]
FLAGS = (0, 16, 99, 147)


# ---- the yardstick ----------------------------------------------------------------------------------------------------------------

class Index(object):
    """dbase, n_dbuckets, n_dpos and the entries of any buckets, from the sorted distinct site positions D and the sorted flagged
    positions F (int64)."""

    def __init__(self, D, F):
        self.D, self.F = D, F
        both = np.concatenate((D, F))
        self.n_dpos = int(D.shape[0])
        if both.shape[0] == 0:
            self.lo = self.hi = None
            self.dbase, self.n_dbuckets = 0, 0
            return
        self.lo, self.hi = int(both.min()), int(both.max())
        self.dbase = self.lo - 64 if self.lo >= 64 else -64
        self.n_dbuckets = ((self.hi - self.dbase) >> 5) + 2

    def start(self, b):
        return self.dbase + 32 * b

    @staticmethod
    def _bits(P, starts):
        """Per start: the set {k : start + k in P, 0 <= k < 32} as a word."""
        a = np.searchsorted(P, starts, side="left")
        z = np.searchsorted(P, starts + 32, side="left")
        word = np.zeros(starts.shape[0], np.uint64)
        for k in range(int((z - a).max()) if starts.shape[0] else 0):     # the k-th member of every bucket that has one
            sel = np.nonzero(z - a > k)[0]
            word[sel] |= np.uint64(1) << (P[a[sel] + k] - starts[sel]).astype(np.uint64)
        assert not np.any(word >> np.uint64(32))
        return word.astype(np.uint32)

    def entries(self, buckets):
        """uint32[len(buckets), 3]: first, occ, rival of the buckets named."""
        starts = self.dbase + 32 * np.asarray(buckets, np.int64)
        out = np.zeros((starts.shape[0], 3), np.uint32)
        out[:, 0] = np.searchsorted(self.D, starts, side="left")
        out[:, 1] = self._bits(self.D, starts)
        out[:, 2] = self._bits(self.F, starts)
        return out

    def words(self, first=0, count=None):
        count = self.n_dbuckets - first if count is None else count
        return self.entries(np.arange(first, first + count, dtype=np.int64))


def index_of(table):
    D = np.unique(np.asarray(table.pos, np.int64))
    F = np.array(sorted(table.junction_ends()), np.int64)
    return Index(D, F)


def resolve(index, x):
    """What the kernels make of coordinate(s) x (spl_dbk_slot_of + spl_dbk_resolve_at, and the rival bit of dbk_resolve):
    -> (u = distinct positions below x, x is a site, x is flagged), arrays like x."""
    x = np.atleast_1d(np.asarray(x, np.int64))
    rel = x - index.dbase
    slot = np.clip(rel >> 5, 0, index.n_dbuckets - 1)
    e = index.entries(slot).astype(np.int64)
    bit = rel & 31
    below = e[:, 1] & ((np.int64(1) << bit) - 1)
    pop = np.zeros(x.shape[0], np.int64)
    for k in range(32):
        pop += (below >> k) & 1
    return e[:, 0] + pop, ((e[:, 1] >> bit) & 1).astype(bool), ((e[:, 2] >> bit) & 1).astype(bool)


# ---- the tables -------------------------------------------------------------------------------------------------------------------

def build_table(seed, sites, edges, flags=True):
    """sites: [(position, strands)], strands a sequence of '+', '-', '' (one row each); edges: positions (rows' or not) that the
    table's junctions with rivals run between -- consecutive edges first, then edges two apart, and so on.  Every row becomes a
    rival of such a junction that it lies outside of (so that the junction's reads can cover it: checkBam's beta1-type reads, which
    count doubles), a junction getting the next row only when the round is through; an end that is a row's position is linked as a
    partner row on even turns and named as a competitor on odd ones, an end that is no row's position is a loose partner position
    or a competitor.  Junctions that found no row that way take the row nearest to them (between their ends if need be), so that
    every edge is flagged.  Neighbouring rows are partners of each other, two pairs in three.
    -> (Table, [(l, r)] the junctions made on purpose)."""
    tb = L.TableBuilder(seed)
    rows = []
    for p, strands in sites:
        for s in strands:
            rows.append((tb.row(p, s), p))
    rows.sort(key=lambda r: r[1])
    for k in range(0, len(rows) - 1, 2):
        if k % 6 != 4 and rows[k][1] != rows[k + 1][1]:
            tb.link(rows[k][0], rows[k + 1][0])
    if not flags:
        return tb.build(), []
    edges = sorted(set(edges))
    pairs = [(edges[i], edges[i + g]) for g in range(1, len(edges)) for i in range(len(edges) - g)]
    row_at = {}
    for r, p in rows:
        row_at.setdefault(p, r)
    used = {}

    def add(turn, t, l, r):
        pp, cp = (l, r) if turn % 2 == 0 else (r, l)
        if pp in row_at and row_at[pp] != t:
            tb.partner(t, row_at[pp])
        else:
            tb.rows[t][3].append(pp)
        tb.compete(t, cp)
        used[(l, r)] = used.get((l, r), 0) + 1

    for i, (t, p) in enumerate(rows):
        for j in range(len(pairs)):
            l, r = pairs[(i + j) % len(pairs)]
            if (p < l or p > r) and min(abs(p - l), abs(p - r)) < 3000:
                add(i, t, l, r)
                break
    for g, (l, r) in enumerate(pairs[:max(len(edges) - 1, 1)]):            # the chain of consecutive edges holds every edge
        if (l, r) not in used:
            t, p = min(rows, key=lambda rp: (rp[1] in (l, r), min(abs(rp[1] - l), abs(rp[1] - r))))
            add(g, t, l, r)
    return tb.build(), sorted(used)


def _pattern(base):
    """The site pattern of the phase cases from its lowest position on, (bucket, bit) counted from that position's own bucket
    (= bucket 2 of the index where base >= 64, base on its bit 0): sites on bit 31 and on the next bucket's bit 0, a bit 31 and a bit
    0 alone, three empty buckets, and a bucket of a few bits."""
    at = lambda b, bit: base + 32 * b + bit
    sites = [(at(0, 0), "+"), (at(0, 31), "-"), (at(1, 0), "+"), (at(1, 13), "-"), (at(2, 31), "+"), (at(3, 0), "-"),
             (at(7, 5), "+"), (at(7, 17), "-"), (at(7, 30), "+"), (at(8, 31), "-"), (at(9, 0), "+"), (at(9, 1), "-"), (at(10, 20), "+")]
    edges = [at(0, 0), at(0, 31), at(1, 0), at(2, 31), at(3, 0), at(8, 31), at(9, 0), at(10, 20)]
    return sites, edges


PHASES = (0, 1, 31, 17)
PHASE_BASE = 64 + 32 * 300
LOW_LO = (0, 1, 63, 64, 65)


def phase_table(k):
    return build_table(k, *_pattern(PHASE_BASE + k))


def low_lo_table(lo):
    return build_table(100 + lo, *_pattern(lo))


def full_bucket_table(k=7):
    """From dbase = 9600 + k on: bucket 2 bit 0; bucket 6 full; 33 consecutive positions from bucket 10 bit 10 to bucket 11 bit 10;
    bucket 15 bit 31 alone, bucket 16 bit 0 alone; bucket 20 bit 15; three empty buckets between the groups."""
    at = lambda b, bit: PHASE_BASE - 64 + k + 32 * b + bit
    sites = [(at(2, 0), "+")] + [(at(6, j), "+-"[j % 2]) for j in range(32)] + [(at(10, 10) + j, "-+"[j % 2]) for j in range(33)]
    sites += [(at(15, 31), "+"), (at(16, 0), "-"), (at(20, 15), "+")]
    edges = [at(2, 0), at(6, 0), at(6, 31), at(10, 10), at(10, 31), at(11, 0), at(15, 31), at(16, 0), at(20, 15)]
    return build_table(32, sites, edges)


def multirow_table(k=5):
    """Two and three rows ('+', '-', no strand) at positions on bit 0 and bit 31."""
    at = lambda b, bit: PHASE_BASE - 64 + k + 32 * b + bit
    sites = [(at(2, 0), ("+", "-")), (at(2, 31), ("+", "-", "")), (at(3, 0), ("+", "-", "")), (at(3, 31), ("+", "")),
             (at(5, 0), ("+",)), (at(5, 9), ("-",)), (at(7, 31), ("-", "")), (at(8, 0), ("+", "-", "")), (at(9, 12), ("+", "-"))]
    edges = [at(2, 0), at(2, 31), at(3, 0), at(3, 31), at(7, 31), at(8, 0), at(9, 12)]
    return build_table(33, sites, edges)


def flag_not_site_table(k=11):
    """Junction ends that are no row's position (competitors and loose partner positions): on bit 0 and bit 31 of buckets with and
    without sites, one below the lowest site (dbase comes from it) and one above the highest (so does n_dbuckets)."""
    at = lambda b, bit: PHASE_BASE - 64 + k + 32 * b + bit
    sites = [(at(2, 9), "+"), (at(2, 31), "-"), (at(3, 0), "+"), (at(4, 31), "-"), (at(5, 0), "+"), (at(5, 16), "-"), (at(7, 5), "+"),
             (at(8, 31), "-"), (at(9, 0), "+"), (at(10, 12), "-")]
    loose = [at(2, 0), at(3, 31), at(4, 0), at(6, 0), at(6, 31), at(9, 31), at(10, 0), at(12, 3)]
    edges = loose + [at(2, 31), at(3, 0), at(8, 31), at(9, 0)]
    return build_table(34, sites, edges)


def no_flags_table():
    return build_table(35, _pattern(PHASE_BASE + 3)[0], [], flags=False)


def one_site_table():
    return build_table(36, [(5000, "+")], [4990, 5031])


def wide_table():
    """Two groups of sites 2^27 bases apart: 4.2 million buckets, most of them empty, more than 256 * 4096 of them."""
    (s0, e0), (s1, e1) = _pattern(10000 + 9), _pattern(10000 + 9 + (1 << 27))
    # (the junctions stay inside a group: each group is dressed on its own and the two are laid end to end)
    (table0, j0), (table1, j1) = build_table(37, s0, e0), build_table(38, s1, e1)
    return _concat_tables(table0, table1), j0 + j1


def _concat_tables(a, b):
    return L.Table(np.concatenate((a.pos, b.pos)), np.concatenate((a.strand, b.strand)),
                   np.concatenate((a.part_off, b.part_off[1:] + a.part_off[-1])), np.concatenate((a.part_pos, b.part_pos)),
                   np.concatenate((a.part_site, np.where(b.part_site >= 0, b.part_site + a.n, -1))),
                   np.concatenate((a.comp_off, b.comp_off[1:] + a.comp_off[-1])), np.concatenate((a.comp_pos, b.comp_pos)),
                   np.concatenate((a.alpha, b.alpha)), np.concatenate((a.edge_cnt, b.edge_cnt)))


TOP_SPAN = 32 * 10 + 20         # the pattern's highest position above its lowest


def top_table():
    """The pattern with its highest site at SPL_COORD_MAX and a row a million bases (31 250 buckets) below its lowest, so that the
    pattern's sites lie on the bits they lie on in phase_0."""
    base = COORD_MAX - TOP_SPAN
    sites, edges = _pattern(base)
    assert max(p for p, _ in sites) == COORD_MAX
    return build_table(39, [(base - 1000000, "+")] + sites, [base - 1000000 + 40] + edges)


def top_both_ends_table():
    """Sites at 0 and at SPL_COORD_MAX in one table: 67 million buckets."""
    lo_sites, lo_edges = _pattern(0)
    hi_sites, hi_edges = _pattern(COORD_MAX - TOP_SPAN)
    (a, ja), (b, jb) = build_table(40, lo_sites, lo_edges), build_table(41, hi_sites, hi_edges)
    return _concat_tables(a, b), ja + jb


TABLES = dict([("phase_%d" % k, lambda k=k: phase_table(k)) for k in PHASES] + [("low_lo_%d" % lo, lambda lo=lo: low_lo_table(lo)) for lo in LOW_LO]
              + [("full_bucket", full_bucket_table), ("multirow", multirow_table), ("flag_not_site", flag_not_site_table),
                 ("no_flags", no_flags_table), ("one_site", one_site_table), ("wide", wide_table), ("top", top_table),
                 ("top_both_ends", top_both_ends_table)])
BIG = "top_both_ends"            # read back in ranges only
_MADE = {}


def table(name):
    """-> (Table, Index, the junctions made on purpose); made once."""
    if name not in _MADE:
        t, juncs = TABLES[name]()
        _MADE[name] = (t, index_of(t), juncs)
    return _MADE[name]


def ranges_to_read(index, around=32, ends=4096):
    """[(first bucket, count)] for a table too large to read back whole: the first and the last `ends` buckets and 2 * around
    buckets about every site and flagged position."""
    n = index.n_dbuckets
    out = [(0, min(ends, n)), (max(n - ends, 0), min(ends, n))]
    for b in sorted(set(((np.concatenate((index.D, index.F)) - index.dbase) >> 5).tolist())):
        first = max(b - around, 0)
        out.append((first, min(2 * around, n - first)))
    return out


# ---- the reads ----------------------------------------------------------------------------------------------------------------

def _span(ops):
    return sum(ln for ln, c in ops if c in (M, D, N, L.EQ, L.X))


def index_reads(t, index, juncs):
    """Reads in the table's own coordinates, as records (flag, pos, ops).  A read looks up pos - 1 and the last base of every block
    and intron (c - 1); a shape moved base by base over a bucket puts each of those on every bit of it.
      simple reads: 5M and 40M moved over every occupied bucket and two empty ones; reads that begin and end on the first and the
        last base of a bucket of 32 sites, one in front of them and one behind, inside that bucket and across it; reads from each
        group of sites to the next, over the empty buckets;
      once- and twice-spliced reads, all four flags: 2M34N3M and 2M33N3M35N2M moved over the first occupied bucket (of every group
        of sites), a full one and an empty one, so far that each of their coordinates passes over the whole bucket; the table's
        own junctions (l, r) -- both ends flagged -- with first blocks of 1 and 33 bases and from each rival in front on, second
        blocks of 2 and 45 bases and up to each rival behind; the same with an end one base off (not in the junction table: one
        end still flagged, or none); pairs of the junctions as twice-spliced reads;
      the general path: a soft clip, an insertion, a deletion and three introns, their last block ending on bit 0 and bit 31."""
    recs = []
    occ_buckets = sorted(set(((index.D - index.dbase) >> 5).tolist()))
    full = [b for b in occ_buckets if index.entries([b])[0, 1] == 0xffffffff]
    groups = np.split(np.array(occ_buckets), np.nonzero(np.diff(occ_buckets) > 100)[0] + 1)          # (`top`: a lone row far below the rest)
    empty = [b for b in range(int(groups[-1][0]), occ_buckets[-1]) if b not in occ_buckets][:2]
    moves = range(-6, 33)

    def put(flag, x0, ops):
        """A read whose pos - 1 is x0, if it lies in the coordinate space."""
        if x0 + 1 >= 1 and x0 + 1 + _span(ops) <= COORD_MAX:
            recs.append((flag, x0 + 1, ops))

    for b in occ_buckets + empty:
        for mv in moves:
            for ln in (5, 40):
                for f in (0, 16):
                    put(f, index.start(b) + mv, [(ln, M)])
    for b in full:
        s = index.start(b)
        for f in (0, 16):
            for x0, ln in ((s - 1, 32), (s - 1, 33), (s - 1, 34), (s, 31), (s, 32), (s, 33), (s + 1, 30), (s + 1, 31), (s + 30, 2),
                           (s + 30, 3), (s - 33, 34), (s - 33, 65), (s - 33, 66), (s - 33, 100)):
                put(f, x0, [(ln, M)])
    for a, z in zip(occ_buckets[:-1], occ_buckets[1:]):
        if z - a > 1 and z - a < 1000:
            for f in (0, 16):
                put(f, index.start(a) + 20, [(32 * (z - a) + 30, M)])
                put(f, index.start(a) + 31, [(32 * (z - a) - 30, M)])
    anchors = sorted(set([int(g[0]) for g in groups] + full[:1] + empty[:1]))
    shapes = ([(2, M), (34, N), (3, M)], [(2, M), (33, N), (3, M), (35, N), (2, M)])
    for b in anchors:
        for ops in shapes:
            # from the read's last base on the bucket's bit 0 to its pos - 1 on bit 31: every coordinate passes over the whole bucket
            for mv in range(ops[0][0] - _span(ops) - 1, ops[0][0] + 33):
                for f in FLAGS:
                    put(f, index.start(b) + mv - ops[0][0], ops)     # (the first block's last base on the bucket's start + mv)
    rivals = {}
    for l, r in juncs:
        rivals[(l, r)] = sorted(int(t.pos[row]) for row in t.rivals(l, r))
    for (l, r), riv in sorted(rivals.items()):
        if r - l >= 1 << 28:
            continue
        firsts = sorted({1, 33} | {l + 1 - p for p in riv if 0 < l - p < 3000})
        seconds = sorted({2, 45} | {p + 1 - r for p in riv if 0 < p - r < 3000})
        for f in FLAGS:
            for m0 in firsts:
                put(f, l - m0, [(m0, M), (r - l, N), (45, M)])
            for m1 in seconds:
                put(f, l - 33, [(33, M), (r - l, N), (m1, M)])
            for dl, dr in ((1, 0), (0, -1), (-1, 1), (-1, 0), (0, 1)):
                if r + dr - l - dl > 0:
                    put(f, l + dl - 20, [(20, M), (r + dr - l - dl, N), (30, M)])
    js = sorted(rivals)
    n_twice = 0
    for (l1, r1) in js:
        for (l2, r2) in js:
            if 0 < l2 - r1 < 4000 and r1 - l1 < 1 << 28 and r2 - l2 < 1 << 28 and n_twice < 40:
                n_twice += 1
                for f in FLAGS:
                    for m0, m2 in ((1, 2), (20, 45)):
                        put(f, l1 - m0, [(m0, M), (r1 - l1, N), (l2 - r1, M), (r2 - l2, N), (m2, M)])
                    put(f, l1 - 7, [(7, M), (r1 - l1, N), (l2 + 1 - r1, M), (r2 - l2 - 1, N), (11, M)])   # the second junction one off
    general = ([(3, S), (40, M)], [(10, M), (2, I), (25, M)], [(10, M), (3, D), (25, M)], [(4, S), (12, M), (3, D), (6, M), (1, I), (9, M), (5, S)],
               [(8, M), (40, N), (8, M), (40, N), (8, M), (40, N), (14, M)])
    for b in anchors:
        for k, ops in enumerate(general):
            for bit in (0, 31):
                for f in FLAGS[k % 2::2]:
                    put(f, index.start(b) + bit - _span(ops), ops)
    return recs


def consumer_case(name, shift=0):
    """The reads of index_reads over table `name` as a limitcases.Case: sorted by position in one segment; then a segment whose
    first read lies left of the index's bucket 0 and one whose first read lies right of its last bucket (the clamp; where the
    coordinate space has room for them), each followed by every seventh read of the first.  shift: the segments hold the reads'
    positions less `shift` and are added with it; reads that would then begin below 1 form segments that are added as they are."""
    t, index, juncs = table(name)
    recs = sorted(index_reads(t, index, juncs), key=lambda r: r[1])
    near = [r for r in recs if r[1] - shift >= 1]
    far = [r for r in recs if r[1] - shift < 1]          # (a table wider than the shift's room: those reads go unshifted)
    segments = [(near, shift)]
    firsts = [(0, index.dbase - 5000)]
    if index.start(index.n_dbuckets) + 5000 + 50 <= COORD_MAX:
        firsts.append((16, index.start(index.n_dbuckets) + 5000))
    for f, p in firsts:
        sh = shift if p - shift >= 1 else 0
        if p - sh >= 1:
            segments.append(([(f, p, [(50, M)])] + (near if sh == shift else recs)[::7], sh))
    if far:
        segments.append((far, 0))
    segments = [(L.reads_from([(f, p - sh, ops) for f, p, ops in rs]), sh) for rs, sh in segments]
    named = sorted(set(int(p) for p in t.pos if ((int(p) - index.dbase) & 31) in (0, 31)
                       or index.entries([(int(p) - index.dbase) >> 5])[0, 1] == 0xffffffff))
    return L.Case("index_" + name, t, segments, "position index: " + name, named=named)


def assert_named_rows_count(oracle_lib, case):
    """The case exercises what it names: on the oracle's unstranded result, beta1, beta2Simple's reads and the double counts are
    each non-zero on every row on bit 0, on bit 31 and inside a full bucket."""
    t, r = case.table, case.reads
    b1, b2, dbl = oracle_lib.check_bam(t.pos, t.strand, t.part_off, t.part_pos, t.comp_off, t.comp_pos, r.pos, r.flag, r.cig_off, r.cigar, 0, 0)
    assert case.meta["named"]
    for p in case.meta["named"]:
        for row in t.rows_at(p):
            assert b1[row] > 0 and b2[row] > 0 and dbl[t.part_off[row]:t.part_off[row + 1]].sum() > 0, (case.name, p, row)


CONSUMER_CASES = ["full_bucket", "multirow", "flag_not_site", "phase_0", "phase_1", "phase_31"]
TOP_SHIFT = COORD_MAX - TOP_SPAN - 20000      # brings reads around 20 000 to the sites of `top`
