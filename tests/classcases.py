"""Reads at the limits of their record classes (spl_pack.h: SIMPLE len < 65536; MNM a < 65536 with d and b full words; M2 a, b, c
< 65536 with b | c << 16 in one word; every class with the read's end <= SPL_COORD_MAX), for the counting kernels, which unpack
those fields with shifts and masks of their own (read_at, the range kernel's three paths, the fused pass, the pair kernel), and in
every spelling that takes a read through another of the classifiers that must agree with classify_ops (classify_plain,
classify_fast5 / classify_clip5, classify_clipped, classify_lean).

One table: N_ROWS rows GRID bases apart on alternating strands, neighbours linked as partners, rows of their own wherever a limit
read's junction ends off the grid, a few junctions with rivals (two with more than the range kernel settles itself: their reads
go to the literal queue), alpha, edge counts and partner rows given, so that the counting pass computes SSE.  `top` has the same
table with its last grid row at SPL_COORD_MAX.

Every case states the run each read must land in, from the rule as test_pack_host.classify states it.  "End" is the coordinate
behind a read's last base (POS + the reference length), which is what the classes hold to SPL_COORD_MAX.

Shared by test_classcases_host.py (CPU) and test_gpu_class_limits.py (GPU).  No GPU and no call into the library here."""
import numpy as np

import limitcases as L
from limitcases import M, I, D, N, S, H, P, EQ, X
from test_pack_host import classify as pack_classify

COORD_MAX = L.C["SPL_COORD_MAX"]
SCAN_OPS = L.C["SPL_PACK_SCAN_OPS"]
GRID, P0, N_ROWS = 20, 1000, 3600
TOP_BASE = COORD_MAX - GRID * (N_ROWS - 1)      # the grid whose last row is SPL_COORD_MAX
TOP_SHIFT = TOP_BASE - P0                        # brings reads written against the low grid to it
LIMITS = (65534, 65535, 65536, 65537, 70000)
EDGE16 = (4095, 4096, 65535, 65536)
LONG_B = (65535, 65536, 1 << 20)
BIG_D = (1 << 28) - 1
FLAGS = (0, 16, 99, 147)
SPELLINGS = ("plain", "eqx", "clipped", "lean", "wide9")
MAX_READS = 3 * L.CHUNK_BIG
CONSUMING = (M, D, N, EQ, X)


def gpos(k, base=P0):
    return base + GRID * k


# ---- shapes: (POS, [a, d, b, ...]) -- aligned and skipped lengths in turn ---------------------------------------------------------

def junctions_of(pos, lens):
    out, cur = [], pos
    for i, ln in enumerate(lens):
        if i % 2:
            out.append((cur - 1, cur + ln - 1))
        cur += ln
    return out


def simple_shapes(base=P0):
    """One aligned block of L bases from about row 30 on, its last base on a row and one behind it (beta1 needs t and t + 1)."""
    out = []
    for lv in LIMITS:
        kend = 30 + (lv + GRID - 1) // GRID
        for e in (0, 1):
            out.append((gpos(kend, base) + e + 1 - lv, [lv]))
    return out


def once_shapes(base=P0, hi=(3560, 3565), lo=(40, 45), k_d1=50, k_dbig=60):
    """a = L before the junction of rows `hi`; a small before the junction of rows `lo` with b long; d = 1 and d = 2^28 - 1."""
    out = []
    l, r = gpos(hi[0], base), gpos(hi[1], base)
    out += [(l + 1 - lv, [lv, r - l, 30]) for lv in LIMITS]
    l, r = gpos(lo[0], base), gpos(lo[1], base)
    out += [(l + 1 - 25, [25, r - l, b]) for b in LONG_B]
    if k_d1 is not None:
        out.append((gpos(k_d1, base) + 1 - 30, [30, 1, 40]))
        out.append((gpos(k_dbig, base) + 1 - 30, [30, BIG_D, 40]))
    return out


def twice_shapes(base=P0, ka=3570, kb=100, kc=120, k_all=3300, k_big=70):
    """Each of a, b, c in turn on and beyond 12 and 16 bits, the others small; all three 65535; both introns 2^28 - 1.  The small
    lengths are whole grid steps, so the junctions of a read whose long block is a or c end on grid rows."""
    d1, bs, d2, sa, sc = 100, 40, 200, 30, 50
    out = []
    out += [(gpos(ka, base) + 1 - v, [v, d1, bs, d2, sc]) for v in EDGE16]
    out += [(gpos(kb, base) + 1 - sa, [sa, d1, v, d2, sc]) for v in EDGE16]
    out += [(gpos(kc, base) + 1 - sa, [sa, d1, bs, d2, v]) for v in EDGE16]
    if k_all is not None:
        out.append((gpos(k_all, base) + 1 - 65535, [65535, d1, 65535, d2, 65535]))
        out.append((gpos(k_big, base) + 1 - sa, [sa, BIG_D, bs, BIG_D, sc]))
    return out


# junctions with rivals: (rows of the junction's ends, rows of its rivals)
RIVALS = [((40, 45), [42, 50]), ((3560, 3565), [3562]), ((100, 105), [102, 108]), ((3577, 3587), [3580]),
          ((3500, 3505), [3502] + list(range(3506, 3506 + L.RIV_ONCE))),                                  # RIV_ONCE + 1: literal queue
          ((3527, 3537), list(range(3528, 3537)) + list(range(3538, 3538 + L.RIV_TWICE + 1 - 9))),        # RIV_TWICE + 1
          ((150, 155), list(range(156, 156 + L.RIV_TWICE + 1)))]
Q_ONCE, Q_TWICE_A, Q_TWICE_B = (3500, 3505), 3520, 150      # (twice: ka = kc = 3520 -> junctions (3520, 3525), (3527, 3537))


def queued_shapes(base=P0):
    return (simple_shapes(base), once_shapes(base, hi=Q_ONCE, lo=Q_ONCE, k_d1=None),
            twice_shapes(base, ka=Q_TWICE_A, kb=Q_TWICE_B, kc=Q_TWICE_A, k_all=None))


def top_shapes():
    """MNM and M2 shapes that end at SPL_COORD_MAX, in the coordinates of the top grid."""
    lens = [[65535, 100, 39], [30, 100, 65535], [30, 60, 39], [65535, 100, 40, 200, 39], [30, 100, 65535, 200, 39],
            [30, 100, 40, 200, 65535], [30, 100, 40, 200, 39]]
    return [(COORD_MAX - sum(x), x) for x in lens]


def _all_limit_shapes(base):
    qs, qo, qt = queued_shapes(base)
    return simple_shapes(base) + once_shapes(base) + twice_shapes(base) + qs + qo + qt


# ---- spellings ------------------------------------------------------------------------------------------------------------------

def spell(lens, which, turn=0):
    """The shape's CIGAR in one of SPELLINGS: M only; = / X; one clip op (S or H) on either side or on both; H S ... S H, or an I and
    a P inside, within SPL_PACK_SCAN_OPS ops; nine ops (WIDE as it stands).  The reference-consuming ops are the same in all."""
    cons = [(ln, N if i % 2 else M) for i, ln in enumerate(lens)]
    if which == "plain":
        return cons
    if which == "eqx":
        return [(ln, c if c == N else (EQ, X)[(i // 2 + turn) % 2]) for i, (ln, c) in enumerate(cons)]
    if which == "clipped":
        lead, trail = [[(5, S)], [(2, H)], [], [(3, H)]][turn % 4], [[(3, H)], [], [(7, S)], [(4, S)]][turn % 4]
        return lead + cons + trail
    if which == "lean":
        if len(cons) <= 3:
            return [(2, H), (4, S)] + cons + [(6, S), (1, H)]
        return [(4, S), cons[0], (2, I), cons[1], cons[2], (3, P), cons[3], cons[4]]
    assert which == "wide9"
    if len(cons) == 1:
        return [(2, H), (4, S), (1, P), (2, I), cons[0], (1, I), (1, P), (6, S), (1, H)]
    if len(cons) == 3:
        return [(2, H), (4, S), cons[0], (2, I), cons[1], (3, P), cons[2], (6, S), (1, H)]
    return [(2, H), (4, S), cons[0], (2, I), cons[1], cons[2], (3, P), cons[3], cons[4]]


def spelling_of(ops):
    """Which of SPELLINGS a CIGAR is, from its ops."""
    codes = [c for _, c in ops]
    idle = [c not in CONSUMING for c in codes]
    if len(ops) > SCAN_OPS:
        return "wide9" if len(ops) == 9 else "long"
    if not any(idle):
        return "plain" if all(c in (M, N) for c in codes) else "eqx"
    inner = idle[1:-1] if len(ops) > 1 else []
    if not any(inner) and all(c in (S, H) for c, i in zip(codes, idle) if i) and len(ops) <= 7:
        return "clipped"
    return "lean"


def consuming_lens(ops):
    return [ln for ln, c in ops if c in CONSUMING]


def shape_of(ops):
    """'A', 'ANA', 'ANANA' or None, from the reference-consuming ops."""
    s = "".join("N" if c == N else ("A" if c in (M, EQ, X) else "D") for _, c in ops if c in CONSUMING)
    return s if s in ("A", "ANA", "ANANA") else None


def declared_run(flag, pos, ops):
    return pack_classify(int(pos), int(flag), [(ln << 4) | c for ln, c in ops])[0]


def spelled(shapes, flags=FLAGS, spellings=SPELLINGS):
    """Every shape under every flag in every spelling -> records (flag, POS, ops)."""
    out = []
    for pos, lens in shapes:
        for turn, f in enumerate(flags):
            for sp in spellings:
                out.append((f, pos, spell(lens, sp, turn)))
    return out


# ---- what each family must hold, as predicates over the reference-consuming lengths ------------------------------------------------

def _small(*v):
    return all(x < 1000 for x in v)


REQUIRED = {
    "simple": [("len=%d" % v, lambda x, v=v: len(x) == 1 and x[0] == v) for v in LIMITS],
    "once_spliced": [("mnm a=%d" % v, lambda x, v=v: len(x) == 3 and x[0] == v and _small(x[1], x[2])) for v in LIMITS]
                    + [("mnm b=%d" % v, lambda x, v=v: len(x) == 3 and x[2] == v and _small(x[0])) for v in LONG_B]
                    + [("mnm d=%d" % v, lambda x, v=v: len(x) == 3 and x[1] == v) for v in (1, BIG_D)],
    "twice_spliced": [("m2 %s=%d" % ("abc"[k], v), lambda x, v=v, k=k: len(x) == 5 and x[2 * k] == v
                       and _small(*[x[2 * j] for j in range(3) if j != k])) for k in range(3) for v in EDGE16]
                     + [("a=b=c=65535", lambda x: len(x) == 5 and x[0] == x[2] == x[4] == 65535),
                        ("d1=d2=2^28-1", lambda x: len(x) == 5 and x[1] == x[3] == BIG_D)],
}
REQUIRED["queued"] = (REQUIRED["simple"] + [r for r in REQUIRED["once_spliced"] if not r[0].startswith("mnm d=")]
                      + [r for r in REQUIRED["twice_spliced"] if r[0].count("=") == 1])
REQUIRED["top"] = [("MNM a=65535", lambda x: len(x) == 3 and x[0] == 65535), ("MNM b=65535", lambda x: len(x) == 3 and x[2] == 65535),
                   ("MNM small", lambda x: len(x) == 3 and _small(*x))] + \
                  [("M2 %s=65535" % "abc"[k], lambda x, k=k: len(x) == 5 and x[2 * k] == 65535) for k in range(3)] + \
                  [("M2 small", lambda x: len(x) == 5 and _small(*x))]


# ---- the table ------------------------------------------------------------------------------------------------------------------

_TABLES = {}


def table(base=P0):
    """The grid from `base` on, with rows at the limit reads' junction ends that lie off it (the top grid: those of top_shapes),
    their ends linked as partners, and RIVALS."""
    if base in _TABLES:
        return _TABLES[base]
    tb = L.TableBuilder(base % 1000 + 5)
    row_at = {}
    for k in range(N_ROWS):
        row_at[gpos(k, base)] = tb.row(gpos(k, base), "+-"[k % 2])
    for k in range(0, N_ROWS - 1, 2):
        tb.link(k, k + 1)
    shapes = _all_limit_shapes(base) if base == P0 else top_shapes()
    linked = set()
    extra = 0
    for pos, lens in shapes:
        ends = junctions_of(pos, lens)
        last = pos + sum(lens) - 1
        for l, r in ends + ([(last - 1, None)] if len(lens) == 5 and last - 1 <= COORD_MAX else []):
            for x in (l, r):
                if x is not None and x not in row_at and x <= COORD_MAX:
                    row_at[x] = tb.row(x, "-+"[extra % 2])
                    extra += 1
            if r is not None and r in row_at and (l, r) not in linked and abs(row_at[l] - row_at[r]) != 1:
                linked.add((l, r))
                tb.link(row_at[l], row_at[r])
    if base == P0:
        for (kl, kr), riv in RIVALS:
            for t in riv:
                tb.rival(t, kl, gpos(kr, base))
    else:
        for x in (COORD_MAX - 1, COORD_MAX - 2):
            if x not in row_at:
                row_at[x] = tb.row(x, "+")
        l, r = junctions_of(*top_shapes()[2])[0]
        tb.rival(row_at[COORD_MAX - 1], row_at[l], r)           # a rival under the last block of the small MNM read
    _TABLES[base] = tb.build()
    return _TABLES[base]


# ---- the cases ------------------------------------------------------------------------------------------------------------------

def _fillers(rng, n, base=P0):
    """Ordinary short reads over the first rows: simple, once- and twice-spliced on grid junctions, one with a deletion."""
    out = []
    for _ in range(n):
        f = int(rng.choice(FLAGS))
        k = int(rng.integers(2, 70))
        kind = int(rng.integers(0, 8))
        p = gpos(k, base) - int(rng.integers(0, 30))
        if kind < 4:
            out.append((f, p, [(int(rng.integers(20, 150)), M)]))
        elif kind < 6:
            a = gpos(k, base) + 1 - p
            out.append((f, p, [(a, M), (GRID * int(rng.integers(1, 6)), N), (int(rng.integers(5, 60)), M)]))
        elif kind == 6:
            a = gpos(k, base) + 1 - p
            out.append((f, p, [(a, M), (GRID * 2, N), (GRID, M), (GRID * 3, N), (int(rng.integers(5, 60)), M)]))
        else:
            out.append((f, p, [(int(rng.integers(5, 40)), M), (2, D), (int(rng.integers(5, 40)), M)]))
    return out


def _laid_out(limit_recs, n_total, seed, base=P0):
    """The limit reads with a filler after every second one, the whole repeated up to n_total reads; every L.CHUNK-th read is a
    short read at row 2, so that the LDS window of every chunk (of either size) begins there."""
    rng = np.random.default_rng(seed)
    body = []
    for i, rec in enumerate(limit_recs):
        body.append(rec)
        if i % 2:
            body += _fillers(rng, 1, base)
    recs = (body * (n_total // len(body) + 1))[:n_total]
    for i in range(0, n_total, L.CHUNK):
        recs[i] = (0, gpos(2, base), [(50, M)])
    assert len(recs) <= MAX_READS
    return recs


def _case(name, tab, recs, limit, shift=0, **meta):
    runs = np.array([declared_run(f, p, ops) for f, p, ops in recs], np.uint8)
    seg = L.reads_from([(f, p - shift, ops) for f, p, ops in recs])
    return L.Case("class_" + name, tab, [(seg, shift)], limit, runs=runs, records=recs, **meta)


def _listed(tab, recs, runs):
    """Reads that reach the literal queue in every mode: placed flag-0x4 reads, once- / twice-spliced reads over a junction with more
    rivals than the range kernel settles (RIV_ONCE / RIV_TWICE), reads of the general path over a junction with a flagged end."""
    ends = tab.junction_ends()
    n_riv = {}
    n = 0
    for (f, p, ops), run in zip(recs, runs):
        if f & 4:
            n += 1
            continue
        cur, juncs = p, []
        for ln, c in ops:
            if c == N:
                juncs.append((cur - 1, cur + ln - 1))
            cur += ln if c in CONSUMING else 0
        for j in juncs:
            if j not in n_riv:
                n_riv[j] = len(tab.rivals(*j))
        if run == 1:
            n += n_riv[juncs[0]] > L.RIV_ONCE
        elif run == 2:
            n += any(n_riv[j] > L.RIV_TWICE for j in juncs)
        elif run == 3:
            n += any(a in ends or b in ends for a, b in juncs)
    return n


def long_reads(n, seed=11, base=P0):
    """n reads of 20 to 400 ops: M blocks of 1 to 3000 bases, I and D of 1 to 5, 2 to 15 N ops whose ends are grid rows, soft clips;
    sorted by POS."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        n_ops = 23 + int(378 * rng.random() ** 3)     # (most of them short; the loop stops within three ops of it: 20 to 400 as they stand)
        n_n = int(rng.integers(2, 16))
        cuts = np.sort(rng.choice(np.arange(2, n_ops - 6), n_n, replace=False))
        pos = gpos(0, base) + int(rng.integers(-40, 12000))
        cur, ops = pos, []
        if rng.random() < 0.5:
            ops.append((int(rng.integers(1, 30)), S))
        k = 0
        while len(ops) < n_ops - 3:
            if k < n_n and len(ops) >= cuts[k]:
                # an aligned block up to the next grid row (or some rows further), then an intron of whole grid steps
                step = (gpos(0, base) - cur) % GRID + 1 + GRID * int(rng.integers(0, 4))
                if i % 97 == 0 and k == 0:
                    step += GRID * ((3000 - step) // GRID)
                ops.append((step, M))
                cur += step
                d = GRID * int(rng.integers(1, 12))
                ops.append((d, N))
                cur += d
                k += 1
                continue
            big = rng.random() < 0.02
            ln = 3000 if i % 89 == 0 and len(ops) <= 1 else int(rng.integers(1000, 3001)) if big else int(rng.integers(1, 40))
            ops.append((ln, M))
            cur += ln
            if rng.random() < 0.5:
                ops.append((int(rng.integers(1, 6)), I))
            else:
                ln = int(rng.integers(1, 6))
                ops.append((ln, D))
                cur += ln
        ops.append((int(rng.integers(1, 60)), M))
        if rng.random() < 0.5:
            ops.append((int(rng.integers(1, 30)), S))
        # neighbouring M ops (an intron's block behind an ordinary one) are fine for every consumer: CIGARs are taken as they stand
        out.append((int(rng.choice(FLAGS)), pos, ops))
    out.sort(key=lambda r: r[1])
    return out


NAMES = ["simple", "once_spliced", "twice_spliced", "queued", "top", "long_reads"]
_CASES = {}


def case(name):
    """-> limitcases.Case with meta: runs (the declared run of every read), records, and per family what its test asserts
    (queued: n_listed; top: bad_segments, the set with the twins that end one base later)."""
    if name not in _CASES:
        _CASES[name] = _make(name)
    return _CASES[name]


def _make(name):
    tab = table()
    if name == "simple":
        recs = _laid_out(spelled(simple_shapes()), L.CHUNK_BIG + 300, 1)
        return _case(name, tab, recs, "SIMPLE len on and beyond 16 bits")
    if name == "once_spliced":
        recs = _laid_out(spelled(once_shapes()), L.CHUNK_BIG + 300, 2)
        return _case(name, tab, recs, "MNM a on and beyond 16 bits; b and d full words")
    if name == "twice_spliced":
        recs = _laid_out(spelled(twice_shapes()), L.CHUNK_BIG + 300, 3)
        return _case(name, tab, recs, "M2 a, b, c on and beyond 12 and 16 bits")
    if name == "queued":
        qs, qo, qt = queued_shapes()
        limit = spelled(qo + qt) + spelled(qs, flags=FLAGS[:2])
        limit += [(f | 4, p, ops) for f, p, ops in spelled(qs + qo + qt, flags=FLAGS[:1], spellings=SPELLINGS)]
        recs = _laid_out(limit, L.CHUNK_BIG + 300, 4)
        c = _case(name, tab, recs, "limit reads through the wave lists and the literal queue")
        c.meta["n_listed"] = _listed(tab, recs, c.meta["runs"])
        return c
    if name == "top":
        ttab = table(TOP_BASE)
        good = spelled(top_shapes())
        twins = spelled([(p, lens[:-1] + [lens[-1] + 1]) for p, lens in top_shapes()])
        rng = np.random.default_rng(5)
        fill = _fillers(rng, 600, TOP_BASE) + [(f, gpos(N_ROWS - 8, TOP_BASE) - 3 * k, [(30, M)]) for k in range(40) for f in (0, 16)]
        recs = [r for pair in zip(fill, good * 4) for r in pair]
        bad = recs[:300] + twins + recs[300:]
        c = _case(name, ttab, recs, "MNM and M2 reads that end at SPL_COORD_MAX", shift=TOP_SHIFT)
        c.meta["bad_records"] = bad
        c.meta["bad_segments"] = [(L.reads_from([(f, p - TOP_SHIFT, ops) for f, p, ops in bad]), TOP_SHIFT)]
        c.meta["twins"] = twins
        return c
    assert name == "long_reads"
    return _case(name, tab, long_reads(L.CHUNK + 100), "CIGARs of 20 to 400 ops with blocks of up to 3000 bases")


# ---- damaged fields: what a wrong decode would count ------------------------------------------------------------------------------

FIELDS = {"simple_len": ("A", 0, 0), "mnm_a": ("ANA", 1, 0), "mnm_b": ("ANA", 1, 2), "m2_a": ("ANANA", 2, 0), "m2_b": ("ANANA", 2, 2),
          "m2_c": ("ANANA", 2, 4)}
DAMAGES = [(f, d) for f in FIELDS for d in ("&0xfff", "&0x7fff", "wrap65536")] + [("mnm_b", "&0xffff"), ("m2_b", "swap_bc")]
FAMILY_FIELDS = {"simple": ["simple_len"], "once_spliced": ["mnm_a", "mnm_b"], "twice_spliced": ["m2_a", "m2_b", "m2_c"]}


def distinct(recs):
    seen, out = set(), []
    for f, p, ops in recs:
        key = (f, p, tuple(ops))
        if key not in seen:
            seen.add(key)
            out.append((f, p, list(ops)))
    return out


def damaged(recs, field, damage):
    """recs with one packed field decoded wrongly -> (records, the number of reads that changed).  A mask or a swap hits the reads
    that are packed in the field's class; 'wrap65536' is a classifier that let 65536 into the field: reads of the class's shape
    whose length there is 65536 count as if it were 0.  (mnm_b is a full word: 65536 there is a packed value, and & 0xffff is the
    decode that would lose it.)"""
    shape, run, idx = FIELDS[field]
    out, changed = [], 0
    for f, p, ops in recs:
        ops = list(ops)
        at = [i for i, (_, c) in enumerate(ops) if c in CONSUMING]
        if shape_of(ops) == shape and not f & 4:
            packed = declared_run(f, p, ops) == run
            lens = [ops[i][0] for i in at]
            new = list(lens)
            if damage == "wrap65536":
                if lens[idx] == 65536 and len(ops) <= SCAN_OPS and (packed or field != "mnm_b"):
                    new[idx] = 0
            elif packed and damage == "swap_bc":
                new[2], new[4] = lens[4], lens[2]
            elif packed:
                new[idx] = lens[idx] & int(damage[1:], 16)
            if new != lens:
                changed += 1
                for i, ln in zip(at, new):
                    ops[i] = (ln, ops[i][1])
        out.append((f, p, ops))
    return out, changed
