"""Read sets built to land on the junction table's limits (spl_junction_kernel / spl_junction_compact_kernel in spl_kernels.hip,
spl_junctions in spl_capi.cpp): every packed record class carrying N ops, the -a / -m / -M filters one below, on and one above
the values in the reads, keys that meet in one wave in different rounds with their largest anchors on lanes other than the
leader, one junction in more than 65 535 reads over many chunks, keys that collide in the open-addressing table and run past its
last slot, the same (left, right) on both strands, coordinates at 2^30 and at SPL_COORD_MAX.  Shared by
test_gpu_junction_limits.py (GPU against oracle.junction_table) and test_junction_cases_host.py (CPU checks that every case
reaches the limit it names).

The constants come from the kernel sources, as in limitcases.py, so the cases follow the code when one is retuned."""
import os
import re

import numpy as np

from limitcases import CSRC, D, EQ, H, I, M, N, P, S, X, _header_constants, reads_from, records
from spliser_amd import native, samio

C = _header_constants()
CHUNK, CHUNK_BIG = C["SPL_CHUNK"], C["SPL_CHUNK_BIG"]
NOPS_SAT = C["SPL_NOPS_SAT"]
COORD_MAX = C["SPL_COORD_MAX"]
RC_WIDE = C["SPL_RC_WIDE"]
RC_SHIFT = C["SPL_RC_SHIFT"]


def _source(name):
    with open(os.path.join(CSRC, name)) as fh:
        return fh.read()


def _one(pattern, text):
    found = set(re.findall(pattern, text))
    assert len(found) == 1, (pattern, found)
    return found.pop()


_KERNELS, _CAPI = _source("spl_kernels.hip"), _source("spl_capi.cpp")
S_OPS_ROW = int(_one(r"s_ops\[\w+\]\[(\d+)\]", _KERNELS))              # the words a lane's rebuilt short CIGAR may use
HASH = int(_one(r"kk \* (0x[0-9A-Fa-f]+)ull >> 32", _KERNELS), 16)       # the table's multiplicative hash
MIN_SLOTS = int(_one(r"uint64_t slots = (\d+);", _CAPI))                # the smallest table spl_junctions makes
LANES = 64                                                              # a wave (the kernel's ballots are 64-bit)
_MASK64 = (1 << 64) - 1


# ---- the table's slot arithmetic, restated -------------------------------------------------------------------------------------

def n_slots(n_ops):
    """Slots of the table spl_junctions makes for a set of n_ops CIGAR ops: MIN_SLOTS or the next power of two >= n_ops."""
    s = MIN_SLOTS
    while s < n_ops:
        s <<= 1
    return s


def key_of(l, r, minus=False):
    """The kernel's 64-bit key: (l << 32) | (r << 1) | strand bit (1 = read strand '-' in a stranded run)."""
    return (((l & 0xffffffff) << 32) | ((r & 0xffffffff) << 1) | int(bool(minus))) & _MASK64


def home(key, mask):
    """The first slot the insert of `key` tries: the high half of (key * HASH mod 2^64), masked."""
    return (((key * HASH) & _MASK64) >> 32) & mask


def place(keys, slots):
    """Linear probing as the kernel does it, (home + i) & mask, inserting in the order given -> {key: slot}.  (The slots a set of
    keys ends up in does not depend on the order of the inserts; which key sits where does.)"""
    mask = slots - 1
    table, out = {}, {}
    for k in keys:
        if k in out:
            continue
        for i in range(slots):
            s = (home(k, mask) + i) & mask
            if s not in table:
                table[s] = k
                out[k] = s
                break
        else:
            raise AssertionError("table full")
    return out


# ---- what a read carries ------------------------------------------------------------------------------------------------------

_ADV = (M, D, N, EQ, X)


def junctions_of(rec):
    """[(l, r, d, anchor_left, anchor_right)] of every N op of a placed, mapped read (oracle.junction_table's walk)."""
    flag, p, ops = rec
    if flag & 4 or p < 0:
        return []
    out, cur, before = [], p, 0
    for k, (ln, code) in enumerate(ops):
        if code not in _ADV:
            continue
        cur += ln
        if code != N:
            before += ln
            continue
        after = 0
        for ln2, c2 in ops[k + 1:]:
            if c2 == N:
                break
            if c2 in _ADV:
                after += ln2
        out.append((cur - ln - 1, cur - 1, ln, before, after))
        before = 0
    return out


def passes(j, a, m, mx):
    _, _, d, al, ar = j
    return al >= a and ar >= a and d >= m and (mx == 0 or d <= mx)


def read_minus(flag, stranded):
    """check_strand's read strand (SpliSER_v0_1_8.py:374-406) is '-'."""
    if not stranded:
        return False
    first = bool(flag & 64) or not (flag & 1)
    rev = bool(flag & 16)
    plus = (first != rev) if stranded == 1 else (first == rev)
    return not plus


def packed_run(rec):
    """(run, wide) of one read as the host packer files it (spl_pack_host on a set of that read alone): run 0 SIMPLE, 1 MNM,
    2 M2, 3 OTHER; wide for an OTHER record whose ops live in the wide array.  (Asked of the packer itself rather than restated:
    limitcases.read_class files twice-spliced reads with blocks of 2^12 and more as OTHER, the host packer keeps them M2 up to
    2^16.)"""
    rs = reads_from([rec])
    desc, rec_blob, _ = native.pack_host(native.ReadArrays(rs.pos, rs.flag, rs.cig_off, rs.cigar))
    n = desc[0]["n"].tolist()
    run = n.index(1)
    wide = False
    if run == 3:
        w1 = int(np.frombuffer(rec_blob[4:8].tobytes(), np.uint32)[0])
        wide = (w1 >> RC_SHIFT) == RC_WIDE
    return run, wide


def slot_order(recs, chunk):
    """Per read: (chunk, slot) -- the slot is its place in the chunk's record runs (reads stably partitioned by run)."""
    runs = [packed_run(r)[0] for r in recs]
    out = [None] * len(recs)
    for c0 in range(0, len(recs), chunk):
        idx = list(range(c0, min(c0 + chunk, len(recs))))
        for s, i in enumerate(sorted(idx, key=lambda i: runs[i])):
            out[i] = (c0 // chunk, s)
    return out


def wave_groups(recs, chunk, stranded=0, a=0, m=0, mx=0):
    """The kernel's merge, restated: in round q of a wave's outer loop every lane holds its q-th N op that passes the filter; the
    lanes holding the same key form a group, its leader the lowest such lane.  -> [{key, wave, round, leader, lanes: {lane:
    (anchor_left, anchor_right)}}]."""
    where = slot_order(recs, chunk)
    per_wave = {}
    for i, rec in enumerate(recs):
        ch, s = where[i]
        lane_js = [j for j in junctions_of(rec) if passes(j, a, m, mx)]
        per_wave.setdefault((ch, s // LANES), {})[s % LANES] = [(key_of(j[0], j[1], read_minus(rec[0], stranded)), j[3], j[4]) for j in lane_js]
    out = []
    for wave, lanes in sorted(per_wave.items()):
        for q in range(max(len(v) for v in lanes.values()) if lanes else 0):
            groups = {}
            for lane in sorted(lanes):
                if q < len(lanes[lane]):
                    k, al, ar = lanes[lane][q]
                    groups.setdefault(k, {})[lane] = (al, ar)
            for k, g in groups.items():
                out.append(dict(key=k, wave=wave, round=q, leader=min(g), lanes=g))
    return out


# ---- cases --------------------------------------------------------------------------------------------------------------------

class JCase(object):
    """Read segments [(ReadSet, shift)] and the filter settings [(min_anchor, min_intron, max_intron)] to run them with."""

    def __init__(self, name, segments, filters, limit, **meta):
        self.name, self.segments, self.filters, self.limit, self.meta = name, segments, filters, limit, meta
        recs = []
        for rs, shift in segments:
            recs += [(f, p + shift, ops) for f, p, ops in records(rs)]
        self.recs = recs
        self.reads = reads_from(recs) if recs else samio.ReadSet.empty()

    def want(self, stranded, a, m, mx):
        from oracle import oracle
        r = self.reads
        return oracle.junction_table(r.pos, r.flag, r.cig_off, r.cigar, stranded, a, m, mx)


NO_FILTER = [(0, 0, 0)]
DEFAULTS = (8, 70, 500000)          # regtools' -a / -m / -M, the `junctions` command's defaults


def record_classes_case():
    """Every record class with N ops in it: MNM and M2 with blocks on the packers' limits and one past them, OTHER-narrow (at most
    three reference ops, non-consuming ones dropped), OTHER-wide with I/S/H/P/D/=/X around the N ops, a read of more ops than the
    packed op count holds, and records that must carry nothing: unmapped (0x4) with N ops, '*' CIGARs, SIMPLE reads."""
    base = 100000
    recs = [
        (0, base, [(100, M)]),                                                            # SIMPLE
        (0, base - 60, [(60, M), (400, N), (40, M)]),                                      # MNM
        (16, base - (1 << 16) + 1, [((1 << 16) - 1, M), (400, N), (40, M)]),               # MNM, first block at its limit
        (0, base - (1 << 16), [(1 << 16, M), (400, N), (40, M)]),                          # ... one past it: OTHER
        (0, base - 60, [(60, M), (400, N), ((1 << 16) + 7, M)]),                           # MNM, a long last block
        (0, base - 30, [(30, M), (400, N), (50, M), (300, N), (20, M)]),                  # M2
        (0, base - 4095, [(4095, M), (400, N), (4095, M), (300, N), (4095, M)]),           # M2, blocks of 2^12 - 1
        (0, base - 4096, [(4096, M), (400, N), (4096, M), (300, N), (4096, M)]),           # ... of 2^12
        (0, base - 65535, [(65535, M), (400, N), (65535, M), (300, N), (65535, M)]),       # ... of 2^16 - 1
        (16, base - 65536, [(65536, M), (400, N), (50, M), (300, N), (20, M)]),            # ... one past: OTHER
        (0, base - 30, [(30, M), (400, N), (50, M), (300, N), (60, M), (200, N), (10, M)]),  # three N ops: OTHER-wide
        (0, base + 1, [(400, N), (30, M)]),                                                # OTHER-narrow: N first
        (0, base - 30, [(30, M), (400, N)]),                                               # ... N last
        (0, base - 30, [(30, M), (400, N), (5, D)]),                                       # ... M N D
        (0, base - 30, [(7, S), (30, M), (400, N), (2, I), (5, D), (3, H)]),               # narrow after the clips go
        (16, base - 30, [(4, H), (6, S), (10, EQ), (1, X), (19, M), (400, N), (8, EQ), (3, I), (2, D), (1, P), (30, X), (5, S)]),
        (0, base - 30, [(30, M), (2, I), (400, N), (1, P), (40, M), (3, D), (300, N), (6, S)]),
        (0, base - 30, [(30, M), (4, D), (400, N), (40, M)]),                              # a deletion in the left anchor
        (4, base - 60, [(60, M), (400, N), (40, M)]),                                      # unmapped with an N op: nothing
        (4, base - 60, [(60, M), (400, N), (40, M), (300, N), (20, M)]),
        (0, base + 5, []),                                                                 # '*'
        (20, base + 5, []),
    ]
    # more ops than the packed op count holds: 1M 1N ... with the N ops in runs of junctions one base apart
    many = []
    for k in range(NOPS_SAT // 2 + 50):
        many += [(1 + k % 3, M), (1 + k % 5, N)]
    many.append((25, M))
    recs.append((0, base + 2000, many))
    recs.append((16, base + 2000, many[:-3] + [(9, M)]))
    return JCase("record_classes", [(reads_from(recs), 0)], NO_FILTER + [(1, 1, 0), (8, 70, 500000), (3, 2, 4)],
                 "every record class with N ops", n_ops_long=len(many))


def filter_boundaries_case():
    """Anchors A1 = 10 / A2 = 12 and intron D = 100 with -a / -m / -M one below, on and one above; 0N ops; anchors of 0 (an N op
    at the read's start or end, adjacent N ops); reads whose first N op passes and the next fails; one whose failed N op must
    still end the next op's left anchor (the kernel resets it after every N op); N ops at the first bases: left = 0 and -1."""
    A1, A2, Dn = 10, 12, 100
    L0 = 50000
    recs = [
        (0, L0 + 1 - A1, [(A1, M), (Dn, N), (A2, M)]),
        (16, L0 + 1 - A2, [(A2, M), (Dn, N), (A1, M)]),                                   # the same junction, anchors swapped
        (0, L0 + 1 - A1, [(A1, M), (Dn - 1, N), (A2, M)]),
        (0, L0 + 1 - A1, [(A1, M), (Dn + 1, N), (A2, M)]),
        (0, L0 + 1001 - 20, [(20, M), (0, N), (20, M)]),                                   # 0N
        (0, L0 + 2001 - 20, [(20, M), (Dn, N), (0, M), (Dn, N), (20, M)]),                 # an empty block between two N ops
        (0, L0 + 3001 - 20, [(20, M), (Dn, N), (Dn + 1, N), (20, M)]),                     # adjacent N ops
        (0, L0 + 4001, [(Dn, N), (30, M)]),                                                # N op first: left anchor 0
        (0, L0 + 5001 - 30, [(30, M), (Dn, N)]),                                           # N op last: right anchor 0
        (0, L0 + 6001 - A2, [(A2, M), (Dn, N), (A1, M), (50, N), (A2, M)]),               # passes -m 70, the next one fails
        (0, L0 + 7001 - 20, [(20, M), (50, N), (3, M), (Dn, N), (20, M)]),                # -m 70 -a 5: the second one's left anchor is 3
        (0, L0 + 8001 - A1, [(A1 - 4, M), (2, D), (4, M), (Dn, N), (5, EQ), (A2 - 5, X)]),  # anchors of several ops
        (0, L0 + 9001 - 15, [(15, M), (5 * Dn, N), (15, M)]),                              # longer than every -M below
        (0, 1, [(30, N), (20, M)]),                                                        # N op at POS 1: left = 0
        (0, 0, [(30, N), (20, M)]),                                                        # POS 0 (host arrays only: unplaced in a
        (0, 0, [(5, M), (30, N), (20, M)]),                                                # BAM file): left = -1
    ]
    filters = [(a, 0, 0) for a in (0, 1, A1 - 1, A1, A1 + 1, A2 - 1, A2, A2 + 1)]
    filters += [(0, m, 0) for m in (1, Dn - 1, Dn, Dn + 1)]
    filters += [(0, 0, mx) for mx in (Dn - 1, Dn, Dn + 1)]
    filters += [(0, Dn, Dn), (A1, Dn, Dn), (A2, Dn, Dn + 1), (5, 70, 0), DEFAULTS]
    return JCase("filter_boundaries", [(reads_from(recs * 3), 0)], filters, "-a / -m / -M at the reads' values", anchors=(A1, A2),
                 intron=Dn)


def wave_merge_case():
    """Wave 0 of chunk 0: 64 reads with three N ops each (OTHER-wide records, so their slots are their places in the file).  All
    carry J = (L, R); on even lanes it is the third N op (round 2 of the kernel's loop), on odd lanes the first (round 0).  Lane 1
    leads J's round-0 group with the smallest anchors; lane 17 holds the largest left anchor and lane 41 the largest right anchor,
    both of the whole set.  Then a second wave of the same reads the other way round, its anchors below those maxima."""
    L, R = 200000, 200500
    D1, D2 = 120, 80

    def first(al, ar):      # J first, two more N ops after it
        return (0, L + 1 - al, [(al, M), (R - L, N), (ar, M), (D1, N), (20, M), (D2, N), (15, M)])

    def third(al, ar):      # two N ops in front, J third
        return (16, L + 1 - al - D2 - 30 - D1 - 25, [(25, M), (D1, N), (30, M), (D2, N), (al, M), (R - L, N), (ar, M)])
    recs = []
    for lane in range(LANES):
        al, ar = 20 + lane % 7, 30 + lane % 5
        if lane == 1:
            al, ar = 5, 5                       # the round-0 leader: the smallest anchors of its group
        if lane == 17:
            al = 90                             # the largest left anchor
        if lane == 41:
            ar = 95                             # the largest right anchor
        if lane == 0:
            al, ar = 6, 6                       # the round-2 leader
        recs.append(third(al, ar) if lane % 2 == 0 else first(al, ar))
    for lane in range(LANES):                   # wave 1: J third on odd lanes, first on even ones, anchors below the maxima
        al, ar = 40 + lane % 11, 50 + lane % 13
        recs.append(third(al, ar) if lane % 2 else first(al, ar))
    return JCase("wave_merge", [(reads_from(recs), 0)], NO_FILTER + [(6, 0, 0), (21, 100, 0)], "one key in several rounds of a wave",
                 junction=(L, R), max_left=(17, 90), max_right=(41, 95))


def many_chunks_case(n=65536 + 3 * CHUNK_BIG):
    """One junction in n reads (more than 65 535, over many chunks of either size); the largest left anchor in one read of an early
    chunk, the largest right anchor in one read of a late chunk, everything else smaller.  A few other junctions between them."""
    L, R = 300000, 300800
    rng = np.random.default_rng(11)
    al = rng.integers(8, 60, n)
    ar = rng.integers(8, 60, n)
    i_left, i_right = 3 * CHUNK + 17, n - 2 * CHUNK - 5
    al[i_left] = 150
    ar[i_right] = 170
    # 0, 99 and 147 are all the same read strand ('+' for fr, '-' for rf): the count stays above 65 535 in stranded runs too
    flags = rng.choice(np.array([0, 99, 147], np.uint16), n)
    recs = []
    for i in range(n):
        if i % 997 == 0:                        # a few other junctions between them
            recs.append((16, L - 500, [(40, M), (100 + i % 7, N), (40, M)]))
        recs.append((int(flags[i]), L + 1 - int(al[i]), [(int(al[i]), M), (R - L, N), (int(ar[i]), M)]))
    return JCase("many_chunks", [(reads_from(recs), 0)], NO_FILTER + [(60, 0, 0)], "one junction in %d reads" % n,
                 junction=(L, R), n_same=n, max_left=150, max_right=170)


def _colliding(n_keys, target, mask, l0):
    """n_keys distinct (l, r) with home slot `target` (strand bit 0)."""
    out = []
    l = l0
    while len(out) < n_keys:
        ls = np.arange(l, l + 4096, dtype=np.uint64)
        for d in (150, 151, 152):
            keys = (ls << np.uint64(32)) | ((ls + np.uint64(d)) << np.uint64(1))
            with np.errstate(over="ignore"):
                h = ((keys * np.uint64(HASH)) >> np.uint64(32)) & np.uint64(mask)
            for x in ls[h == target].tolist():
                if len(out) < n_keys:
                    out.append((int(x), int(x) + d))
        l += 4096
    return out


def hash_case():
    """A set small enough for the smallest table: 45 distinct junctions whose home is slot mask - 9 (so the probe runs past the last
    slot to slot 0 and on), 4 more whose home is slot 1 (they meet the wrapped run), each junction in a few reads; and one (l, r)
    on both strands, paired 99/147/83/163 and unpaired 0/16, for the stranded runs."""
    mask = MIN_SLOTS - 1
    hot = _colliding(45, mask - 9, mask, 400000)
    low = _colliding(4, 1, mask, max(hot)[0] + 5000)
    recs = []
    for k, (l, r) in enumerate(sorted(hot + low)):
        for f in (0, 99):
            recs.append((f, l + 1 - 30, [(30, M), (r - l, N), (20 + k % 9, M)]))
    Lb, Rb = max(low)[0] + 10000, max(low)[0] + 10300
    for f in (0, 16, 99, 147, 83, 163):
        recs.append((f, Lb + 1 - 25, [(25, M), (Rb - Lb, N), (25 + f % 7, M)]))
    rs = reads_from(recs)
    assert int(rs.cig_off[-1]) <= MIN_SLOTS
    return JCase("hash", [(rs, 0)], NO_FILTER + [(25, 0, 0)], "collisions and the wrap at mask", hot=hot, low=low, both=(Lb, Rb),
                 mask=mask)


def coordinates_case():
    """Junctions with left / right around 2^30 (the key's bit 31 of r << 1) and as high as the shard space allows: reads that end
    exactly at SPL_COORD_MAX (allowed), with the N op in the middle and at the end."""
    G = 1 << 30
    recs = [
        (0, G - 50, [(50, M), (100, N), (50, M)]),                   # l = 2^30 - 1
        (16, G - 49, [(49, M), (100, N), (50, M)]),                  # l = 2^30 - 1 as well, other strand
        (0, G - 150, [(50, M), (100, N), (50, M)]),                  # r = 2^30 - 1
        (0, G - 151, [(50, M), (101, N), (50, M)]),                  # r = 2^30 - 1, another l
        (0, G + 7, [(50, M), (300, N), (20, M)]),
        (0, COORD_MAX - 150, [(50, M), (50, N), (50, M)]),           # ends at SPL_COORD_MAX
        (16, COORD_MAX - 100, [(50, M), (50, N)]),                   # ... with the N op last: r = SPL_COORD_MAX - 1
        (0, COORD_MAX - 200, [(40, M), (10, N), (50, M), (50, N), (50, M)]),
        (0, COORD_MAX - 64 - 30, [(30, M), (34, N), (30, M)]),
    ]
    return JCase("coordinates", [(reads_from(recs), 0)], NO_FILTER + [(50, 50, 0)], "left / right near 2^30 and SPL_COORD_MAX")


def shifted_case():
    """Three segments with non-zero shifts (begin_reads + add): the table comes back in the moved coordinates."""
    segs = []
    for k, shift in enumerate((1000, 70000, 1 << 29)):
        recs = [(f, 500 + 13 * i, [(20 + i % 9, M), (100 + 10 * (i % 4), N), (25 + i % 6, M)]) for i in range(300) for f in (0, 147)]
        recs.append((0, 400, [(5, S), (30, M), (50, N), (2, I), (40, M), (60, N), (10, M)]))
        segs.append((reads_from(recs), shift))
    return JCase("shifted_segments", segs, NO_FILTER + [(22, 101, 120)], "segments moved by their shifts")


def empty_cases():
    unmapped = reads_from([(4, 100, [(30, M), (100, N), (30, M)]), (4, 200, []), (20, 300, [(10, M), (5, N), (10, M)])])
    return [JCase("empty", [(samio.ReadSet.empty(), 0)], NO_FILTER, "no reads"),
            JCase("only_unmapped", [(unmapped, 0)], NO_FILTER, "only flag 0x4 reads")]


def beyond_coord_max():
    """A read that ends one base past SPL_COORD_MAX (an N op in it): spl_junctions must refuse the set with SPL_ERR_RANGE."""
    return reads_from([(0, 5000, [(20, M), (100, N), (20, M)]), (0, COORD_MAX - 150, [(50, M), (50, N), (51, M)])])


def all_cases():
    return [record_classes_case(), filter_boundaries_case(), wave_merge_case(), many_chunks_case(), hash_case(), coordinates_case(),
            shifted_case()] + empty_cases()


CASE_NAMES = ["record_classes", "filter_boundaries", "wave_merge", "many_chunks", "hash", "coordinates", "shifted_segments", "empty",
              "only_unmapped"]


def case(name):
    return {"record_classes": record_classes_case, "filter_boundaries": filter_boundaries_case, "wave_merge": wave_merge_case,
            "many_chunks": many_chunks_case, "hash": hash_case, "coordinates": coordinates_case, "shifted_segments": shifted_case,
            "empty": lambda: empty_cases()[0], "only_unmapped": lambda: empty_cases()[1]}[name]()


def merge_tables(tables):
    """Junction tables of disjoint read sets (dicts of arrays) -> one list as oracle.junction_table gives it: counts added, anchors
    the maximum."""
    acc = {}
    for t in tables:
        for l, r, st, n, al, ar in zip(*[t[k].tolist() for k in ("left", "right", "strand", "count", "anchor_left", "anchor_right")]):
            c, a, b = acc.get((l, r, st), (0, 0, 0))
            acc[(l, r, st)] = (c + n, max(a, al), max(b, ar))
    return [k + acc[k] for k in sorted(acc)]


def rows(table):
    """DeviceReads.junctions' dict of arrays -> [(left, right, strand, count, anchor_left, anchor_right)]."""
    return list(zip(*[table[k].tolist() for k in ("left", "right", "strand", "count", "anchor_left", "anchor_right")]))
