"""Shared by the tests of duplicate marking (``spl_reads_duplicates``, ``spl_reads_dedup``, ``duplicates``, ``--dedup``): the
yardstick -- who is examined, a read's unclipped 5' end, a fragment's signature, a group's representative -- restated in plain
Python integers from the issue's text, on top of ``matecases``' mate table, and seeded builders of segments that say what they
cover.  Fragments are grouped in a dictionary keyed by (W0, W1); nothing here sorts them, knows of radix passes or binary searches,
imports the package's code or calls the library; nothing touches the GPU."""
import numpy as np

import genecases as G
import matecases as M
import subsamplecases as S

COUNTS = ("reads", "examined", "pair_fragments", "single_fragments", "duplicate_pairs", "duplicate_singles", "flagged_in_file")
BINS, HIST = 256, 257
CLIPS, ON_REFERENCE = (4, 5), (0, 2, 3, 7, 8)          # S H; M D N = X
LANE_OPS = 8                                           # a CIGAR of more ops than this is copied by the wave
BIAS = 1 << 31

Reads = S.Reads


# ---- the rule -----------------------------------------------------------------------------------------------------------------
def end_of(pos, flag, ops):
    """-> (u, o): the unclipped 5' end of a read and its orientation."""
    ops = [int(v) for v in ops]
    lead = 0
    while lead < len(ops) and (ops[lead] & 15) in CLIPS:
        lead += 1
    o = (flag >> 4) & 1
    if not o:
        u = pos - sum(op >> 4 for op in ops[:lead])
    else:
        rest = ops[lead:]
        tail = 0
        while tail < len(rest) and (rest[len(rest) - 1 - tail] & 15) in CLIPS:
            tail += 1
        u = pos + sum(op >> 4 for op in rest if (op & 15) in ON_REFERENCE) - 1 + sum(op >> 4 for op in rest[len(rest) - tail:] if tail)
    return max(-BIAS, min(BIAS - 1, u)), o


def fragments_of(rs, keys, mate=None):
    """One segment -> (fragments [(W0, W1, W2, leader, mate or None)] in leader order, examined reads [index])."""
    pos, flag, off, cig = rs.pos.tolist(), rs.flag.tolist(), rs.cig_off.tolist(), rs.cigar.tolist()
    keys = [int(k) for k in keys]
    if mate is None:
        mate = M.mate_table_of(rs, keys)[0]
    out, examined = [], []
    for i in range(len(pos)):
        if not G.eligible(flag[i], pos[i], off[i + 1] - off[i]):
            continue
        examined.append(i)
        m = mate[i]
        if m != M.NONE and m < i:
            continue                                   # silent: its leader has the fragment
        mine = end_of(pos[i], flag[i], cig[off[i]:off[i + 1]])
        if m == M.NONE:
            out.append(((mine[0] + BIAS) << 3 | mine[1] << 2, 0, keys[i], i, None))
            continue
        its = end_of(pos[m], flag[m], cig[off[m]:off[m + 1]])
        a_is_mine = mine < its or (mine == its and bool(flag[i] & 0x40))
        a, b = (mine, its) if a_is_mine else (its, mine)
        a_first = 1 if (flag[i] if a_is_mine else flag[m]) & 0x40 else 0
        out.append(((a[0] + BIAS) << 3 | a[1] << 2 | 2 | a_first, (b[0] + BIAS) << 1 | b[1], keys[i], i, m))
    return out, examined


def duplicates(rs, keys, mate=None):
    """One segment -> (dup bool[n], counts dict, hist int64[257])."""
    frags, examined = fragments_of(rs, keys, mate)
    groups = {}
    for w0, w1, w2, leader, m in frags:
        groups.setdefault((w0, w1), []).append((w2, leader, m))
    dup, hist = np.zeros(rs.n, bool), np.zeros(HIST, np.int64)
    counts = dict.fromkeys(COUNTS, 0)
    counts.update(reads=rs.n, examined=len(examined), pair_fragments=sum(1 for f in frags if f[4] is not None), single_fragments=sum(1 for f in frags if f[4] is None),
                  flagged_in_file=sum(1 for i in examined if int(rs.flag[i]) & 0x400))
    for members in groups.values():
        keeper = min(members, key=lambda f: (f[0], f[1]))
        hist[min(len(members), BINS) - 1] += 1
        if len(members) >= BINS:
            hist[BINS] += len(members)
        for w2, leader, m in members:
            if (w2, leader) == keeper[:2]:
                continue
            dup[leader] = True
            if m is None:
                counts["duplicate_singles"] += 1
            else:
                dup[m] = True
                counts["duplicate_pairs"] += 1
    assert counts["examined"] == 2 * counts["pair_fragments"] + counts["single_fragments"]
    return dup, counts, hist


def table_rows(per_chrom):
    """[(chrom, counts dict)] -> the text of ``PREFIX.duplicates.tsv``."""
    lines = ["chrom\treads\texamined\tpair_fragments\tsingle_fragments\tduplicate_pairs\tduplicate_singles\tduplicate_reads\tflagged_in_file\tfraction_duplicated"]
    total = dict.fromkeys(COUNTS, 0)
    for chrom, c in list(per_chrom) + [("total", total)]:
        if chrom != "total":
            for k in COUNTS:
                total[k] += c[k]
        dup_reads = 2 * c["duplicate_pairs"] + c["duplicate_singles"]
        lines.append("\t".join([chrom] + ["%d" % c[k] for k in COUNTS[:6]] + ["%d" % dup_reads, "%d" % c["flagged_in_file"],
                                          repr(dup_reads / c["examined"]) if c["examined"] else "NA"]))
    return "\n".join(lines) + "\n"


def hist_rows(hist):
    return "group_size\tgroups\n" + "".join("%s\t%d\n" % (str(k + 1) if k < BINS - 1 else "256+", int(hist[k])) for k in range(BINS))


# ---- builders -----------------------------------------------------------------------------------------------------------------
class Segment(object):
    """Reads gathered one by one, handed out sorted by POS (stable)."""

    def __init__(self, rng):
        self.rng, self.rows = rng, []

    def read(self, flag, pos, cigar, key):
        self.rows.append((int(pos), int(flag), [int(v) for v in (G.ops(cigar) if isinstance(cigar, str) else cigar)], int(key)))

    def single(self, pos, cigar, key, reverse=False, extra=0):
        self.read((16 if reverse else 0) | extra, pos, cigar, key)

    def pair(self, pos1, cigar1, rev1, pos2, cigar2, rev2, key, extra1=0, extra2=0):
        """Read 1 (0x40) and read 2 (0x80) of one name."""
        self.read(0x1 | 0x2 | 0x40 | (0x10 if rev1 else 0) | (0x20 if rev2 else 0) | extra1, pos1, cigar1, key)
        self.read(0x1 | 0x2 | 0x80 | (0x10 if rev2 else 0) | (0x20 if rev1 else 0) | extra2, pos2, cigar2, key)

    def reads(self):
        order = sorted(range(len(self.rows)), key=lambda i: self.rows[i][0])
        rows = [self.rows[i] for i in order]
        counts = [len(r[2]) for r in rows]
        return Reads([r[0] for r in rows], [r[1] for r in rows], np.concatenate(([0], np.cumsum(counts))), [w for r in rows for w in r[2]],
                     self.rng.choice(np.array([43, 45, 0], np.uint8), len(rows)), np.array([r[3] for r in rows], np.uint64))


def fresh_keys(rng, n):
    """n name keys whose upper 63 bits differ (no two names are one group of the mate table), none 0."""
    out = set()
    while len(out) < n:
        out.add(int(rng.integers(1, 1 << 62)) << 1)
    return sorted(out, key=lambda k: (k * 0x9e3779b97f4a7c15) & M.MASK)


def long_cigar(n_ops, lead_clip=0):
    """A CIGAR text of n_ops ops (above LANE_OPS when asked for), behind an optional soft clip that is one of them."""
    parts = ["%dS" % lead_clip] if lead_clip else []
    while len(parts) < n_ops:
        parts.append("2M" if (len(parts) - (1 if lead_clip else 0)) % 2 == 0 else "1I")
    if parts[-1] == "1I":
        parts[-1] = "1M"
    return "".join(parts)


def corners(rng):
    """One segment with every kind of content the rule distinguishes, each by hand."""
    seg, k = Segment(rng), iter(fresh_keys(rng, 200))
    # forward and reverse singles, and duplicates of each; the representative is the smallest key
    for reverse in (False, True):
        for _ in range(3):
            seg.single(1000, "30M", next(k), reverse)
    # duplicates that differ only in soft clipping (one u, two POS) and non-duplicates at one POS (two u)
    seg.single(2000, "30M", next(k)); seg.single(2005, "5S25M", next(k)); seg.single(2003, "2H1S27M", next(k))
    seg.single(2100, "30M", next(k)); seg.single(2100, "4S26M", next(k))
    seg.single(2200, "30M", next(k), True); seg.single(2200, "26M4S", next(k), True); seg.single(2190, "40M", next(k), True); seg.single(2190, "20M10D10M", next(k), True)
    # POS 1 behind 5S: u = -4, twice
    seg.single(1, "5S20M", next(k)); seg.single(1, "5S22M", next(k))
    # H and S on both sides, forward and reverse; a read of clips only, forward and reverse
    seg.single(2300, "2H3S20M4S1H", next(k)); seg.single(2305, "20M", next(k)); seg.single(2300, "2H3S20M4S1H", next(k), True); seg.single(2300, "25M", next(k), True)
    seg.single(2400, "10S5H", next(k)); seg.single(2415, "20M", next(k)); seg.single(2400, "10S5H", next(k), True); seg.single(2400, "3S", next(k), True)
    # pairs of every orientation, each with a duplicate whose reads are clipped otherwise, and one that is none (another second end)
    for n, (rev1, rev2) in enumerate(((False, True), (True, False), (False, False), (True, True))):
        at = 3000 + 400 * n
        seg.pair(at, "30M", rev1, at + 150, "30M", rev2, next(k))
        seg.pair(at + 2, "2S28M", rev1, at + 150, "28M2S", rev2, next(k))
        seg.pair(at, "30M", rev1, at + 151, "30M", rev2, next(k))
        seg.pair(at + 150, "30M", rev2, at, "30M", rev1, next(k))           # the same two ends with read 1 and read 2 swapped
    # pairs with equal ends: the tie goes to the read with 0x40
    seg.pair(5000, "30M", False, 5000, "30M", False, next(k)); seg.pair(5000, "30M", False, 5000, "20M", False, next(k))
    seg.pair(5000, "25M", True, 5001, "24M", True, next(k))
    # nameless reads: singles that tie at W2 = 0 (the lowest index stays), and a nameless "pair" that is two singles
    seg.single(6000, "30M", 0); seg.single(6000, "30M", 0); seg.single(6000, "30M", next(k))
    seg.read(99, 6100, "30M", 0); seg.read(147, 6200, "30M", 0)
    # a name occurring twice: two pairs of one key, at the same ends
    twice = next(k)
    seg.pair(6500, "30M", False, 6700, "30M", True, twice); seg.pair(6500, "30M", False, 6700, "30M", True, twice)
    # an incoming 0x400 on the representative (the smaller key) and none on the duplicate
    a, b = sorted((next(k), next(k)))
    seg.single(7000, "30M", a, extra=0x400); seg.single(7000, "30M", b)
    a, b = sorted((next(k), next(k)))
    seg.pair(7100, "30M", False, 7300, "30M", True, a, extra1=0x400, extra2=0x400); seg.pair(7100, "30M", False, 7300, "30M", True, b)
    # secondary, supplementary, QC-failed and unmapped records under a duplicate's name: never marked
    a, b = sorted((next(k), next(k)))
    seg.single(7500, "30M", a); seg.single(7500, "30M", b)
    for extra in (0x100, 0x800, 0x200, 0x4):
        seg.read(extra, 7500, "30M", b)
    # a pair whose mate is on another segment: a single here (pairs_across puts its mate elsewhere), twice
    seg.read(0x1 | 0x40 | 0x20, 8000, "30M", ACROSS[0]); seg.read(0x1 | 0x40 | 0x20, 8000, "30M", ACROSS[1])
    # CIGARs above LANE_OPS ops on a kept read and on a removed one
    a, b = sorted((next(k), next(k)))
    seg.single(9000, long_cigar(21), a); seg.single(9003, long_cigar(22, lead_clip=3), b)
    a, b = sorted((next(k), next(k)))
    seg.pair(9100, long_cigar(300), False, 9800, long_cigar(11), True, a); seg.pair(9100, long_cigar(300), False, 9800, long_cigar(11), True, b)
    return seg.reads()


ACROSS = (0x5eed0000, 0x5eed0100)


def across(rng):
    """The segment that holds the mates of ``corners``' last two: second reads alone, duplicates of each other."""
    seg = Segment(rng)
    seg.read(0x1 | 0x80 | 0x10, 400, "30M", ACROSS[0]); seg.read(0x1 | 0x80 | 0x10, 400, "30M", ACROSS[1])
    seg.single(100, "30M", 77 << 1)
    return seg.reads()


CIGARS = ("30M", "3S27M", "27M3S", "12M80N18M", "10M2D20M", "2H28M", "15M1I14M")


def crowd(rng, n, places=None, pair_share=0.5):
    """A segment of exactly n reads: pairs and singles at few places, so that groups of every small size occur."""
    seg, keys = Segment(rng), iter(fresh_keys(rng, n + 1))
    places = max(2, n // 6) if places is None else places
    left = n
    while left:
        at = 50 + 7 * int(rng.integers(0, places))
        cigar = CIGARS[int(rng.integers(0, len(CIGARS)))]
        if left >= 2 and rng.random() < pair_share:
            seg.pair(at, cigar, bool(rng.integers(0, 2)), at + 60 * int(rng.integers(0, 3)), CIGARS[int(rng.integers(0, 3))], bool(rng.integers(0, 2)), next(keys))
            left -= 2
        else:
            seg.single(at, cigar, 0 if rng.random() < 0.05 else next(keys), bool(rng.integers(0, 2)))
            left -= 1
    return seg.reads()


def one_group(rng, n_fragments, paired, long_at=()):
    """n_fragments identical fragments; ``long_at``: the fragments (by number) whose first read has a CIGAR above LANE_OPS ops."""
    seg, keys = Segment(rng), fresh_keys(rng, n_fragments)
    for j in range(n_fragments):
        cigar = long_cigar(13) if j in long_at else "26M"
        if paired:
            seg.pair(500, cigar, False, 640, "30M", True, keys[j])
        else:
            seg.single(500, cigar, keys[j])
    return seg.reads()


def unique(rng, n):
    seg, keys = Segment(rng), fresh_keys(rng, n)
    for j in range(n):
        seg.single(10 + 3 * j, "20M", keys[j], bool(j & 1))
    return seg.reads()


def joined(*parts):
    """Segments' reads as one segment, sorted by POS again."""
    pos = np.concatenate([p.pos for p in parts])
    order = np.argsort(pos, kind="stable")
    n_ops = np.concatenate([p.n_ops for p in parts])
    starts = np.concatenate(([0], np.cumsum(n_ops)))[:-1]
    cigar = np.concatenate([p.cigar for p in parts])
    words = [cigar[starts[i]:starts[i] + n_ops[i]] for i in order]
    return Reads(pos[order], np.concatenate([p.flag for p in parts])[order], np.concatenate(([0], np.cumsum(n_ops[order]))),
                 np.concatenate(words) if words else np.zeros(0, np.uint32), np.concatenate([p.xs for p in parts])[order], np.concatenate([p.keys for p in parts])[order])


def sizes(tile):
    return [0, 1, 2, 255, 256, 257, tile - 1, tile, tile + 1, 2 * tile + 3]


def all_cases(tile):
    """-> [(name, [Reads per segment])]."""
    rng = np.random.default_rng(20261021)
    out = [("corners", [corners(rng), across(rng)])]
    for n in sizes(tile):
        out.append(("n%d" % n, [crowd(rng, n)]))
    out.append(("group_across_tiles", [joined(one_group(rng, tile + 200, True, long_at=(0, 5, tile + 199)), crowd(rng, 40))]))
    out.append(("group_255_and_256", [joined(one_group(rng, 255, False), unique(rng, 9)), one_group(rng, 256, True)]))
    out.append(("all_unique", [unique(rng, tile + 5)]))
    out.append(("all_one_group", [one_group(rng, tile // 2 + 3, True)]))
    out.append(("singles_only", [crowd(rng, 300, places=5, pair_share=0.0)]))
    out.append(("empty_middle", [crowd(rng, 70), crowd(rng, 0), crowd(rng, tile + 9)]))
    out.append(("empty_middle_corners", [corners(rng), crowd(rng, 0), across(rng)]))
    return out


# ---- what the cases cover -----------------------------------------------------------------------------------------------------
def kinds_of(segs):
    """The set of what occurs in one set's segments, read off the restatement's own answers."""
    kinds = set()
    lone = []
    for rs in segs:
        keys = rs.keys.tolist()
        mate = M.mate_table_of(rs, keys)[0]
        frags, examined = fragments_of(rs, keys, mate)
        dup, counts, hist = duplicates(rs, keys, mate)
        pos, flag, off, cig = rs.pos.tolist(), rs.flag.tolist(), rs.cig_off.tolist(), rs.cigar.tolist()
        ops = lambda i: cig[off[i]:off[i + 1]]
        groups = {}
        for w0, w1, w2, leader, m in frags:
            groups.setdefault((w0, w1), []).append((w2, leader, m))
            o_a = (w0 >> 2) & 1
            if m is None:
                kinds.add("single reverse" if o_a else "single forward")
            else:
                kinds.add("pair " + "FR"[o_a] + "FR"[w1 & 1])
                if w0 >> 2 == w1:
                    kinds.add("equal ends")
            if not w2:
                kinds.add("nameless")
        for members in groups.values():
            leaders = [f[1] for f in members]
            if len({pos[i] for i in leaders}) > 1:
                kinds.add("one u, two POS")
            if len(members) >= 3:
                kinds.add("group of three")
            keeper = min(members, key=lambda f: (f[0], f[1]))[1]
            if flag[keeper] & 0x400 and any(not flag[i] & 0x400 for i in leaders if i != keeper):
                kinds.add("0x400 on the representative only")
            names = [f[0] for f in members if f[0]]
            if len(set(names)) < len(names):
                kinds.add("a name twice")
        by_pos = {}
        for w0, w1, w2, leader, m in frags:
            if m is None:
                by_pos.setdefault((pos[leader], (w0 >> 2) & 1), set()).add(w0)
        if any(len(v) > 1 for v in by_pos.values()):
            kinds.add("one POS, two u")
        marked_keys = {keys[i] for i in np.flatnonzero(dup)}
        for i in range(rs.n):
            codes = [w & 15 for w in ops(i)]
            inner = [j for j, c in enumerate(codes) if c not in CLIPS]
            if i in examined:
                if pos[i] == 1 and ops(i)[:1] == [5 << 4 | 4] and end_of(pos[i], flag[i], ops(i))[0] == -4:
                    kinds.add("u = -4")
                if codes and not inner:
                    kinds.add("clips only")
                if inner and {4, 5} <= set(codes[:inner[0]]) and {4, 5} <= set(codes[inner[-1] + 1:]):
                    kinds.add("H and S on both sides")
                if len(codes) > LANE_OPS:
                    kinds.add("long CIGAR removed" if dup[i] else "long CIGAR kept")
                if M.pairable(flag[i], pos[i], len(codes), keys[i]) and mate[i] == M.NONE and not flag[i] & 0x8:
                    lone.append(keys[i])
            elif keys[i] in marked_keys:
                for bit, name in ((0x100, "secondary"), (0x800, "supplementary"), (0x200, "QC-failed"), (0x4, "unmapped")):
                    if flag[i] & bit:
                        kinds.add(name + " under a duplicate's name")
                assert not dup[i]
        if hist[BINS - 2]:
            kinds.add("group of 255")
        if hist[BINS - 1]:
            kinds.add("group of 256+")
    if len(lone) != len(set(lone)):
        kinds.add("mate on another segment")
    return kinds


KINDS = {"single forward", "single reverse", "pair FR", "pair RF", "pair FF", "pair RR", "equal ends", "u = -4", "H and S on both sides", "clips only", "one u, two POS",
         "one POS, two u", "nameless", "a name twice", "0x400 on the representative only", "secondary under a duplicate's name", "supplementary under a duplicate's name",
         "QC-failed under a duplicate's name", "unmapped under a duplicate's name", "mate on another segment", "long CIGAR kept", "long CIGAR removed", "group of three",
         "group of 255", "group of 256+"}


def assert_covers(cases, tile):
    """Every kind of content and every size the issue lists occurs in the cases."""
    kinds = set()
    for _, segs in cases:
        kinds |= kinds_of(segs)
    assert KINDS <= kinds, KINDS - kinds
    have = {rs.n for _, segs in cases for rs in segs}
    assert set(sizes(tile)) <= have, set(sizes(tile)) - have
    assert any(len(segs) == 3 and segs[1].n == 0 and segs[0].n and segs[2].n for _, segs in cases)
    largest = max(int(np.flatnonzero(duplicates(rs, rs.keys.tolist())[2][:BINS])[-1]) for _, segs in cases for rs in segs if rs.n)
    assert largest == BINS - 1
    assert any(rs.n > 1 and not duplicates(rs, rs.keys.tolist())[0].any() for _, segs in cases for rs in segs)
    assert any(rs.n > 2 * tile and duplicates(rs, rs.keys.tolist())[2][BINS] >= tile + 200 for _, segs in cases for rs in segs)


# ---- files --------------------------------------------------------------------------------------------------------------------
def reads_of_records(records, names):
    """[(flag, POS, CIGAR text)] and their names, in the file's order -> Reads with the names' keys."""
    counts = [len(G.ops(r[2])) for r in records]
    cigar = np.concatenate([G.ops(r[2]) for r in records]) if records else np.zeros(0, np.uint32)
    return Reads([r[1] for r in records], [r[0] for r in records], np.concatenate(([0], np.cumsum(counts))), cigar, np.zeros(len(records), np.uint8),
                 np.array([M.name_key(n) for n in names], np.uint64))
