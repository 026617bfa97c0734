"""Shared by the tests of mate pairing and fragment counting: the yardstick -- the name key, who is pairable, the mate table and a
fragment's gene -- restated in plain Python from the issue's text, on top of ``genecases``' per-base gene sets, and a generator of
paired read sets that says what it covers.  The mate table is made by grouping tuples in dictionaries and zipping lists; nothing here
knows of radix sorts or binary searches; nothing here imports the package's counting code or calls the library; nothing touches the
GPU."""
import numpy as np

import genecases as G

NONE = 0xFFFFFFFF            # a read without a mate
SILENT = -4                  # what a read adds whose leader counts the fragment
MASK = (1 << 64) - 1


# ---- the key ------------------------------------------------------------------------------------------------------------------
def name_key(name):
    name = bytes(name)
    if name in (b"", b"*"):
        return 0
    h = 0xcbf29ce484222325
    for b in name:
        h = ((h ^ b) * 0x100000001b3) & MASK
    h ^= h >> 33
    h = (h * 0xff51afd7ed558ccd) & MASK
    h ^= h >> 33
    h = (h * 0xc4ceb9fe1a85ec53) & MASK
    h ^= h >> 33
    return h or 1


# ---- the table ----------------------------------------------------------------------------------------------------------------
def pairable(flag, pos, n_ops, key):
    return G.eligible(flag, pos, n_ops) and bool(flag & 1) and (bool(flag & 0x40) != bool(flag & 0x80)) and key != 0


def mate_table(flag, pos, n_ops, keys):
    """One segment's reads in their order -> (mate list, counts dict): per group (equal key >> 1) the j-th first and the j-th second
    read are mates."""
    flag, pos, n_ops, keys = [int(v) for v in flag], [int(v) for v in pos], [int(v) for v in n_ops], [int(v) for v in keys]
    groups = {}
    for i in range(len(flag)):
        if pairable(flag[i], pos[i], n_ops[i], keys[i]):
            groups.setdefault(keys[i] >> 1, ([], []))[1 if flag[i] & 0x80 else 0].append(i)
    mate = [NONE] * len(flag)
    for firsts, seconds in groups.values():
        for a, b in zip(firsts, seconds):
            mate[a], mate[b] = b, a
    n_pairable = sum(len(f) + len(s) for f, s in groups.values())
    paired = sum(1 for m in mate if m != NONE)
    lonely = sum(1 for f, s in groups.values() for i in f + s if mate[i] == NONE and not flag[i] & 0x8)
    return mate, dict(pairable=n_pairable, paired=paired, unpaired_mate_mapped=lonely)


def mate_table_of(rs, keys):
    return mate_table(rs.flag, rs.pos, np.diff(rs.cig_off.astype(np.int64)), keys)


def group_shapes(flag, pos, n_ops, keys):
    """-> the set of (first reads, second reads) over the groups."""
    groups = {}
    for i in range(len(flag)):
        if pairable(int(flag[i]), int(pos[i]), int(n_ops[i]), int(keys[i])):
            g = groups.setdefault(int(keys[i]) >> 1, [0, 0])
            g[1 if int(flag[i]) & 0x80 else 0] += 1
    return {tuple(g) for g in groups.values()}


# ---- a fragment's gene --------------------------------------------------------------------------------------------------------
def genes_under(flag, pos, ops, bases, stranded=0, shift=0):
    """-> (set of genes, whether a base says many) under the blocks of one read, on the bases of its own strand."""
    mine = bases[G.read_strand(flag, stranded)] if stranded else bases
    genes, many = set(), False
    for s, e in G.blocks_of(pos, ops, shift):
        for p in range(s, e):
            c = mine.at(p)
            if c == G.MANY:
                many = True
            elif c:
                genes.add(c - 1)
    return genes, many


def fragment_results(rs, keys, bases, stranded=0, shift=0, mate=None):
    """Per read: a gene's index, G.NO_FEATURE, G.AMBIGUOUS, G.NOT_COUNTED or SILENT."""
    pos, flag, off, cig = rs.pos.tolist(), rs.flag.tolist(), rs.cig_off.tolist(), rs.cigar.tolist()
    if mate is None:
        mate = mate_table_of(rs, keys)[0]
    out = []
    for i in range(len(pos)):
        ops = cig[off[i]:off[i + 1]]
        if not G.eligible(flag[i], pos[i], len(ops)):
            out.append(G.NOT_COUNTED)
            continue
        m = mate[i]
        if m != NONE and m < i:
            out.append(SILENT)
            continue
        genes, many = genes_under(flag[i], pos[i], ops, bases, stranded, shift)
        if m != NONE:
            more, many2 = genes_under(flag[m], pos[m], cig[off[m]:off[m + 1]], bases, stranded, shift)
            genes, many = genes | more, many or many2
        out.append(G.AMBIGUOUS if many or len(genes) > 1 else next(iter(genes)) if genes else G.NO_FEATURE)
    return out


def counts_of(results, n_genes, keep=None):
    """``genecases.counts_of`` over the reads that add something."""
    return G.counts_of([r for i, r in enumerate(results) if r != SILENT and (keep is None or keep[i])], n_genes)


# ---- paired content -----------------------------------------------------------------------------------------------------------
SPECIAL_NAMES = (b"", b"*", b"q", b"n" * 254, b"caf\xc3\xa9\x80\xff\xfe")
PAIR_FLAGS = ((99, 147), (83, 163), (65, 129))
SINGLETON_FLAGS = (73, 137)
READ_CIGARS = ("30M", "50M", "12M3I20M", "10M5D25M", "20M80N20M", "5S25M", "15M40N10M200N15M", "40=", "10X20M")


def paired_records(rng, n_fragments, span, special_names=SPECIAL_NAMES):
    """-> (records [(flag, POS, CIGAR text)], names [bytes], kinds: the set of what occurs), sorted by POS.  Fragments of every flag
    kind and group shape; ``special_names``: names that each name one proper pair."""
    rows, kinds = [], set()

    def place(flag, name, pos=None, cigar=None):
        rows.append((flag, int(rng.integers(1, span)) if pos is None else pos, READ_CIGARS[int(rng.integers(0, len(READ_CIGARS)))] if cigar is None else cigar, name))

    def pair(flags, name, gap=None):
        pos = int(rng.integers(1, span - 900))
        place(flags[0], name, pos)
        place(flags[1], name, pos + (int(rng.integers(0, 800)) if gap is None else gap))

    for k in range(n_fragments):
        name = b"frag:%d/x" % k
        what = k % 20
        if what < 12:
            flags = PAIR_FLAGS[k % 3]
            pair(flags, name)
            kinds.add(flags)
        elif what == 12:
            f = SINGLETON_FLAGS[(k // 20) % 2]
            place(f, name)
            kinds.add(f)
        elif what == 13:                       # a secondary / a supplementary copy with the pair's name, on either mate
            pair((99, 147), name)
            extra = (99 | 256, 147 | 2048)[(k // 20) % 2]
            place(extra, name)
            kinds.add("secondary" if extra & 256 else "supplementary")
        elif what == 14:                       # reads that are no mates, under a pair's name
            pair((83, 163), name)
            which = (k // 20) % 5
            if which == 0:
                place(16, name); kinds.add("0x1 clear")
            elif which == 1:
                place(1 | 64 | 128, name); kinds.add("0x40 and 0x80")
            elif which == 2:
                place(1 | 4 | 64, name); kinds.add("unmapped")
            elif which == 3:
                place(99, name, pos=0); kinds.add("POS 0")
            else:
                place(147, name, cigar=""); kinds.add("no CIGAR")
        elif what == 15:                       # a name used by two fragments: a group of 2 + 2
            pair((99, 147), name); pair((99, 147), name)
            kinds.add("2+2")
        elif what == 16:                       # three first reads and one second
            pair((99, 147), name); place(99, name); place(65, name)
            kinds.add("3+1")
        elif what == 17:                       # mates that are neighbours at one POS
            pair((65, 129), name, gap=0)
            kinds.add("adjacent")
        elif what == 18:                       # a pair without a name: two reads without a mate
            pair((99, 147), (b"", b"*")[(k // 20) % 2])
            kinds.add("nameless")
        else:                                  # a second read alone, its mate mapped elsewhere by its flag
            place(163, name)
            kinds.add("lone second")
    for name in special_names:
        pair((99, 147), name)
        kinds.add(("name", len(name), max(name) >= 0x80 if name else False))
    order = sorted(range(len(rows)), key=lambda i: rows[i][1])
    return [rows[i][:3] for i in order], [rows[i][3] for i in order], kinds


KINDS = set(PAIR_FLAGS) | set(SINGLETON_FLAGS) | {"secondary", "supplementary", "0x1 clear", "0x40 and 0x80", "unmapped", "POS 0", "no CIGAR", "2+2", "3+1", "adjacent",
                                                  "nameless", "lone second"} | {("name", 0, False), ("name", 1, False), ("name", 254, False), ("name", 8, True)}


def assert_covers(kinds, flag, pos, n_ops, keys):
    """Every flag kind, group shape and name kind the issue lists occurs in what the generator made."""
    assert KINDS <= kinds, KINDS - kinds
    shapes = group_shapes(flag, pos, n_ops, keys)
    assert {(1, 1), (2, 2), (3, 1), (1, 0), (0, 1)} <= shapes, shapes
