"""Shared by the tests of ``genecounts``: the yardstick -- the features of an annotation, the gene set under every base, the per-read
rule and the file -- restated in plain loops from the issue's text.  A gene set per base is made from the feature list by slice
writes into per-position Python sets; a read is held against the positions its blocks cover, one by one.  Nothing here knows of
stretch tables, searches or ballots; nothing here imports ``spliser_amd/genecounts.py`` or calls the library; nothing touches the
GPU."""
import numpy as np

MANY = 0xFFFFFFFF
NO_FEATURE, AMBIGUOUS, NOT_COUNTED = -1, -2, -3          # what a read comes to when it is not a gene's index
SPECIALS = ("__no_feature", "__ambiguous", "__not_counted")
COVERING, GAPS = (0, 7, 8), (2, 3)                       # M = X cover and advance; D N advance


# ---- features -----------------------------------------------------------------------------------------------------------------
def value_of(column9, key):
    """``key "value";`` (GTF) or ``key=value;`` (GFF3), quotes stripped; None when the attribute is not there."""
    for part in column9.split(";"):
        part = part.strip()
        for sep in ("=", " "):
            if part.startswith(key + sep):
                return part[len(key) + 1:].strip().strip('"')
    return None


def features_of_text(text, ftype="exon", id_attr="gene_id"):
    """-> (sorted ids, {chrom: [(left, right, strand text, gene index)]}); ValueError with the line number for a feature without the id."""
    rows = []
    for number, line in enumerate(text.split("\n"), 1):
        cols = line.split("\t")
        if line.startswith("#") or len(cols) < 9 or cols[2] != ftype:
            continue
        gene = value_of(cols[8], id_attr)
        if gene is None:
            raise ValueError("line %d" % number)
        rows.append((cols[0], int(cols[3]) - 1, int(cols[4]), cols[6], gene))
    ids = sorted({r[4] for r in rows})
    by_chrom = {}
    for chrom, left, right, strand, gene in rows:
        by_chrom.setdefault(chrom, []).append((left, right, strand, ids.index(gene)))
    return ids, by_chrom


def select(features, which):
    """The selection of a map: None = all features; '+' = those whose strand is not '-'; '-' = those whose strand is not '+'."""
    return [f for f in features if which is None or f[2] != {"+": "-", "-": "+"}[which]]


# ---- the gene set under every base ------------------------------------------------------------------------------------------------
def sets_per_base(features, length):
    """features: [(left, right, strand, gene index)] -> a list of ``length`` sets, the genes whose features cover each 0-based base."""
    sets = [set() for _ in range(length)]
    for left, right, _, gene in features:
        if right <= left:
            continue
        for p in range(max(left, 0), min(right, length)):
            sets[p].add(gene)
    return sets


def code_of_set(s):
    return 0 if not s else MANY if len(s) > 1 else next(iter(s)) + 1


class Bases(object):
    """The code under every base of [0, len(codes)), and ``tail``, the code of every base beyond."""

    def __init__(self, codes, tail=0):
        self.codes, self.tail = codes, tail

    def at(self, p):
        if p < 0:
            return 0
        return self.codes[p] if p < len(self.codes) else self.tail


def bases_of_features(features, length, which=None):
    assert all(f[1] <= length for f in features)
    return Bases([code_of_set(s) for s in sets_per_base(select(features, which), length)])


def bases_of_map(start, code):
    """A gene map by its definition: code[k] holds for start[k] <= p < start[k + 1], the last entry to the end, 0 below start[0]."""
    start, code = [int(v) for v in start], [int(v) for v in code]
    if not start:
        return Bases([])
    codes = [0] * start[-1]
    for k in range(len(start) - 1):
        codes[start[k]:start[k + 1]] = [code[k]] * (start[k + 1] - start[k])
    return Bases(codes, code[-1])


def map_says(start, code, p):
    """What a map (start, code) says at base p, by a walk over all of its entries."""
    said = 0
    for s, c in zip(start, code):
        if int(s) <= p:
            said = int(c)
    return said


# ---- a read -----------------------------------------------------------------------------------------------------------------------
def fr_strand(flag):
    first = bool(flag & 64) or not (flag & 1)
    reverse = bool(flag & 16)
    return "-" if (reverse if first else not reverse) else "+"


def read_strand(flag, stranded):
    s = fr_strand(flag)
    return s if stranded == 1 else {"+": "-", "-": "+"}[s]


def eligible(flag, pos, n_ops):
    return not (flag & (0x4 | 0x100 | 0x200 | 0x800)) and pos >= 1 and n_ops >= 1


def blocks_of(pos, ops, shift=0):
    """-> [(start, end)] 0-based half-open: M, = and X cover; D and N are gaps; covering ops that abut are one block."""
    p, out = pos - 1 + shift, []
    for op in ops:
        code, length = int(op) & 15, int(op) >> 4
        if length == 0:
            continue
        if code in COVERING:
            if out and out[-1][1] == p:
                out[-1] = (out[-1][0], p + length)
            else:
                out.append((p, p + length))
            p += length
        elif code in GAPS:
            p += length
    return out


def result_of(flag, pos, ops, bases, stranded=0, shift=0):
    """bases: a ``Bases`` (unstranded) or {'+': Bases, '-': Bases} -> a gene's index, NO_FEATURE, AMBIGUOUS or NOT_COUNTED."""
    if not eligible(flag, pos, len(ops)):
        return NOT_COUNTED
    mine = bases[read_strand(flag, stranded)] if stranded else bases
    genes, many = set(), False
    for s, e in blocks_of(pos, ops, shift):
        last = None
        for p in range(s, e):
            c = mine.at(p)
            if c == last:
                continue
            last = c
            if c == MANY:
                many = True
            elif c:
                genes.add(c - 1)
    if many or len(genes) > 1:
        return AMBIGUOUS
    return next(iter(genes)) if genes else NO_FEATURE


def results_of(rs, bases, stranded=0, shift=0):
    pos, flag, off, cig = rs.pos.tolist(), rs.flag.tolist(), rs.cig_off.tolist(), rs.cigar.tolist()
    return [result_of(flag[i], pos[i], cig[off[i]:off[i + 1]], bases, stranded, shift) for i in range(len(pos))]


def counts_of(results, n_genes, keep=None):
    """-> n_genes + 3 numbers: the genes' reads, then no feature, ambiguous, not counted."""
    out = [0] * (n_genes + 3)
    for i, r in enumerate(results):
        if keep is not None and not keep[i]:
            continue
        out[r if r >= 0 else n_genes - 1 - r] += 1
    return out


def run_heads(results, wave=64):
    """The adds a wave-by-wave count of runs makes for these results in this order: a lane is a head when it is the wave's first or
    its result differs from the lane's before it; heads whose result is a gene add."""
    heads = 0
    for i, r in enumerate(results):
        if r >= 0 and (i % wave == 0 or results[i - 1] != r):
            heads += 1
    return heads


# ---- the file ---------------------------------------------------------------------------------------------------------------------
def file_text(ids, counts, only=None):
    text = ""
    for k, gene in enumerate(ids):
        if only is None or k in only:
            text += "%s\t%d\n" % (gene, counts[k])
    for k, name in enumerate(SPECIALS):
        text += "%s\t%d\n" % (name, counts[len(ids) + k])
    return text


def ops(text):
    """CIGAR text -> BAM ops."""
    out, num = [], ""
    for ch in text:
        if ch.isdigit():
            num += ch
        else:
            out.append((int(num) << 4) | "MIDNSHP=X".index(ch))
            num = ""
    return np.asarray(out, np.uint32)


# ---- the corner cases: a chromosome whose answers can be read off the rule ----------------------------------------------------------
CORNER_IDS = ["g0", "g1", "gIn", "gOut", "gL", "gR", "gX", "gY", "gZ"]
CORNER_LENGTH = 120000
# (left, right, strand, gene index): two lone genes; gIn inside gOut's intron; gL and gR touch at 2100; gX and gY overlap on
# [3050, 3100), gY without a strand; gZ: 1500 exons of 30 bases every 60 from 10000 on -- 3000 stretches
CORNER_FEATURES = ([(100, 200, "+", 0), (300, 400, "-", 1), (1200, 1300, "-", 2), (1000, 1100, "+", 3), (1400, 1500, "+", 3), (2000, 2100, "+", 4), (2100, 2200, "-", 5),
                    (3000, 3100, "+", 6), (3050, 3150, ".", 7)] + [(10000 + 60 * i, 10030 + 60 * i, "+", 8) for i in range(1500)])
# name, flag, POS, CIGAR, the unstranded answer by the rule's text
CORNERS = [
    ("a block ending exactly at a stretch's start", 0, 91, "10M", NO_FEATURE),
    ("a block starting on a stretch's last base", 0, 200, "5M", 0),
    ("an intron that swallows an inner gene whole", 0, 1051, "40M320N40M", 3),
    ("the inner gene itself", 16, 1251, "20M", 2),
    ("a deletion over a gene boundary", 0, 2091, "5M10D5M", AMBIGUOUS),
    ("a deletion inside one gene", 0, 2011, "5M10D5M", 4),
    ("an insertion between two blocks that abut", 0, 196, "3M2I3M", 0),
    ("many on the first block", 0, 3061, "10M500N10M", AMBIGUOUS),
    ("one gene, then many", 0, 3041, "5M10N5M", AMBIGUOUS),
    ("two genes either side of an intron", 0, 191, "5M100N10M", AMBIGUOUS),
    ("a read of 2 203 ops, one block and an intron", 0, 10001, "1M1I" * 1100 + "5M300N7M", 8),
    ("a read of 2 203 ops, 1 101 blocks", 16, 10001, "1M1D" * 1100 + "5M300N7M", 8),
    ("one block over 3 000 stretches", 0, 9991, "100000M", 8),
    ("soft clips only", 0, 150, "30S", NO_FEATURE),
    ("a duplicate counts", 1024, 150, "30M", 0),
    ("POS 0", 0, 0, "30M", NOT_COUNTED),
    ("no ops", 0, 150, "", NOT_COUNTED),
    ("unmapped", 4, 150, "30M", NOT_COUNTED),
    ("secondary", 256, 150, "30M", NOT_COUNTED),
    ("QC-failed", 512, 150, "30M", NOT_COUNTED),
    ("supplementary", 2048, 150, "30M", NOT_COUNTED),
]
STRAND_FLAGS = (0, 16, 99, 147, 83, 163)
CORNERS += [("flag %d in gX and gY" % f, f, 3061, "10M", AMBIGUOUS) for f in STRAND_FLAGS] + [("flag %d in g1" % f, f, 311, "10M", 1) for f in STRAND_FLAGS]

_CORNER_BASES = {}


def corner_bases(stranded=0):
    """The yardstick's bases of the corner chromosome (made once: it writes every position)."""
    if stranded not in _CORNER_BASES:
        if stranded:
            _CORNER_BASES[stranded] = {w: bases_of_features(CORNER_FEATURES, CORNER_LENGTH, w) for w in "+-"}
        else:
            _CORNER_BASES[stranded] = bases_of_features(CORNER_FEATURES, CORNER_LENGTH)
    return _CORNER_BASES[1 if stranded else 0]


def corner_arrays():
    """left, right, strand byte, gene index of CORNER_FEATURES as arrays."""
    f = CORNER_FEATURES
    return (np.array([x[0] for x in f], np.int64), np.array([x[1] for x in f], np.int64), np.array([ord(x[2]) for x in f], np.uint8), np.array([x[3] for x in f], np.int64))


# ---- random content -----------------------------------------------------------------------------------------------------------
CIGARS = ("30M", "50M", "1M", "12M3I20M", "10M5D25M", "20M80N20M", "5S25M", "15M40N10M200N15M", "25M5S", "8M2D8M30N9M", "40=", "10X20M", "6H30M", "30S")
FLAGS = (0, 16, 99, 147, 83, 163, 1024, 256, 4, 512, 2048)


def random_features(rng, length, n_genes, n_features):
    """Features of every kind on [0, length): nested and overlapping genes, one gene's exons overlapping, genes that touch, '.'
    strands, a feature without a base."""
    out = []
    for _ in range(n_features):
        left = int(rng.integers(0, length - 1))
        right = min(length, left + int(rng.integers(1, max(2, length // 12))))
        out.append((left, right, "+-."[int(rng.integers(0, 3))], int(rng.integers(0, n_genes))))
    l, r, s, g = out[0]
    out.append((r, min(length, r + 17), s, (g + 1) % n_genes))        # touches the first one
    out.append((l, r, s, g))                                          # the same exon twice
    out.append((l + (r - l) // 3, r - (r - l) // 3, "-", (g + 2) % n_genes))   # nested in it (may be empty)
    out.append((min(length, l + 5), min(length, l + 5), "+", g))      # no base
    return out


def random_records(rng, n, span):
    """(flag, POS, CIGAR text) sorted by POS; a few with POS 0 or no ops."""
    recs = []
    for _ in range(n):
        cigar = CIGARS[int(rng.integers(0, len(CIGARS)))] if rng.random() > 0.02 else ""
        recs.append((int(FLAGS[int(rng.integers(0, len(FLAGS)))]) if rng.random() < 0.6 else int(STRAND_FLAGS[int(rng.integers(0, 6))]),
                     int(rng.integers(1, span)) if rng.random() > 0.02 else 0, cigar))
    return sorted(recs, key=lambda r: r[1])
