"""Shared by the tests of ``exoncounts``: the yardstick -- the feature lines over every base, the bins, the per-read verdict and hit
list, and the two files -- restated in plain loops from the rule's text.  Per base, the set of covering feature LINES; a bin is a
maximal run of bases with one non-empty set whose lines share a gene, a run whose lines have two genes or more is shared; a read
is held against the bases its blocks cover, one by one.  Nothing here knows of cuts, stretch tables, searches, rounds or ballots;
nothing here imports ``spliser_amd/exoncounts.py`` or calls the library; nothing touches the GPU.  (``genecases`` gives the
generators, eligibility, strands and blocks: they are ``genecounts``' own by the rule.)

The rule.  Features and selections are ``genecounts``'.  For one selection, cut the chromosome at every left and right of its
features; a piece between two consecutive cuts covered by no feature is nothing, by features of exactly one gene g the BIN
(g, start, end), by features of two or more genes shared.  A chromosome's bins are numbered in the order (start, end, gene) over
the distinct triples of both maps.  A read's hit stretches are those a block overlaps by a base or more, each once.  Any hit
shared, or bins of two genes: ambiguous, no bin incremented; no bin hit: no feature; otherwise counted, every hit bin + 1; every
other read: not counted."""
import genecases as G

COUNTED, NO_FEATURE, AMBIGUOUS, NOT_COUNTED = 0, -1, -2, -3
SHARED = "shared"
SPECIALS = ("__no_feature", "__ambiguous", "__not_counted")


# ---- what lies under every base -------------------------------------------------------------------------------------------------
class Labels(object):
    """Under every base of [0, len(labels)): None, SHARED, or (gene, key) -- the bin ``key`` of gene ``gene``.  Nothing beyond."""

    def __init__(self, labels):
        self.labels = labels

    def at(self, p):
        return self.labels[p] if 0 <= p < len(self.labels) else None


def labels_of_features(features, length, which=None):
    """features: [(left, right, strand, gene index)] -> Labels, the keys being the triples (start, end, gene)."""
    lines = [set() for _ in range(length)]
    for number, (left, right, strand, gene) in enumerate(features):
        if right <= left or (which is not None and strand == {"+": "-", "-": "+"}[which]):
            continue
        assert 0 <= left and right < length
        for p in range(left, right):
            lines[p].add(number)
    labels, p = [None] * length, 0
    while p < length:
        q = p + 1
        while q < length and lines[q] == lines[p]:
            q += 1
        if lines[p]:
            genes = {features[k][3] for k in lines[p]}
            label = (next(iter(genes)), (p, q, next(iter(genes)))) if len(genes) == 1 else SHARED
            labels[p:q] = [label] * (q - p)
        p = q
    return Labels(labels)


def bins_of(label_sets):
    """The distinct bins of these Labels (one or both maps) in their order: -> [(start, end, gene)]."""
    return sorted({lab[1] for labels in label_sets for lab in labels.labels if lab is not None and lab != SHARED})


class MapLabels(object):
    """A bin map by its definition (code[k] holds for start[k] <= p < start[k + 1], the last entry to the end, 0 below start[0]) with
    the bins' genes: the key of a bin is its number."""

    def __init__(self, start, code, bin_gene):
        self.bases, self.bin_gene = G.bases_of_map(start, code), [int(g) for g in bin_gene]

    def at(self, p):
        c = self.bases.at(p)
        return None if c == 0 else SHARED if c == G.MANY else (self.bin_gene[c - 1], c - 1)


# ---- a read -----------------------------------------------------------------------------------------------------------------------
def read_of(flag, pos, ops, labels, stranded=0, shift=0):
    """labels: a Labels / MapLabels (unstranded) or {'+': ..., '-': ...} -> (verdict, the keys of the bins that get + 1, in order)."""
    if not G.eligible(flag, pos, len(ops)):
        return NOT_COUNTED, []
    mine = labels[G.read_strand(flag, stranded)] if stranded else labels
    hits, seen, genes, shared = [], set(), set(), False
    for s, e in G.blocks_of(pos, ops, shift):
        for p in range(s, e):
            lab = mine.at(p)
            if lab is None:
                continue
            if lab == SHARED:
                shared = True
            elif lab[1] not in seen:
                seen.add(lab[1])
                hits.append(lab[1])
                genes.add(lab[0])
    if shared or len(genes) > 1:
        return AMBIGUOUS, []
    return (COUNTED, hits) if hits else (NO_FEATURE, [])


def reads_of(rs, labels, stranded=0, shift=0):
    """-> [(verdict, keys)] per read of a ReadSet.  (Equal reads are walked once: a hot bin has hundreds of thousands of them.)"""
    pos, flag, off, cig = rs.pos.tolist(), rs.flag.tolist(), rs.cig_off.tolist(), rs.cigar.tolist()
    memo, out = {}, []
    for i in range(len(pos)):
        key = (flag[i], pos[i], tuple(cig[off[i]:off[i + 1]]))
        if key not in memo:
            memo[key] = read_of(key[0], key[1], key[2], labels, stranded, shift)
        out.append(memo[key])
    return out


def counts_of(results, number_of, n_bins, keep=None):
    """-> n_bins + 4 numbers: the bins' reads, then counted, no feature, ambiguous, not counted.  number_of: key -> bin number (None:
    the keys are numbers)."""
    out = [0] * (n_bins + 4)
    for i, (verdict, keys) in enumerate(results):
        if keep is not None and not keep[i]:
            continue
        out[n_bins - verdict] += 1
        for key in keys:
            out[key if number_of is None else number_of[key]] += 1
    return out


def adds_of(results, wave=64):
    """The 64-bit adds of the commit's round rule for these reads in this order: in round j every lane of a wave offers its j-th bin
    or nothing, and every run of equal bins in lane order is one add (a lane with nothing ends a run).  -> (adds, naive): naive is
    one add per (read, bin)."""
    adds = naive = 0
    for base in range(0, len(results), wave):
        lists = [keys for _, keys in results[base:base + wave]]
        naive += sum(len(k) for k in lists)
        for j in range(max([len(k) for k in lists] + [0])):
            before = None
            for k in lists:
                cur = k[j] if j < len(k) else None
                if cur is not None and cur != before:
                    adds += 1
                before = cur
    return adds, naive


# ---- the two files ----------------------------------------------------------------------------------------------------------------
def rows_of(ids, chroms, bins_by_chrom, only=None):
    """The rows of both files in their order -- gene ids sorted, then the bin's rank within its gene over the chromosomes of
    ``chroms`` (the annotation's order of first appearance), then (start, end): -> [(id, gene id, chrom, start, end, bin number)];
    ``only``: the rows of that chromosome, under the same ids."""
    rows = []
    for g, gene in enumerate(ids):
        rank = 0
        for chrom in chroms:
            for number, (start, end, bin_gene) in enumerate(bins_by_chrom.get(chrom, [])):
                if bin_gene == g:
                    rank += 1
                    if only is None or chrom == only:
                        rows.append(("%s:%03d" % (gene, rank), gene, chrom, start, end, number))
    return rows


def bins_text(rows):
    return "id\tgene\tchrom\tstart\tend\n" + "".join("%s\t%s\t%s\t%d\t%d\n" % (r[0], r[1], r[2], r[3] + 1, r[4]) for r in rows)


def counts_text(rows, counts_by_chrom, verdicts):
    """counts_by_chrom: {chrom: the bins' reads}, a chromosome that is not there has none; verdicts: counted, no feature, ambiguous,
    not counted."""
    text = "".join("%s\t%d\n" % (r[0], counts_by_chrom[r[2]][r[5]] if r[2] in counts_by_chrom else 0) for r in rows)
    return text + "".join("%s\t%d\n" % (name, verdicts[k + 1]) for k, name in enumerate(SPECIALS))
