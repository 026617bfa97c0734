"""Shared by the tests of ``exoncounts --countReadPairs``: the yardstick -- which bins a FRAGMENT counts for -- restated in plain
loops from the rule's text, on top of ``exoncases`` (what lies under every base) and ``matecases`` (the mate table, the paired
generator).  Per leader: the SET of bin keys under the bases of both reads, each read on the labels of its own strand.  Nothing here
knows of walks, heads or merges; nothing here imports ``spliser_amd/exoncounts.py`` or calls the library; nothing touches the GPU.

The rule.  Mates, pairable reads, groups and the leader are ``matecases``'; eligibility, blocks and what lies under a base are
``exoncases``'.  A read that is not eligible is not counted, one per read.  An eligible read whose mate has a lower index is silent.
Every other eligible read: the labels under its own bases on its own strand's labels and, if it has a mate, under the mate's bases
on the labels of the mate's strand (by the mate's own flag).  Any base shared, or bins of two genes: ambiguous, no bin incremented;
no bin: no feature; otherwise counted, every DISTINCT bin + 1."""
import exoncases as X
import genecases as G
import matecases as M

SILENT = M.SILENT
COUNTED, NO_FEATURE, AMBIGUOUS, NOT_COUNTED = X.COUNTED, X.NO_FEATURE, X.AMBIGUOUS, X.NOT_COUNTED


def under(flag, pos, ops, labels, stranded=0, shift=0):
    """-> ({bin key: its gene} under the blocks of one read on the labels of its own strand, whether a base is shared)."""
    mine = labels[G.read_strand(flag, stranded)] if stranded else labels
    bins, shared = {}, False
    for s, e in G.blocks_of(pos, ops, shift):
        for p in range(s, e):
            lab = mine.at(p)
            if lab is None:
                continue
            if lab == X.SHARED:
                shared = True
            else:
                bins[lab[1]] = lab[0]
    return bins, shared


def fragment_results(rs, keys, labels, stranded=0, shift=0, mate=None):
    """Per read: (verdict | SILENT, the keys of the bins that get + 1, sorted)."""
    pos, flag, off, cig = rs.pos.tolist(), rs.flag.tolist(), rs.cig_off.tolist(), rs.cigar.tolist()
    if mate is None:
        mate = M.mate_table_of(rs, keys)[0]
    out = []
    for i in range(len(pos)):
        ops = cig[off[i]:off[i + 1]]
        if not G.eligible(flag[i], pos[i], len(ops)):
            out.append((NOT_COUNTED, []))
            continue
        m = mate[i]
        if m != M.NONE and m < i:
            out.append((SILENT, []))
            continue
        bins, shared = under(flag[i], pos[i], ops, labels, stranded, shift)
        if m != M.NONE:
            more, shared2 = under(flag[m], pos[m], cig[off[m]:off[m + 1]], labels, stranded, shift)
            bins.update(more)
            shared = shared or shared2
        if shared or len(set(bins.values())) > 1:
            out.append((AMBIGUOUS, []))
        elif bins:
            out.append((COUNTED, sorted(bins)))
        else:
            out.append((NO_FEATURE, []))
    return out


def counts_of(results, number_of, n_bins, keep=None):
    """-> n_bins + 4 numbers: the bins' fragments, then counted, no feature, ambiguous, not counted; a silent read adds nothing."""
    out = [0] * (n_bins + 4)
    for i, (verdict, keys) in enumerate(results):
        if verdict == SILENT or (keep is not None and not keep[i]):
            continue
        out[n_bins - verdict] += 1
        for key in keys:
            out[key if number_of is None else number_of[key]] += 1
    return out


def adds_of(results, wave=64):
    """``exoncases.adds_of`` over the fragments' lists: a silent lane offers nothing in any round (and ends a run).  The keys must be
    in the order the kernel gives them, ascending bin number: number them first.  -> (adds, one add per (fragment, bin))."""
    return X.adds_of([(v, keys if v == COUNTED else []) for v, keys in results], wave)


def numbered(results, number_of):
    """The results with every key replaced by its bin number, ascending."""
    return [(v, sorted(number_of[k] for k in keys)) for v, keys in results]


# ---- the hand cases: a chromosome whose answers can be read off the rule -------------------------------------------------------------
HAND_LENGTH = 3000
MANY_BINS = 75                     # gene 6: abutting exons of 10 bases from 2000, a bin each
HAND_FEATURES = ([(100, 200, "+", 0), (200, 300, "+", 0), (300, 350, "+", 0), (400, 500, "+", 0),        # gene 0: three abutting bins and one apart
                  (600, 700, "+", 1),                                                                    # gene 1
                  (800, 900, "+", 2), (850, 950, "+", 3),                                                # 850..900 is shared
                  (1100, 1200, ".", 4),                                                                  # in both maps of a stranded run: one bin
                  (1300, 1400, "-", 5), (1400, 1500, "-", 5)]                                            # the '-' map's alone
                 + [(2000 + 10 * k, 2010 + 10 * k, "+", 6) for k in range(MANY_BINS)])
A, B, C, D = (100, 200, 0), (200, 300, 0), (300, 350, 0), (400, 500, 0)
DOT, M1, M2 = (1100, 1200, 4), (1300, 1400, 5), (1400, 1500, 5)
MANY = [(2000 + 10 * k, 2010 + 10 * k, 6) for k in range(MANY_BINS)]
LONG = "%dM" % (10 * MANY_BINS)
# name: (the leader (flag, POS, CIGAR), its mate, the answer unstranded, the answer under fr) -- an answer: (verdict, the bins that get + 1)
HAND_CASES = {
    "both mates wholly in one bin: + 1, not + 2": ((99, 121, "30M"), (147, 141, "30M"), (COUNTED, [A]), (COUNTED, [A])),
    "mates overlapping in one bin, each reaching a neighbour: three bins": ((99, 181, "40M"), (147, 281, "40M"), (COUNTED, [A, B, C]), (COUNTED, [A, B, C])),
    "disjoint bins of one gene": ((99, 121, "30M"), (147, 421, "30M"), (COUNTED, [A, D]), (COUNTED, [A, D])),
    "bins of two genes": ((99, 121, "30M"), (147, 621, "30M"), (AMBIGUOUS, []), (AMBIGUOUS, [])),
    "one mate on a shared piece": ((99, 811, "20M"), (147, 861, "20M"), (AMBIGUOUS, []), (AMBIGUOUS, [])),
    "the leader on a shared piece": ((99, 861, "20M"), (147, 911, "20M"), (AMBIGUOUS, []), (AMBIGUOUS, [])),
    "one mate nowhere": ((99, 121, "30M"), (147, 1701, "30M"), (COUNTED, [A]), (COUNTED, [A])),
    "the leader nowhere": ((99, 1701, "30M"), (147, 1901, "200M"), (COUNTED, MANY[:10]), (COUNTED, MANY[:10])),
    "both nowhere": ((99, 1701, "30M"), (147, 1751, "30M"), (NO_FEATURE, []), (NO_FEATURE, [])),
    "a deletion and an intron inside a bin on one mate": ((99, 111, "10M5D10M20N10M"), (147, 141, "30M"), (COUNTED, [A]), (COUNTED, [A])),
    "65 / 129 under a . feature: different maps, one bin": ((65, 1111, "30M"), (129, 1131, "30M"), (COUNTED, [DOT]), (COUNTED, [DOT])),
    "83 / 163 on the - map": ((83, 1321, "30M"), (163, 1421, "30M"), (COUNTED, [M1, M2]), (COUNTED, [M1, M2])),
    "99 / 147 over the - gene": ((99, 1321, "30M"), (147, 1421, "30M"), (COUNTED, [M1, M2]), (NO_FEATURE, [])),
    "65 / 129 over + bins: the second mate sees the other map": ((65, 121, "30M"), (129, 421, "30M"), (COUNTED, [A, D]), (COUNTED, [A])),
    "a mate over 70 bins, a one-bin leader": ((99, 2001, "5M"), (147, 2001, LONG), (COUNTED, MANY), (COUNTED, MANY)),
    "a leader over 70 bins, a one-bin mate": ((99, 2001, LONG), (147, 2741, "5M"), (COUNTED, MANY), (COUNTED, MANY)),
}
FILLER = (4, 1, "")                 # an unmapped read: between the mates, and counted as "not counted"


def hand_set(names, spread=0, lead_at=0):
    """The cases ``names`` one after the other, ``spread`` fillers between a case's mates, ``lead_at`` fillers in front of all:
    -> (records, keys: a key per case, 0 for the fillers, where: the index of every case's leader)."""
    records, keys, where = [FILLER] * lead_at, [0] * lead_at, []
    for k, name in enumerate(names):
        lead, mate = HAND_CASES[name][:2]
        where.append(len(records))
        records += [lead] + [FILLER] * spread + [mate]
        keys += [2 * k + 2] + [0] * spread + [2 * k + 2]
    return records, keys, where
