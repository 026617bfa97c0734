"""Shared by the tests of ``strandedness`` / ``-s auto``: the yardstick -- the per-read rule, the cover map's per-position code, the
decision and the report's grammar, restated here in plain loops over records and genes from the issue's text -- and the synthetic
libraries the command tests run on.  Nothing here calls the library or ``spliser_amd/strandedness.py``; nothing touches the GPU."""
import bisect

import numpy as np

from spliser_amd import samio

PLUS, MINUS = ord("+"), ord("-")
REF_OPS = (0, 2, 3, 7, 8)           # M D N = X: the ops that consume the reference


# ---- section 1: the per-read rule -------------------------------------------------------------------------------------------
def fr_strand(flag):
    """check_strand for "fr": a first or unpaired read has its own strand, a second read the opposite one."""
    first = bool(flag & 64) or not (flag & 1)
    reverse = bool(flag & 16)
    minus = reverse if first else not reverse
    return MINUS if minus else PLUS


def mate_class(flag):
    if not flag & 1:
        return 0
    return 1 if flag & 0x40 else 2


def map_evidence(pos, ops, starts, codes):
    """starts (a list, ascending) / codes: the cover map -> PLUS, MINUS or 0 for a read at pos with these ops."""
    ref_len = 0
    for op in ops:
        if (int(op) & 15) in REF_OPS:
            ref_len += int(op) >> 4
    if ref_len < 1 or not len(starts):
        return 0
    k = bisect.bisect_right(starts, pos) - 1      # the last entry with start <= pos
    if k < 0:
        return 0
    if k + 1 < len(starts) and pos + ref_len - 1 >= starts[k + 1]:
        return 0
    return {1: PLUS, 2: MINUS}.get(int(codes[k]), 0)


def add_read(out, flag, pos, ops, xs, starts=(), codes=()):
    out[0] += 1
    if flag & (0x4 | 0x100 | 0x200 | 0x800):
        return
    out[1] += 1
    m, fr = mate_class(flag), fr_strand(flag)
    if xs in (PLUS, MINUS):
        out[2 + 2 * m + (0 if fr == xs else 1)] += 1
    ev = map_evidence(pos, ops, starts, codes)
    if ev:
        out[8 + 2 * m + (0 if fr == ev else 1)] += 1


def tally(rs, xs=None, cover=None, keep=None):
    """The 14 numbers of a ReadSet (``keep``: a mask of the reads that are there at all)."""
    out = [0] * 14
    starts, codes = ([], []) if cover is None else (np.asarray(cover[0]).tolist(), np.asarray(cover[1]).tolist())
    pos, flag, off, cig = rs.pos.tolist(), rs.flag.tolist(), rs.cig_off.tolist(), rs.cigar.tolist()
    bytes_ = None if xs is None else np.asarray(xs).tolist()
    for i in range(len(pos)):
        if keep is not None and not keep[i]:
            continue
        add_read(out, flag[i], pos[i], cig[off[i]:off[i + 1]], 0 if bytes_ is None else bytes_[i], starts, codes)
    return out


# ---- section 2: the cover map -----------------------------------------------------------------------------------------------
def code_at(genes, p):
    """genes: [(left, right, strand text)] as the GFF reader has them (left = column 4 - 1, right = column 5); p: 1-based."""
    code = 0
    for left, right, strand in genes:
        if left + 1 <= p <= right:
            code |= 1 if strand == "+" else 2 if strand == "-" else 0
    return code


def map_code_at(starts, codes, p):
    code = 0
    for s, c in zip(starts, codes):
        if s <= p:
            code = c
    return code


def cover_of_genes(genes):
    """The map by its definition: walk every position, emit an entry where the code changes."""
    end = max([r for _, r, _ in genes] + [0]) + 2
    starts, codes, last = [], [], 0
    for p in range(0, end + 1):
        c = code_at(genes, p)
        if c != last:
            starts.append(p)
            codes.append(c)
            last = c
    return np.asarray(starts, np.int32), np.asarray(codes, np.uint8)


# ---- section 5: the decision and the report -----------------------------------------------------------------------------------
def source_verdict(a, b, min_evidence=1000):
    n = a + b
    if n < min_evidence:
        return "none"
    if 10 * a >= 9 * n:
        return "fr"
    if 10 * a <= n:
        return "rf"
    if 4 * n <= 10 * a and 10 * a <= 6 * n:
        return "unstranded"
    return "undetermined"


def verdict(out, min_evidence=1000):
    said = []
    for first in (2, 8):
        v = source_verdict(out[first] + out[first + 2] + out[first + 4], out[first + 1] + out[first + 3] + out[first + 5], min_evidence)
        if v != "none":
            said.append(v)
    if not said:
        return "undetermined (too little evidence)"
    if len(said) == 2 and said[0] != said[1]:
        return "undetermined (tags and annotation disagree)"
    return said[0]


def parse_report(text):
    """-> (the 14 numbers, {source: (fraction text, verdict)}, verdict, note lines) from the tab-separated text."""
    out, per, final, notes = [0] * 14, {}, None, []
    lines = text.split("\n")
    assert lines[-1] == "" and lines[-2].startswith("verdict\t")
    for line in lines[:-1]:
        cols = line.split("\t")
        if cols[0] == "reads seen":
            out[0] = int(cols[1])
        elif cols[0] == "reads eligible":
            out[1] = int(cols[1])
        elif cols[0] in ("tags", "annotation"):
            first = 2 if cols[0] == "tags" else 8
            if cols[1] == "all":
                per[cols[0]] = (int(cols[2]), int(cols[3]), cols[4], cols[5])
            else:
                m = ("unpaired", "first", "second").index(cols[1])
                out[first + 2 * m], out[first + 2 * m + 1] = int(cols[2]), int(cols[3])
        elif cols[0] == "verdict":
            final = cols[1]
        else:
            assert cols[0] == "note", line
            notes.append(cols[1])
    return out, per, final, notes


# ---- synthetic libraries ----------------------------------------------------------------------------------------------------
NAMES, LENGTHS = ["c1", "c2"], [100000, 100000]
GENES = {        # (left, right, strand): gaps, abutting / overlapping / nested genes of one strand, overlaps of both, a gene without a strand
    "c1": [(500, 8000, "+"), (7000, 15000, "+"), (18000, 28000, "-"), (27000, 35000, "+"), (38000, 50000, "-"), (52000, 57000, "."),
           (60000, 75000, "+"), (63000, 66000, "+")],
    "c2": [(1000, 22000, "-"), (22000, 45000, "+"), (46000, 50000, "-"), (52000, 80000, "-")],
}
FLAGS_BY_STRAND = {PLUS: (0, 99, 147), MINUS: (16, 83, 163)}      # flags whose fr strand is + / -


def write_gff(path, genes=GENES, flip=False):
    swap = {"+": "-", "-": "+", ".": "."}
    with open(path, "w") as fh:
        fh.write("##gff-version 3\n")
        for chrom in NAMES:
            for k, (left, right, strand) in enumerate(genes[chrom]):
                fh.write("%s\tsynth\tgene\t%d\t%d\t.\t%s\t.\tID=%s_g%d;Name=%s_g%d\n" % (chrom, left + 1, right, swap[strand] if flip else strand, chrom, k, chrom, k))


def library(p, seed, n_per_gene=450, with_xs=True):
    """Reads inside genes whose fr strand equals the gene's strand with probability p; six in ten spliced over a few junctions of
    their gene, with XS:A equal to the gene's strand (``with_xs``).  -> (sets [(chrom, ReadSet)], tags per set, strand bytes per set)."""
    rng = np.random.default_rng(seed)
    sets, tags, xs = [], [], []
    for chrom in NAMES:
        recs = []
        for left, right, strand in GENES[chrom]:
            if strand == ".":
                continue
            g = PLUS if strand == "+" else MINUS
            donors = rng.integers(left + 200, right - 2000, 4)
            for _ in range(n_per_gene):
                same = rng.random() < p
                flag = int(rng.choice(FLAGS_BY_STRAND[g if same else (PLUS if g == MINUS else MINUS)]))
                if rng.random() < 0.6:
                    d = int(donors[int(rng.integers(0, 4))])
                    a, b = int(rng.integers(10, 60)), int(rng.integers(10, 60))
                    recs.append((d - a + 1, flag, "%dM%dN%dM" % (a, 100 + int(d % 7) * 100, b), g))
                else:
                    pos = int(rng.integers(left + 1, right - 120))
                    recs.append((pos, flag, "%dM" % int(rng.integers(40, 101)), 0))
        recs.sort(key=lambda r: r[0])
        sets.append((chrom, samio.ReadSet.from_records([(f, pos, c) for pos, f, c, _ in recs])))
        tags.append([(b"NHC\x01XSA" + bytes([g])) if (g and with_xs) else b"NHC\x01" for _, _, _, g in recs])
        xs.append(np.asarray([g if with_xs else 0 for _, _, _, g in recs], np.uint8))
    return sets, tags, xs


_COVERS = {}


def library_cover(chrom, flip=False):
    """The yardstick's cover map of a chromosome of GENES (made once: it walks every position)."""
    if (chrom, flip) not in _COVERS:
        swap = {"+": "-", "-": "+", ".": "."}
        _COVERS[(chrom, flip)] = cover_of_genes([(l, r, swap[s] if flip else s) for l, r, s in GENES[chrom]])
    return _COVERS[(chrom, flip)]


def library_tally(sets, xs, annotated=True, flip=False, keep=None):
    out = [0] * 14
    for k, ((chrom, rs), x) in enumerate(zip(sets, xs)):
        cover = library_cover(chrom, flip) if annotated else None
        out = [a + b for a, b in zip(out, tally(rs, x, cover, None if keep is None else keep[k]))]
    return out
