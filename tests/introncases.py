"""Shared by the tests of ``intronretention``: the yardstick -- the introns of an annotation, their measurable pieces, the trimmed
depth, the splice counts, the ratio and the file -- restated in plain loops from the issue's text.  Per base it keeps the set of
covering features; a gene's introns are the runs of bases its features leave open between bases they cover; the depth under the
measurable bases is expanded base by base and sorted; the splice sums are a loop over the junction rows.  Nothing here knows of
cuts, searches or histograms; nothing here imports ``spliser_amd/intronretention.py`` or calls the library; nothing touches the
GPU."""
HEADER = "id\tgene\tchrom\tstart\tend\tstrand\tmeasurable\tcovered\tdepth_n\tdepth_sum\tdepth\tsplice_left\tsplice_right\tsplice_exact\tIRratio\n"


def tracks_of(stranded):
    return ["+", "-"] if stranded else ["."]


def select(features, track):
    """features: [(left, right, strand text, gene index)].  Track '.': all; '+': those whose strand is not '-'; '-': not '+'.  Only
    features with a base (right > left; a base below 0 is none)."""
    out = []
    for left, right, strand, gene in features:
        left = max(left, 0)
        if right <= left:
            continue
        if track == "." or strand != {"+": "-", "-": "+"}[track]:
            out.append((left, right, strand, gene))
    return out


def introns_of(features, track, length=None):
    """The introns of one chromosome's features on one track: -> [(gene, s, e, [(ps, pe)])] sorted by (gene, s).  ``length``: the
    pieces keep only bases below it (None: all)."""
    chosen = select(features, track)
    if not chosen:
        return []
    extent = max(f[1] for f in chosen)
    under = [set() for _ in range(extent)]              # the features over every base
    for k, (left, right, _, _) in enumerate(chosen):
        for p in range(left, right):
            under[p].add(k)
    out = []
    for gene in sorted({f[3] for f in chosen}):
        mine = {k for k, f in enumerate(chosen) if f[3] == gene}
        covered = [bool(under[p] & mine) for p in range(extent)]
        first, last = covered.index(True), extent - 1 - covered[::-1].index(True)
        p = first
        while p <= last:
            if covered[p]:
                p += 1
                continue
            s = p
            while not covered[p]:
                p += 1
            pieces, at = [], None
            for q in range(s, p):
                free = not under[q] and (length is None or q < length)
                if free and at is None:
                    at = q
                if not free and at is not None:
                    pieces.append((at, q))
                    at = None
            if at is not None:
                pieces.append((at, p))
            out.append((gene, s, p, pieces))
    return out


def depth_per_base(bound_pos, bound_depth, length):
    """Boundaries by their definition: depth[k] holds for pos[k] <= p < pos[k + 1], the last to the end, 0 before the first."""
    out = [0] * length
    for k in range(len(bound_pos)):
        stop = bound_pos[k + 1] if k + 1 < len(bound_pos) else length
        for p in range(max(int(bound_pos[k]), 0), min(int(stop), length)):
            out[p] = int(bound_depth[k])
    return out


def stats_of(depth, pieces, trim):
    """depth: per base (anything indexable) -> (L, covered, depth_n, depth_sum) of one intron's pieces."""
    d = sorted(int(depth[p]) for ps, pe in pieces for p in range(ps, pe))
    lo = (len(d) * trim) // 100
    hi = len(d) - lo
    return len(d), sum(1 for v in d if v > 0), hi - lo, sum(d[lo:hi])


def stats_of_runs(bound_pos, bound_depth, pieces, trim):
    """The same from boundaries, without a per-base array of the whole reference: the pieces' bases one by one."""
    d = []
    for ps, pe in pieces:
        for p in range(ps, pe):
            v = 0
            for k in range(len(bound_pos)):
                if int(bound_pos[k]) <= p:
                    v = int(bound_depth[k])
                else:
                    break
            d.append(v)
    d.sort()
    lo = (len(d) * trim) // 100
    hi = len(d) - lo
    return len(d), sum(1 for v in d if v > 0), hi - lo, sum(d[lo:hi])


def splice_of(junction_rows, s, e, track, stranded):
    """junction_rows: [(left, right, strand text, count)] -> (splice_left, splice_right, splice_exact)."""
    left = right = exact = 0
    for l, r, strand, count in junction_rows:
        if stranded and strand != track:
            continue
        if l == s:
            left += count
        if r == e:
            right += count
        if l == s and r == e:
            exact += count
    return left, right, exact


def ratio_texts(depth_n, depth_sum, splice_left, splice_right):
    if depth_n == 0:
        return "NA", "NA"
    depth = depth_sum / depth_n
    below = depth + max(splice_left, splice_right)
    return repr(depth), ("NA" if below == 0 else repr(depth / below))


def rows_of(ids, chroms, by_chrom, stranded, trim, lengths, depths, junctions, only=None):
    """ids: the sorted gene ids; chroms: the annotation's chromosomes in its order; by_chrom: {chrom: features}; lengths: {chrom:
    length} (a chromosome without one clips nothing); depths: {(chrom, track): per-base depth} (none: no read); junctions: {chrom:
    rows}.  -> the file's rows as tuples of texts, in the file's order; ``only``: that chromosome's rows, under the same ids."""
    found = []
    for c, chrom in enumerate(chroms):
        for t, track in enumerate(tracks_of(stranded)):
            for gene, s, e, pieces in introns_of(by_chrom[chrom], track, lengths.get(chrom)):
                found.append((gene, c, s, e, t, chrom, track, pieces))
    found.sort(key=lambda r: r[:5])
    rows, rank, before = [], 0, None
    for gene, _, s, e, _, chrom, track, pieces in found:
        rank = rank + 1 if gene == before else 1
        before = gene
        if only is not None and chrom != only:
            continue
        depth = depths.get((chrom, track))
        if depth is None:
            n = sum(pe - ps for ps, pe in pieces)
            stats = (n, 0, n - 2 * ((n * trim) // 100), 0)
        else:
            stats = stats_of(depth, pieces, trim)
        splice = splice_of(junctions.get(chrom, []), s, e, track, stranded)
        rows.append(("%s:I%03d" % (ids[gene], rank), ids[gene], chrom, str(s + 1), str(e), track) + tuple(str(v) for v in stats) +
                    (ratio_texts(stats[2], stats[3], splice[0], splice[1])[0],) + tuple(str(v) for v in splice) +
                    (ratio_texts(stats[2], stats[3], splice[0], splice[1])[1],))
    return rows


def file_text(rows):
    return HEADER + "".join("\t".join(r) + "\n" for r in rows)


def random_bounds(rng, length, n, max_depth=40):
    """n boundaries (fewer when the positions collide) on [0, length): strictly ascending positions, any depths, zeros among them."""
    pos = sorted({int(v) for v in rng.integers(0, length, n)})
    depth = [0 if rng.random() < 0.2 else int(rng.integers(1, max_depth + 1)) for _ in pos]
    return pos, depth


def random_pieces(rng, length, n):
    """Up to n disjoint ascending pieces on [0, length]."""
    cuts = sorted({int(v) for v in rng.integers(0, length + 1, 2 * n)})
    return [(cuts[k], cuts[k + 1]) for k in range(0, len(cuts) - 1, 2)]


def body_cases():
    """What a team's body can get wrong, as (name, bound_pos, bound_depth, [pieces of each intron], length): the tests of the body
    under the wave emulator and those of the kernel on the device both run them."""
    import numpy as np
    cases = []
    for inside in (0, 1, 63, 64, 65, 4097):           # a boundary before the piece whose depth enters it, `inside` boundaries in it
        rng = np.random.default_rng(inside)
        cases.append(("%d boundaries inside" % inside, [40] + [101 + 2 * k for k in range(inside)], [7] + [int(v) for v in rng.integers(0, 30, inside)],
                      [[(100, 100 + 2 * inside + 50)]], 100 + 2 * inside + 200))
    cases.append(("no boundary inside, at depth 0 and above", [50, 90, 200], [9, 0, 4], [[(10, 40)], [(100, 150)], [(55, 80)], [(300, 1000)]], 1000))
    cases.append(("no boundary at all", [], [], [[(0, 10)], [(5, 6), (8, 20)], []], 20))
    cases.append(("a piece that starts or ends on a boundary", [100, 110, 120, 130], [1, 2, 3, 0],
                  [[(100, 110)], [(110, 130)], [(105, 120)], [(90, 100)], [(120, 121)], [(129, 131)], [(130, 140)]], 200))
    for n_pieces in (64, 65, 200):                    # as many pieces as shared memory keeps, and more
        rng = np.random.default_rng(n_pieces)
        pos, depth = random_bounds(rng, 40 * n_pieces, 3 * n_pieces)
        pieces = [(40 * k + int(rng.integers(0, 10)), 40 * k + int(rng.integers(11, 40))) for k in range(n_pieces)]
        cases.append(("%d pieces" % n_pieces, pos, depth, [pieces, pieces[:3], pieces[1:]], 40 * n_pieces))
    for name, values in (("the top byte", [k << 24 for k in (1, 200, 3, 255, 17)]), ("the bottom byte", [0x01020300 | k for k in (9, 0, 255, 31, 128)]),
                         ("whole bytes", [0xFFFFFFFF, 0xFFFFFF00, 0xFF000000, 0x00FFFFFF])):
        pos = list(range(0, 400, 4))
        cases.append(("depths that differ in " + name, pos, [values[k % len(values)] for k in range(len(pos))], [[(0, 400)], [(3, 77), (100, 333)]], 400))
    cases.append(("both ranks on one value, or in different buckets", [0, 10, 90], [1, 5, 70000], [[(0, 100)]], 100))
    cases.append(("ties that straddle lo and hi", [0, 3, 7], [2, 9, 300], [[(0, 10)]], 10))
    cases.append(("rank values in different buckets of the top byte", [0, 2, 4, 6, 8], [5, 0x02000000, 0x10000007, 0xF0000000, 0x0F000000], [[(0, 10)], [(1, 9)]], 10))
    cases.append(("few bases", [0, 1, 2], [4, 0, 6], [[], [(0, 1)], [(0, 2)], [(0, 3)], [(1, 2)], [(2, 3)], [(0, 1), (2, 3)]], 3))
    cases.append(("the greatest depth", [0, 1000], [2 ** 32 - 1, 0], [[(0, 1000)], [(500, 1200)]], 1200))
    return cases


def junction_rows(rs, stranded=0, keep=None):
    """The junction table of a ReadSet by a walk over every read's ops: an N op over the 0-based bases [s, e) of a mapped read is
    the junction (left = s, right = e); under a stranded run its strand is the read's (check_strand's rule), else '?'.  -> [(left,
    right, strand text, count)], sorted."""
    table = {}
    pos, flag, off, cig = rs.pos.tolist(), rs.flag.tolist(), rs.cig_off.tolist(), rs.cigar.tolist()
    for i in range(len(pos)):
        if (keep is not None and not keep[i]) or flag[i] & 4 or pos[i] < 1:
            continue
        strand = "?"
        if stranded:
            first = bool(flag[i] & 64) or not (flag[i] & 1)
            reverse = bool(flag[i] & 16)
            minus = reverse if first else not reverse
            strand = "-" if minus != (stranded == 2) else "+"
        p = pos[i] - 1
        for op in cig[off[i]:off[i + 1]]:
            code, n = op & 15, op >> 4
            if code == 3 and n:
                table[(p, p + n, strand)] = table.get((p, p + n, strand), 0) + 1
            if code in (0, 2, 3, 7, 8):
                p += n
    return sorted(k + (v,) for k, v in table.items())
