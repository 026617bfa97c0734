"""Inputs and expectations for the tests of ``process_sites``' planning (``spliser_amd/process.py``): which shards a context's
chromosomes are packed into before the reads are known, the second plan after a read reached beyond its slot, the counting of one
chromosome on several contexts after a decode in shares.  No tests in here, and no GPU: test_plancases_host.py checks that every
world reaches what it names, test_gpu_process_plans.py runs them.

A WORLD is a handful of references whose header lengths are chosen for what ``shard.pack`` makes of them -- a BAM header may claim
any length below 2^31 and the first plan believes it --, a few hundred to 1 500 reads per reference at two loci (around position
1 000 and at the reference's true end), a BED file made from the reads' own junctions, and the files.  Every world also has a
reference the BED knows and the BAM lacks (``ghost``, first in the BED: the writer waits for it) and one the BAM has without reads
(``empty``, last in the header).  The expectation is the oracle's, per chromosome in the chromosome's own coordinates: sharding does
not enter it.

A locus is four exons with the junctions 1-2, 2-3, 3-4, the skip 1-3 and an alternative end of exon 2 (``JUNCTIONS``), so that its
sites have competitors; the reads over it (``TEMPLATES``) are one-op reads across every site, ``M N M`` reads over every junction and
``M N M N M`` reads over three pairs of them: beta1, beta2Simple and the double counts are all non-zero.  The first locus of a reference
is on '+' (flags 0, 99, 147 under ``fr``), the second on '-' (16, 83, 163); the one-op reads carry all six."""
import collections
import struct

import numpy as np

import ordercases
from spliser_amd import samio, shard, sites, tsv

M, N, S = 0, 3, 4
SLACK = 1 << 20       # what process_sites' first plan adds to the header's LN
BLOCK = 3072          # BGZF blocks of 3 KiB of records: some sixty records each, so that a decode in shares has blocks to cut at

# (left, right) = (last base of the exon before, last base of the intron), relative to the locus' base
JUNCTIONS = [(99, 299), (399, 599), (99, 599), (699, 899), (379, 599)]
LAST_SITE = 899
TAIL_END = 1099       # the last read of a locus ends here: 200 bases past the locus' last site
# (relative POS, ops, weight)
TEMPLATES = [
    (50, [(100, M)], 6), (330, [(100, M)], 6), (550, [(100, M)], 6), (650, [(100, M)], 6), (850, [(100, M)], 6), (1000, [(100, M)], 2),
    (50, [(50, M), (200, N), (50, M)], 8), (350, [(50, M), (200, N), (50, M)], 8), (50, [(50, M), (500, N), (50, M)], 4),
    (650, [(50, M), (200, N), (50, M)], 8), (330, [(50, M), (220, N), (50, M)], 4),
    (50, [(50, M), (200, N), (100, M), (200, N), (50, M)], 6), (350, [(50, M), (200, N), (100, M), (200, N), (50, M)], 6),
    (50, [(50, M), (500, N), (100, M), (200, N), (50, M)], 4),
]
PLUS_FLAGS, MINUS_FLAGS = (0, 99, 147), (16, 83, 163)

Ref = collections.namedtuple("Ref", "name ln end n spill", defaults=(0, 0, ()))
# name: in header and BED; ln: what the header says; end: where the last read ends (0: no reads); n: reads; spill: relative
# positions of further one-op reads BEYOND the second locus, which make no site (overhang_middle)

World = collections.namedtuple("World", "name refs names lengths sets so understated cg")


def _words(ops):
    return [(ln << 4) | code for ln, code in ops]


def _locus(rng, base, n, flags_spliced):
    """``n`` reads over the locus at ``base`` -> [(pos, flag, ops)]: every template once, the rest drawn by weight."""
    assert n >= len(TEMPLATES)
    weights = np.array([w for _, _, w in TEMPLATES], float)
    pick = list(range(len(TEMPLATES))) + rng.choice(len(TEMPLATES), size=n - len(TEMPLATES), p=weights / weights.sum()).tolist()
    out = []
    for k in pick:
        rel, ops, _ = TEMPLATES[k]
        if len(ops) == 1:       # (the tail read stays where it is: its end is the locus' end)
            out.append((base + rel + (0 if rel == 1000 else int(rng.integers(-20, 21))), int(rng.choice(PLUS_FLAGS + MINUS_FLAGS)), ops))
        else:
            out.append((base + rel, int(rng.choice(flags_spliced)), ops))
    return out


def _read_set(ref, seed):
    """The reads of one reference: half at the locus around 1 000 ('+'), half at the one that ends at ``ref.end`` ('-'), and the
    spill reads behind it, in coordinate order."""
    if not ref.n:
        return samio.ReadSet.empty()
    rng = np.random.default_rng(seed)
    base2 = ref.end - TAIL_END
    assert base2 > 1000 + TAIL_END + 1000
    recs = _locus(rng, 1000, ref.n // 2, PLUS_FLAGS) + _locus(rng, base2, ref.n - ref.n // 2, MINUS_FLAGS)
    recs += [(base2 + LAST_SITE + rel, int(rng.choice(PLUS_FLAGS + MINUS_FLAGS)), [(100, M)]) for rel in ref.spill]
    recs.sort(key=lambda r: r[0])
    off = np.concatenate(([0], np.cumsum([len(r[2]) for r in recs])))
    return samio.ReadSet(np.array([r[0] for r in recs], np.int64), np.array([r[1] for r in recs], np.int64), off,
                         np.array([w for r in recs for w in _words(r[2])], np.int64))


def junction_counts(rs):
    """{(left, right): reads} of a ReadSet, one count per N op, walked as checkBam walks a CIGAR (SpliSER_v0_1_8.py:457-483)."""
    out = collections.Counter()
    off = np.asarray(rs.cig_off, np.int64)
    for k in range(rs.n):
        cur = int(rs.pos[k])
        for w in rs.cigar[off[k]:off[k + 1]].tolist():
            d, code = w >> 4, w & 15
            if code in (0, 2, 3, 7, 8):
                cur += d
                if code == 3:
                    out[(cur - d - 1, cur - 1)] += 1
    return out


GHOST = [(1099, 1299, "+", 7), (1099, 1599, "+", 3), (1399, 1599, "+", 5)]       # the BED-only reference's junctions, with their read counts
EMPTY = [(1099, 1299, "-", 4), (1399, 1599, "-", 6), (1379, 1599, "-", 2)]       # those of the reference without reads


def write_bed(path, world, overhang=20):
    """The junctions of the world's reads (their strand: the locus'), regtools' twelve columns; ``ghost`` first, then header order."""
    rows = [("ghost",) + j for j in GHOST]
    for ref, rs in zip(world.refs, world.sets):
        if ref.n == 0:
            rows += [(ref.name,) + j for j in EMPTY]
            continue
        counts = junction_counts(rs)
        strands = {(l, r): st for l, r, st in world_junctions(ref)}
        assert set(counts) == set(strands)
        rows += [(ref.name, l, r, strands[(l, r)], counts[(l, r)]) for l, r in sorted(counts)]
    with open(path, "w") as fh:
        fh.write('track name=junctions description="plan worlds"\n')
        for i, (chrom, left, right, st, count) in enumerate(rows):
            start, end = left - overhang, right + overhang
            fh.write("%s\t%d\t%d\tJUNC%08d\t%d\t%s\t%d\t%d\t255,0,0\t2\t%d,%d\t0,%d\n" % (chrom, start, end, i + 1, count, st, start, end, overhang, overhang,
                                                                                   end - start - overhang))


def world_junctions(ref):
    base2 = ref.end - TAIL_END
    return [(1000 + l, 1000 + r, "+") for l, r in JUNCTIONS] + [(base2 + l, base2 + r, "-") for l, r in JUNCTIONS]


# Six references: two fill a shard of the int32 coordinate space by their header (LN 1e9 + 1 MiB twice is 2.002e9 of 2.147e9), the
# two of 5e8 make the third.  Read counts are uneven so that equal shares of the FILE cut inside c1 and c2 (three shares) and c1,
# c2 and c3 (five), and the last of three shares holds the rest of c2 and everything behind it: three shards on that context.
_BIG = [("c1", 10 ** 9, 990_000_000, 1500), ("c2", 10 ** 9, 990_000_000, 1500), ("c3", 10 ** 9, 990_000_000, 200), ("c4", 10 ** 9, 990_000_000, 200)]
_SPILL = (1024 + 1000 + 30, 1024 + 1000 + 310, 1024 + 1000 + 520, 1024 + 1000 + 640, 1024 + 1000 + 840)     # lands on the next reference's first locus
SPECS = {
    "three_shards": dict(refs=_BIG + [("c5", 5 * 10 ** 8, 400_000_000, 200), ("c6", 5 * 10 ** 8, 400_000_000, 200)]),
    "overhang_last": dict(refs=_BIG + [("c5", 5 * 10 ** 8, 400_000_000, 200), ("c6", 1000, 3_000_000, 200)], understated="c6"),
    # the understated reference first; c4's header overstates it, so that the exact plan has room for it in the first shard
    "overhang_first": dict(refs=[("c1", 1000, 3_000_000, 300), ("c2", 10 ** 9, 990_000_000, 300), ("c3", 10 ** 9, 990_000_000, 300),
                                 ("c4", 5 * 10 ** 8, 100_000_000, 300)], understated="c1"),
    "overhang_middle": dict(refs=[("c1", 10 ** 8, 99_000_000, 300), ("c2", 1000, 3_000_000, 300, _SPILL), ("c3", 10 ** 8, 99_000_000, 300)], understated="c2"),
    # one shard per context: six references of 3e8
    "cut": dict(refs=[("c%d" % (k + 1), 3 * 10 ** 8, 290_000_000, n) for k, n in enumerate((1500, 1500, 200, 200, 200, 200))]),
    "cut_overhang": dict(refs=_BIG + [("c5", 5 * 10 ** 8, 400_000_000, 200), ("c6", 1000, 3_000_000, 200)], understated="c6"),
    # ... and with a fifth reference that fills a shard with c4 to within 3e6 (1e9 + 1.144e9 + 2 MiB is 2.1461e9 of 2.1475e9), so that the last of three contexts has the understated reference in its THIRD shard: its
    # first, with the rest of c2, is counted and handed over before the overhang is found (the second shard's layout finds nothing)
    "cut_overhang_late": dict(refs=_BIG + [("c5", 1_144_000_000, 400_000_000, 200), ("c6", 1000, 3_000_000, 200)], understated="c6"),
    "cut_three_shards": dict(refs=_BIG + [("c5", 5 * 10 ** 8, 400_000_000, 200), ("c6", 5 * 10 ** 8, 400_000_000, 200)]),
    # cut's reads, the twice-spliced ones with their CIGAR parked in a CG tag: the device decoder hands such a file to the host threads
    "declined": dict(refs=[("c%d" % (k + 1), 3 * 10 ** 8, 290_000_000, n) for k, n in enumerate((1500, 1500, 200, 200, 200, 200))], cg=True),
    # three_shards, the second half of c1's records behind the last reference's
    "unsorted_three_shards": dict(refs=_BIG + [("c5", 5 * 10 ** 8, 400_000_000, 200), ("c6", 5 * 10 ** 8, 400_000_000, 200)], so="unsorted"),
}
NAMES = list(SPECS)
_SEEDS = {"cut_overhang": "overhang_last", "cut_overhang_late": "overhang_last", "cut_three_shards": "three_shards", "unsorted_three_shards": "three_shards", "declined": "cut"}


def world(name):
    spec = SPECS[name]
    refs = [Ref(*r) for r in spec["refs"]] + [Ref("empty", 5000)]
    seed0 = 20261021 + 100 * NAMES.index(_SEEDS.get(name, name))
    sets = [_read_set(ref, seed0 + k) for k, ref in enumerate(refs)]
    return World(name, refs, [r.name for r in refs], [r.ln for r in refs], sets, spec.get("so", "coordinate"), spec.get("understated"), bool(spec.get("cg")))


def _cg_record(rec):
    """A record whose CIGAR has five ops as htslib stores one of more than 65535: ``<l_seq>S<reference length>N`` in the record and
    the real ops in a CG:B,I tag (the writer's records have no SEQ: l_seq is 0)."""
    tid, pos, flag, mapq, ops, aux = rec
    if len(ops) < 5:
        return rec
    rlen = int(sum(int(w) >> 4 for w in ops if (int(w) & 15) in (0, 2, 3, 7, 8)))
    tag = b"CGBI" + struct.pack("<i", len(ops)) + np.asarray(ops, "<u4").tobytes()
    return (tid, pos, flag, mapq, np.array([(0 << 4) | S, (rlen << 4) | N], np.uint32), tag + aux)


def write_files(w, prefix):
    """``prefix``.bam and ``prefix``.bed of a world -> the records in the file's order."""
    recs = ordercases.records_of(w.sets)
    if w.cg:
        recs = [_cg_record(r) for r in recs]
    if w.so == "unsorted":      # file order: c1 (first half), c2 ... c6, c1 (second half)
        first = [r for r in recs if r[0] == 0]
        h = len(first) // 2
        recs = first[:h] + [r for r in recs if r[0] != 0] + first[h:]
    ordercases.write_bam(prefix + ".bam", w.names, w.lengths, recs, so=w.so, block=BLOCK)
    write_bed(prefix + ".bed", w)
    return recs


def table_of(bed, stranded):
    """Host Steps 0-2 over a BED file (golden-pinned), without an annotation."""
    table = sites.SiteTable(sites.GeneBins(), is_stranded=bool(stranded))
    table.add_bed(bed)
    table.find_competitors()
    return table


STRANDED_CODE = {None: 0, "fr": 1, "rf": 2}


def oracle_counts(oracle_lib, arr, rd, stranded, cryptic):
    """checkBam, then findBeta2Counts + calculateSSE, of one chromosome by the oracle -> the results dict and the double counts."""
    cnt = oracle_lib.check_bam(arr.pos, arr.strand, arr.part_off, arr.part_pos, arr.comp_off, arr.comp_pos, rd.pos, rd.flag, rd.cig_off, rd.cigar,
                               STRANDED_CODE[stranded], 0)
    b2s, b2c, b2w, sse = oracle_lib.beta2_sse(arr.pos, arr.part_off, arr.part_pos, arr.part_site, arr.alpha, arr.edge_cnt, cnt[0], cnt[1], cnt[2], cryptic)
    return dict(beta1=cnt[0], beta2_simple=b2s, beta2_cryptic=b2c, beta2_weighted=b2w, sse=sse), cnt[2]


def oracle_tsv(oracle_lib, bed, names, sets, stranded, cryptic, gff=None):
    """The .SpliSER.tsv text the reference's rules give for the reads ``sets`` (a ReadSet or None per entry of ``names``) and a BED
    file: host Steps 0-2 (golden-pinned), then the oracle per chromosome in the chromosome's own coordinates.  A chromosome of the
    BED that is not among ``names`` has no reads."""
    bins = sites.GeneBins.from_annotation(gff, "gene", "All") if gff else sites.GeneBins()
    table = sites.SiteTable(bins, is_stranded=bool(stranded))
    table.add_bed(bed)
    table.find_competitors()
    text = [tsv.HEADER]
    for chrom in table.chrom_index:
        arr = table.chrom_arrays(chrom)
        if arr.n == 0:
            continue
        rd = sets[names.index(chrom)] if chrom in names else None
        res, _ = oracle_counts(oracle_lib, arr, rd if rd is not None else samio.ReadSet.empty(), stranded, cryptic)
        text.extend(tsv.format_chrom(arr, res, cryptic))
    return "".join(text)


def plans(w, table, chroms=None):
    """What ``shard.pack`` makes of the world's chromosomes (``chroms``: those of one context; all otherwise), in the order
    process_sites gives them -- the file's, the BED-only reference last --: (first plan, exact plan), a list of Shards each.  First:
    room for ``LN`` + 1 MiB; exact: for the reads' largest end."""
    tid = {c: k for k, c in enumerate(w.names)}
    order = [c for c in table.chrom_index if (chroms is None or c in chroms) and table.chrom_arrays(c).n]
    order.sort(key=lambda c: tid.get(c, 1 << 30))
    items = [(c, table.chrom_arrays(c), None) for c in order]
    first = shard.pack(items, concat_reads=False, extents={c: (1, w.lengths[tid[c]] + SLACK) for c in order if c in tid})
    exact = shard.pack(items, concat_reads=False, extents={c: (1, max(1, w.sets[tid[c]].max_end)) for c in order if c in tid})
    return first, exact


# the shards of one context that holds every chromosome: [first plan, exact plan]
SHAPES = {
    "three_shards": [[["c1", "c2"], ["c3", "c4"], ["c5", "c6", "empty", "ghost"]]] * 2,
    "overhang_last": [[["c1", "c2"], ["c3", "c4"], ["c5", "c6", "empty", "ghost"]]] * 2,
    "overhang_first": [[["c1", "c2", "c3"], ["c4", "empty", "ghost"]], [["c1", "c2", "c3", "c4", "empty", "ghost"]]],
    "overhang_middle": [[["c1", "c2", "c3", "empty", "ghost"]]] * 2,
    "cut": [[["c1", "c2", "c3", "c4", "c5", "c6", "empty", "ghost"]]] * 2,
    "cut_overhang": [[["c1", "c2"], ["c3", "c4"], ["c5", "c6", "empty", "ghost"]]] * 2,
    "cut_overhang_late": [[["c1", "c2"], ["c3", "c4"], ["c5", "c6", "empty", "ghost"]]] * 2,
    "cut_three_shards": [[["c1", "c2"], ["c3", "c4"], ["c5", "c6", "empty", "ghost"]]] * 2,
    "declined": [[["c1", "c2", "c3", "c4", "c5", "c6", "empty", "ghost"]]] * 2,
    "unsorted_three_shards": [[["c1", "c2"], ["c3", "c4"], ["c5", "c6", "empty", "ghost"]]] * 2,
}
