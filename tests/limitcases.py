"""Read sets and site tables built to land on the counting kernels' limits (the LDS difference windows, the waves' lists, the tiles
of the fused pass, the junction table's rival counts, the scan's blocks), with the helper that counts them the way `process` does
from BAM-native arrays resident on the device.  Shared by test_gpu_kernel_limits.py (GPU parity against the oracle) and
test_limitcases_host.py (CPU checks that every case reaches the limit it names).

The limits are read from the kernel headers, so the cases follow the code when a constant is retuned."""
import os
import re
import tempfile

import numpy as np

from spliser_amd import native, samio, sites, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "spliser_amd", "csrc")

M, I, D, N, S, H, P, EQ, X = 0, 1, 2, 3, 4, 5, 6, 7, 8


def _header_constants():
    """Every object-like `#define SPL_... <integer expression>` of the headers the kernels share (the first definition wins:
    `#ifndef` defaults come first)."""
    pat = re.compile(r"^\s*#\s*define\s+(SPL_[A-Z0-9_]+)\s+([^/\n]+?)\s*(?://.*)?$")
    vals = {}
    for name in ("spl_pack.h", "spl_devpack.h", "spl_device.h"):
        with open(os.path.join(CSRC, name)) as fh:
            for line in fh:
                m = pat.match(line)
                if not m or m.group(1) in vals:
                    continue
                expr = re.sub(r"\b(0x[0-9a-fA-F]+|\d+)[uU]\b", r"\1", m.group(2)).replace("/", "//")
                if not re.fullmatch(r"[\sA-Za-z0-9_()+\-*/<>x]+", expr):
                    continue
                try:
                    v = eval(expr, {"__builtins__": {}}, dict(vals))
                except Exception:
                    continue
                if isinstance(v, int):
                    vals[m.group(1)] = v
    return vals


def _kernel_literal(pattern):
    with open(os.path.join(CSRC, "spl_kernels.hip")) as fh:
        found = re.findall(pattern, fh.read())
    assert len(set(found)) == 1, (pattern, found)
    return int(found[0])


C = _header_constants()
WIN = C["SPL_WIN"]                                    # pair kernel, range kernel unstranded (fused or not)
WIN_STRANDED = C["SPL_WIN_STRANDED"]                  # range kernel, stranded
WIN_STRANDED_FUSED = C["SPL_WIN_STRANDED_FUSED"]      # fused pass, stranded
WAVE_READS = C["SPL_WAVE_READS"]                      # a wave's list entries, range kernel
WAVE_READS_FUSED = C["SPL_WAVE_READS_FUSED"]          # ... fused pass
TILE = C["SPL_TILE_FUSED"]
CHUNK, CHUNK_BIG = C["SPL_CHUNK"], C["SPL_CHUNK_BIG"]
SCAN_BLOCK = C["SPL_SCAN_BLOCK"]
WAVES, WAVES_FUSED = C["SPL_BLOCK"] // 64, C["SPL_BLOCK_FUSED"] // 64
K_RUN = (C["SPL_K_SIMPLE"], C["SPL_K_MNM"], 1, 1)     # reads per lane and wave-iteration, by run
# rival counts above which the range kernel hands a read to the literal kernel (rivals_inline_from / rivals_inline2)
RIV_ONCE = _kernel_literal(r"n_riv > (\d+)u")
RIV_TWICE = _kernel_literal(r"SPL_JF_COUNT_MASK\) > (\d+)u")


# ---- tables and reads -----------------------------------------------------------------------------------------------------------

class Table(object):
    """The arrays of sites.ChromArrays (what native.SiteArrays.from_chrom and the oracle take), alpha and edge counts included."""

    def __init__(self, pos, strand, part_off, part_pos, part_site, comp_off, comp_pos, alpha, edge_cnt):
        self.pos, self.strand = np.asarray(pos, np.int64), np.asarray(strand, np.uint8)
        self.part_off, self.part_pos = np.asarray(part_off, np.uint32), np.asarray(part_pos, np.int64)
        self.part_site = np.asarray(part_site, np.int32)
        self.comp_off, self.comp_pos = np.asarray(comp_off, np.uint32), np.asarray(comp_pos, np.int64)
        self.alpha, self.edge_cnt = np.asarray(alpha, np.int64), np.asarray(edge_cnt, np.int64)
        self.n = int(self.pos.shape[0])

    @classmethod
    def from_chrom(cls, arr):
        return cls(arr.pos, arr.strand, arr.part_off, arr.part_pos, arr.part_site, arr.comp_off, arr.comp_pos, arr.alpha, arr.edge_cnt)

    def sites(self):
        return native.SiteArrays.from_chrom(self)

    def dpos(self):
        return np.unique(self.pos)

    def rows_at(self, x):
        return np.nonzero(self.pos == x)[0]

    def rivals(self, l, r):
        """Rows t for which checkBam's compSplicing holds given the read junction (l, r) (SpliSER_v0_1_8.py:494-501)."""
        out = []
        for t in range(self.n):
            p = set(self.part_pos[self.part_off[t]:self.part_off[t + 1]].tolist())
            c = set(self.comp_pos[self.comp_off[t]:self.comp_off[t + 1]].tolist())
            if (l in p and r in c) or (r in p and l in c):
                out.append(t)
        return out

    def junction_ends(self):
        """Positions that are an end of a junction with rivals (the kernels' flagged positions)."""
        ends = set()
        for t in range(self.n):
            for p in self.part_pos[self.part_off[t]:self.part_off[t + 1]].tolist():
                for c in self.comp_pos[self.comp_off[t]:self.comp_off[t + 1]].tolist():
                    ends.update((p, c))
        return ends


class TableBuilder(object):
    """Rows by (position, strand); partner links by row, competitors by position.  build() sorts the rows by position."""

    def __init__(self, seed=0):
        self.rows = []            # [pos, strand byte, partner rows, loose partner positions, competitor positions]
        self.rng = np.random.default_rng(seed)

    def row(self, pos, strand="+"):
        self.rows.append([int(pos), ord(strand) if strand else 0, [], [], []])
        return len(self.rows) - 1

    def link(self, a, b):
        self.rows[a][2].append(b)
        self.rows[b][2].append(a)

    def partner(self, t, row):
        self.rows[t][2].append(row)

    def compete(self, t, pos):
        self.rows[t][4].append(int(pos))

    def rival(self, t, l_row, r_pos):
        """Make row t a rival of the junction (pos of l_row, r_pos): l_row is a partner of t, r_pos a competitor."""
        self.partner(t, l_row)
        self.compete(t, r_pos)

    def build(self):
        order = sorted(range(len(self.rows)), key=lambda i: (self.rows[i][0], self.rows[i][1]))
        new = {old: k for k, old in enumerate(order)}
        pos, strand, part_off, part_pos, part_site, comp_off, comp_pos, edge = [], [], [0], [], [], [0], [], []
        for old in order:
            p, s, prow, ppos, cpos = self.rows[old]
            pos.append(p)
            strand.append(s)
            for r in prow:
                part_pos.append(self.rows[r][0])
                part_site.append(new[r])
            for x in ppos:
                part_pos.append(x)
                part_site.append(-1)
            part_off.append(len(part_pos))
            comp_pos.extend(cpos)
            comp_off.append(len(comp_pos))
        n = len(pos)
        alpha = self.rng.integers(0, 12, n) * (self.rng.random(n) < 0.7)     # alpha 0 on about a third of the rows
        edge = self.rng.integers(0, 6, len(part_pos))
        return Table(pos, strand, part_off, part_pos, part_site, comp_off, comp_pos, alpha, edge)


def reads_from(recs):
    """[(flag, pos, [(length, op code), ...])] -> samio.ReadSet, in the order given."""
    pos = np.array([r[1] for r in recs], np.int64)
    flag = np.array([r[0] for r in recs], np.uint16)
    off = np.concatenate(([0], np.cumsum([len(r[2]) for r in recs]))).astype(np.uint32)
    cig = np.array([(ln << 4) | code for r in recs for ln, code in r[2]], np.uint32)
    return samio.ReadSet(pos, flag, off, cig)


def records(rs):
    """samio.ReadSet -> [(flag, pos, [(length, op code), ...])]."""
    off = rs.cig_off.astype(np.int64)
    return [(int(rs.flag[i]), int(rs.pos[i]), [(int(o) >> 4, int(o) & 15) for o in rs.cigar[off[i]:off[i + 1]]]) for i in range(rs.n)]


def concat(segments):
    """[(ReadSet, shift)] -> one ReadSet in shard coordinates (what the oracle counts)."""
    recs = []
    for rs, shift in segments:
        recs += [(f, p + shift, ops) for f, p, ops in records(rs)]
    return reads_from(recs)


def read_class(ops, flag=0):
    """The packer's run of a read (spl_pack.h) inside the coordinate space whose CIGAR holds M, N, = and X ops only: 0 simple,
    1 once-spliced (first block below 2^16; the intron and the second block are full words), 2 twice-spliced (all three blocks
    below 2^16), 3 everything else (flag 0x4, longer blocks, more junctions).  Any other op makes it 3 here, which is the
    packer's answer for indels and for CIGARs of more than SPL_PACK_SCAN_OPS ops and what the cases here need of clips."""
    if flag & 4 or any(c not in (M, N, EQ, X) for _, c in ops):
        return 3
    shape = "".join("N" if c == N else "A" for _, c in ops)
    blocks = [ln for ln, c in ops if c != N]
    if shape == "A":
        return 0 if blocks[0] < 1 << 16 else 3
    if shape == "ANA":
        return 1 if blocks[0] < 1 << 16 else 3
    if shape == "ANANA":
        return 2 if max(blocks) < 1 << 16 else 3
    return 3


def _repeat(rs, times):
    """Every read `times` times in a row."""
    keep = np.repeat(np.arange(rs.n), times)
    off = rs.cig_off.astype(np.int64)
    op_idx = np.concatenate([np.arange(off[i], off[i + 1]) for i in keep]) if len(keep) else np.zeros(0, np.int64)
    n_ops = np.diff(off)[keep]
    return samio.ReadSet(rs.pos[keep], rs.flag[keep], np.concatenate(([0], np.cumsum(n_ops))).astype(np.uint32),
                         rs.cigar[op_idx.astype(np.int64)])


class Case(object):
    """A site table, the read segments [(ReadSet, shift)] laid end to end in one set of arrays, the limit they are built to reach,
    and what the CPU self-checks need to show that they reach it."""

    def __init__(self, name, table, segments, limit, **meta):
        self.name, self.table, self.segments, self.limit = name, table, segments, limit
        self.reads = concat(segments) if len(segments) > 1 or segments[0][1] else segments[0][0]
        self.meta = meta
        self.modes = meta.get("modes", [(st, cb) for st in (0, 1, 2) for cb in (0, 1)])


# ---- the hand-built cases of test_gpu_parity.py ---------------------------------------------------------------------------------

def _synth_table(wl, stranded):
    with tempfile.TemporaryDirectory() as tmp:
        bed = os.path.join(tmp, "j.bed")
        synth.write_bed(bed, wl.genome.chrom_names, wl.junctions)
        table = sites.SiteTable(is_stranded=stranded)
        table.add_bed(bed)
        table.find_competitors()
    return table


def non_consuming_ops_case():
    """Soft clips, hard clips, insertions and padding around spliced and unspliced reads, on a table with rivals."""
    rng = np.random.default_rng(17)
    wl = synth.Workload("arabidopsis", scale=0.004, seed=31)
    table = _synth_table(wl, True)
    arr, reads = table.chrom_arrays(wl.genome.chrom_names[0]), wl.reads[0]
    cig_off = reads.cig_off.astype(np.int64)
    new_ops, new_off = [], [0]
    for i in range(reads.n):
        ops = reads.cigar[cig_off[i]:cig_off[i + 1]].tolist()
        style = int(rng.integers(0, 8))
        out = []
        if style in (1, 3, 5):
            out.append((int(rng.integers(1, 9)) << 4) | 5)          # leading hard clip
        if style in (1, 2, 3):
            out.append((int(rng.integers(1, 30)) << 4) | 4)         # leading soft clip
        for k, op in enumerate(ops):
            if style in (4, 5) and k == 0 and (op & 15) == 0 and (op >> 4) > 20:   # an insertion splits the first block
                a = int(rng.integers(5, (op >> 4) - 5))
                out += [(a << 4) | 0, (int(rng.integers(1, 4)) << 4) | 1, (((op >> 4) - a) << 4) | 0]
            elif style == 6 and k == 0:
                out += [op, (3 << 4) | 6]                            # padding after the first op
            else:
                out.append(op)
        if style in (2, 3, 7):
            out.append((int(rng.integers(1, 30)) << 4) | 4)         # trailing soft clip
        new_ops += out
        new_off.append(len(new_ops))
    deco = samio.ReadSet(reads.pos, reads.flag, np.array(new_off, np.uint32), np.array(new_ops, np.uint32))
    return arr, deco


def twice_spliced_limits_case():
    """The twice-spliced class packs five lengths into four words (aligned < 65536, introns whatever a BAM record holds, < 2^28):
    blocks of 4095 and 4096 bases (the limit of an earlier, 12-bit layout; classcases.py has the 16-bit one), the longest intron,
    =/X blocks, soft clips, a deletion instead of an intron, in every neighbourhood.  -> (SiteArrays, ReadArrays)."""
    rng = np.random.default_rng(23)
    # sites: junction ends of the reads below plus alternatives sharing ends (rivals), both strands
    base = [1000, 1100, 1400, 1500, 5000, 5100, 5400, 5600, 9000, 9050, 300000000, 300000100]
    SHIFT = 10000   # (room in front of the first site for the 4095-base blocks)
    pos = np.array(sorted(set(base + [1050, 1450, 5050, 5500, 9020, 1000 + 4095, 1000 + 4096 + 50])), np.int64) + SHIFT
    n = len(pos)
    strand = np.where(np.arange(n) % 3 == 0, ord("-"), ord("+")).astype(np.uint8)
    # partners: a ring of mutual links over neighbours two apart gives everybody competitors
    part = [[] for _ in range(n)]
    for i in range(n):
        for j in (i + 1, i + 2):
            if j < n:
                part[i].append(j)
                part[j].append(i)
    part_off = np.zeros(n + 1, np.uint32)
    np.cumsum([len(x) for x in part], out=part_off[1:])
    part_site = np.array([j for x in part for j in x], np.int32)
    part_pos = pos[part_site]
    comp = [sorted({int(pos[c]) for p_ in x for c in part[p_] if c != i}) for i, x in enumerate(part)]
    comp_off = np.zeros(n + 1, np.uint32)
    np.cumsum([len(x) for x in comp], out=comp_off[1:])
    comp_pos = np.array([c for x in comp for c in x], np.int64)
    sites_c = native.SiteArrays(pos, strand, part_off, part_pos, comp_off, comp_pos, part_site=part_site)

    def rec(flag, p, *ops):
        return (flag, p, ops)
    shapes = [
        rec(0, 951, (50, M), (100, N), (300, M), (100, N), (60, M)),                   # 1000|1100 .. 1400|1500 ends on sites
        rec(16, 951, (50, EQ), (100, N), (300, X), (100, N), (60, EQ)),
        rec(99, 951, (3, S), (50, M), (100, N), (300, M), (100, N), (60, M), (7, S)),   # soft clips: same class after compaction
        rec(0, 951, (50, M), (100, N), (300, M), (100, D), (60, M)),                    # a deletion where the second intron was
        rec(0, 951, (50, M), (100, N), (150, M), (2, I), (150, M), (100, N), (60, M)),  # insertion splits the middle block: wide
        rec(0, 1000 - 4094, (4095, M), (100, N), (300, M), (100, N), (60, M)),          # a block of 12 bits
        rec(0, 1000 - 4095, (4096, M), (100, N), (300, M), (100, N), (60, M)),          # one more: the same class
        rec(0, 4951, (50, M), (100, N), (300, M), (200, N), (4095, M)),
        rec(0, 8951, (50, M), (50, N), (30, M), ((1 << 28) - 1, N), (40, M)),         # the longest intron a BAM record can hold
        rec(147, 8951, (50, M), (50, N), (0, M), (5, N), (40, M)),                    # an empty middle block
        rec(0, 951, (50, M), (100, N), (300, M)), rec(0, 951, (150, M)), rec(4, 1000, (50, M), (100, N), (300, M), (100, N), (60, M)),
    ]
    recs = []
    for k in range(3000):                        # every shape in every neighbourhood
        recs.append(shapes[int(rng.integers(0, len(shapes)))])
    recs += [shapes[0]] * 300 + [shapes[7]] * 200  # and whole waves of the class
    recs.sort(key=lambda r: r[1])
    rpos = np.array([r[1] for r in recs], np.int64) + SHIFT
    rflag = np.array([r[0] for r in recs], np.uint16)
    off = np.concatenate(([0], np.cumsum([len(r[2]) for r in recs])))
    cig = np.array([(ln << 4) | code for r in recs for ln, code in r[2]], np.uint32)
    return sites_c, native.ReadArrays(rpos, rflag, off, cig)


def long_introns_hot_sites_case():
    """Reads whose introns span thousands of sites, one site hit by 200k reads, sites outside the LDS window, unsorted reads.
    -> (SiteArrays with part_site, ReadArrays, row of the hot site)."""
    rng = np.random.default_rng(5)
    n_sites = 30000
    pos = np.sort(rng.choice(np.arange(1000, 3_000_000), n_sites, replace=False)).astype(np.int64)
    strand = np.where(rng.random(n_sites) < 0.5, ord("+"), ord("-")).astype(np.uint8)
    # partners: pair consecutive sites; competitors: a few
    part_off = np.arange(n_sites + 1, dtype=np.uint32)
    partner = np.arange(n_sites) ^ 1
    part_pos = pos[partner]
    comp_off = np.zeros(n_sites + 1, np.uint32)
    has_comp = rng.random(n_sites) < 0.2
    comp_off[1:] = np.cumsum(has_comp)
    comp_pos = pos[(np.arange(n_sites)[has_comp] + 2) % n_sites]
    recs = []
    for _ in range(300):   # long introns: 10 kb .. 2.5 Mb
        p = int(rng.integers(1000, 400000))
        recs.append((int(rng.choice([0, 16, 99, 147])), p, "20M%dN30M" % int(rng.integers(10000, 2_500_000))))
    hot = int(pos[1234])
    recs += [(0, hot - 40, "100M")] * 3000
    hot_reads = samio.ReadSet.from_records(recs)
    # bulk: 200k unspliced reads on the hot site + random 150M reads; then shuffle a slice to break sortedness
    bulk_pos = np.concatenate((np.full(200000, hot - 70), rng.integers(1000, 2_999_000, 300000))).astype(np.int64)
    bulk = samio.ReadSet(bulk_pos, rng.choice([0, 16], bulk_pos.shape[0]), np.arange(bulk_pos.shape[0] + 1),
                         np.full(bulk_pos.shape[0], 150 << 4, np.uint32))
    allpos = np.concatenate((hot_reads.pos, bulk.pos)).astype(np.int64)
    allflag = np.concatenate((hot_reads.flag, bulk.flag))
    nops = np.concatenate((np.diff(hot_reads.cig_off.astype(np.int64)), np.ones(bulk.n, np.int64)))
    ops = np.concatenate((hot_reads.cigar, bulk.cigar))
    order = np.argsort(allpos, kind="stable")
    order[1000:5000] = order[1000:5000][::-1]
    src = np.concatenate(([0], np.cumsum(nops)))
    cig = np.concatenate([ops[src[i]:src[i + 1]] for i in order])
    off = np.concatenate(([0], np.cumsum(nops[order])))
    sites_c = native.SiteArrays(pos, strand, part_off, part_pos, comp_off, comp_pos, part_site=partner)
    return sites_c, native.ReadArrays(allpos[order], allflag[order], off, cig), 1234


def more_ops_than_the_packed_count_case():
    """A read of 70 000 CIGAR ops (the packed op count saturates at 65 535) between ordinary reads.  -> (SiteArrays, ReadArrays)."""
    # the long read ends at 105 099: a walk that borrowed the ops of the next reads would run on over the site at 105 150
    pos = np.array([150, 400, 100300, 100900, 105150, 200500], np.int64)
    strand = np.full(6, ord("+"), np.uint8)
    part_off = np.array([0, 1, 2, 3, 4, 4, 4], np.uint32)
    part_pos = np.array([400, 150, 100900, 100300], np.int64)
    part_site = np.array([1, 0, 3, 2], np.int32)
    comp_off = np.zeros(7, np.uint32)
    comp_pos = np.zeros(0, np.int64)
    sites_c = native.SiteArrays(pos, strand, part_off, part_pos, comp_off, comp_pos, part_site=part_site)
    n_pairs = 35000
    long_ops = np.empty(2 * n_pairs, np.uint32)       # 1M 2D 1M 2D ...: 70 000 ops, 105 000 reference bases
    long_ops[0::2] = (1 << 4) | 0
    long_ops[1::2] = (2 << 4) | 2
    recs_ops = [long_ops, np.array([(100 << 4) | 0], np.uint32), np.array([(50 << 4) | 0, (249 << 4) | 3, (60 << 4) | 0], np.uint32),
                np.array([(120 << 4) | 0], np.uint32)]
    rpos = np.array([100, 120, 101, 100250], np.int64)
    order = np.argsort(rpos, kind="stable")
    off = np.concatenate(([0], np.cumsum([len(recs_ops[i]) for i in order])))
    return sites_c, native.ReadArrays(rpos[order], np.zeros(4, np.uint16), off, np.concatenate([recs_ops[i] for i in order]))


def _table_of(s):
    """native.SiteArrays -> Table (alpha and edge counts made up where the arrays have none)."""
    rng = np.random.default_rng(s.n)
    part_site = s.part_site if s.part_site is not None else np.full(s.n_part, -1, np.int32)
    alpha = s.alpha if s.alpha is not None else rng.integers(0, 9, s.n)
    edge = s.edge_cnt if s.edge_cnt is not None else rng.integers(0, 5, s.n_part)
    return Table(s.pos, s.strand, s.part_off, s.part_pos, part_site, s.comp_off, s.comp_pos, alpha, edge)


def _readset(r):
    return samio.ReadSet(r.pos, r.flag, r.cig_off, r.cigar)


def parity_cases():
    """test_gpu_parity.py's hand-built cases as Cases for the device path."""
    out = []
    arr, deco = non_consuming_ops_case()
    out.append(Case("non_consuming_ops", Table.from_chrom(arr), [(deco, 0)], "S/H/I/P around spliced reads"))
    s, r = twice_spliced_limits_case()
    out.append(Case("twice_spliced_class_limits", _table_of(s), [(_readset(r), 0)], "blocks of 4095 and 4096 bases (well inside 16 bits), 28-bit introns"))
    s, r, hot = long_introns_hot_sites_case()
    out.append(Case("long_introns_and_hot_sites", _table_of(s), [(_readset(r), 0)], "200k reads on one site, unsorted",
                    modes=[(0, 0), (1, 0), (2, 1)], hot_row=hot))
    s, r = more_ops_than_the_packed_count_case()
    out.append(Case("more_ops_than_the_packed_count", _table_of(s), [(_readset(r), 0)], "70 000 ops in one read"))
    tb = TableBuilder(3)
    tb.row(120, "+")
    star = reads_from([(0, 120, []), (4, 120, [(60, M)]), (0, 100, [(50, M)]), (4, 90, [(40, M)]), (0, 130, [(10, S), (20, M)])])
    out.append(Case("star_and_unmapped_with_cigar", tb.build(), [(star, 0)], "'*' CIGAR, flag 0x4 with a CIGAR"))
    return out


# ---- window edges -------------------------------------------------------------------------------------------------------------

def window_case(win, lead=50):
    """Dense sites, one chunk whose first read lies on site `lead`: the window's base is `lead` (range kernels: the first distinct
    position at or after the first POS - 1; pair kernel: the first row at or after the first POS), so its last entry is row
    E = lead + win.  Ranges of every difference array (beta1 / ME x read strand) end at E - 1, E and E + 1 -- both ends inside,
    one inside and one outside, both outside -- and rivals of two junctions sit at E - 1, E, E + 1, so that their point
    corrections (a key at t and at t + 1) fall on the same edge: flanking ones inside an intron, beta1-type ones under a block.
    One row per position, so that rows and distinct positions have the same indexes."""
    tb = TableBuilder(win)
    E = lead + win
    n = E + 64
    P0 = 10000
    rows = [tb.row(P0 + 3 * k, "+-"[k % 2]) for k in range(n)]
    for k in range(0, n - 1, 2):
        tb.link(rows[k], rows[k + 1])
    pos = lambda k: P0 + 3 * k
    # junction A: (E - 6, E + 4), rivals E - 1, E, E + 1 inside its intron; junction B: (E - 40, E - 30), the same rows as rivals
    # that its reads' second block covers
    la, ra, lb, rb = E - 6, E + 4, E - 40, E - 30
    for t in (E - 1, E, E + 1):
        tb.rival(rows[t], rows[la], pos(ra))
        tb.rival(rows[t], rows[lb], pos(rb))
    table = tb.build()
    flags = (0, 16, 83, 163)
    fp = pos(lead)
    recs = [(0, fp, [(pos(E - 1) + 1 - fp, M)])]             # the chunk's first read: the window's base
    body = []
    for f in flags:
        for d in (-1, 0, 1):
            body.append((f, fp, [(pos(E + d) + 1 - fp, M)]))                          # beta1 range [lead + 1, E + d)
            body.append((f, pos(lead + 7), [(pos(E + d) + 1 - pos(lead + 7), M)]))
            body.append((f, pos(E + d), [(pos(E + 3) + 1 - pos(E + d), M)]))          # starts at E + d, ends outside
            body.append((f, pos(E + 2 + d), [(pos(E + 6) + 1 - pos(E + 2 + d), M)]))  # both ends outside
            # once-spliced: the intron's ME range ends at E + d (c1 - 1 = pos(E + d)), or begins there
            c0 = pos(lead + 12) + 1
            body.append((f, c0 - 20, [(20, M), (pos(E + d) + 1 - c0, N), (25, M)]))
            body.append((f, pos(E + d) - 10, [(11, M), (pos(E + 5) - pos(E + d), N), (12, M)]))
            # twice-spliced: the second intron ends at E + d
            body.append((f, c0 - 20, [(20, M), (30, N), (15, M), (pos(E + d) + 1 - (c0 + 45), N), (9, M)]))
            # junction B, the second block ending just before, at and after a rival (t + 1 covered or not)
            for end in (pos(E + d) - 1, pos(E + d), pos(E + d) + 1, pos(E + d) + 2):
                b1 = pos(lb) + 1 - 25
                body.append((f, b1, [(25, M), (pos(rb) - pos(lb), N), (end - pos(rb), M)]))
        # junction A: rivals flanking; the second block runs on past the window
        body.append((f, pos(la) + 1 - 18, [(18, M), (pos(ra) - pos(la), N), (pos(E + 8) - pos(ra), M)]))
        body.append((f, pos(la) + 1 - 4, [(4, M), (pos(ra) - pos(la), N), (5, M)]))
    recs += body * 3
    recs.insert(len(recs) // 2, (16, pos(lead - 20), [(pos(E) + 1 - pos(lead - 20), M)]))     # POS before the chunk's first one
    recs.insert(len(recs) // 3, (0, pos(n - 1) + 40, [(30, M), (200, N), (30, M)]))            # past the last site
    recs.append((0, pos(n - 1) - 2, [(50, M)]))
    return Case("window_%d" % win, table, [(reads_from(recs), 0)], "LDS window of %d distinct positions" % win,
                win=win, wbase=lead, edge=E)


def window_base(table, first_pos):
    """The range kernels' window base for a chunk whose first read has POS first_pos: dpos of the first site at or after
    first_pos - 1 (dbk_resolve at first_pos - 1)."""
    return int(np.searchsorted(table.dpos(), first_pos - 1, side="left"))


def pair_window_base(table, first_pos):
    """The pair kernel's: the first ROW at or after first_pos (first_site_at_or_after)."""
    return int(np.searchsorted(table.pos, first_pos, side="left"))


def read_ranges(table, rec):
    """[(array kind 'b1' / 'me', lo, ub)] of the dpos ranges a read of plain M/N ops adds to (what the range kernel commits)."""
    dpos = table.dpos()
    flag, p, ops = rec
    out = []
    cur = p
    lo = int(np.searchsorted(dpos, p - 1, side="right"))
    for ln, code in ops:
        if code not in (M, N, EQ, X):
            return None
        cur += ln
        ub = int(np.searchsorted(dpos, cur - 1, side="left"))
        at = int(ub < len(dpos) and dpos[ub] == cur - 1)
        if ub > lo:
            out.append(("me" if code == N else "b1", lo, ub))
        lo = ub + at
    return out


# ---- rival-table thresholds -----------------------------------------------------------------------------------------------------

def _spliced_reads(l, r, starts, ends, flags=(0, 16, 99, 147)):
    """Once-spliced reads with junction (l, r): the first block from each of `starts`, the second to each of `ends` (last base)."""
    out = []
    for f in flags:
        for a in starts:
            for e in ends:
                out.append((f, a, [(l + 1 - a, M), (r - l, N), (e - r, M)]))
    return out


def rival_case(which):
    """Junctions with exactly as many rivals as a threshold allows and one more, and the table flags:
      once_<RIV_ONCE> / once_<RIV_ONCE + 1>: a once-spliced junction (rivals_inline_from: n_riv > RIV_ONCE -> literal);
      twice_<RIV_TWICE> / twice_<RIV_TWICE + 1>: the second junction of twice-spliced reads (rivals_inline2);
      multirow: a rival whose position holds a + and a - row (SPL_JF_MULTIROW: unstranded runs take the literal kernel);
      complex: rivals at the junction's own end, and two rows of one strand at one position (SPL_JF_COMPLEX);
      rival_is_end: a rival of the first junction of twice-spliced reads is an end of their second junction.
    Rivals lie inside the intron (flanking), under the blocks (beta1-type) and on the first and last base of the reads, whose
    blocks start and end one base before, on and after them."""
    tb = TableBuilder(sum(map(ord, which)))
    L, R = 20000, 20600
    kind, _, num = which.partition("_")
    lrow = rrow = None
    if kind != "rival":                                    # (rival_is_end: nothing at L but the other junction's rival)
        lrow, rrow = tb.row(L, "+"), tb.row(R, "+")
        tb.link(lrow, rrow)
    if kind in ("once", "twice"):
        n_riv = int(num)
        inside = [L + 40 + 37 * k for k in range((n_riv + 1) // 2)]
        outside = [R + 30 + 23 * k for k in range(n_riv // 2)]
        riv_pos = inside + outside
    elif kind == "multirow":
        riv_pos = [L + 100, R + 40]
    elif kind == "complex":
        riv_pos = [L + 150, R + 20]
    else:
        riv_pos = [R + 60]
    riv = []
    for k, t in enumerate(riv_pos):
        riv.append(tb.row(t, "+-"[k % 2]))
        if lrow is None:
            tb.rows[riv[-1]][3].append(L)                  # (a partner position that is no row)
            tb.compete(riv[-1], R)
        else:
            tb.rival(riv[-1], lrow, R)
    if kind == "multirow":
        for k, t in enumerate(riv_pos):                    # the other strand at the same positions: not rivals themselves
            tb.link(tb.row(t, "-+"[k % 2]), lrow)
    if kind == "complex":
        c = tb.row(R + 20, "-")                            # a second '-' row at a rival's position, also a rival
        tb.rival(c, lrow, R)
        end = tb.row(L, "-")                               # a rival at the junction's own end: (L, R) with t at L
        tb.rival(end, rrow, L)
    recs = []
    last = max(riv_pos + [R + 80])
    if kind in ("once", "multirow", "complex"):
        firsts = [L - 30, L - 2]
        ends = sorted({R + 5, last + 10} | {t + d for t in riv_pos if t > R for d in (-1, 0, 1, 2)})
        recs += _spliced_reads(L, R, firsts, ends)
        # the first block's first base on a rival before the junction
        recs += _spliced_reads(L, R, [L - 8], [R + 12])
    else:
        # twice-spliced: junction 1 (J1l, J1r) in front, then the junction with the rivals
        J1l, J1r = L - 300, L - 200
        j1row, j1rrow = tb.row(J1l, "+"), tb.row(J1r, "-")
        tb.link(j1row, j1rrow)
        if kind == "rival":                                # (rival_is_end) a rival of junction 1 at L, an end of junction 2
            tb.rival(tb.row(L, "-"), j1row, J1r)
        ends = sorted({R + 5, last + 10} | {t + d for t in riv_pos if t > R for d in (-1, 0, 1, 2)})
        for f in (0, 16, 99, 147):
            for a in (J1l - 20, J1l - 3):
                for e in ends:
                    recs.append((f, a, [(J1l + 1 - a, M), (J1r - J1l, N), (L - J1r, M), (R - L, N), (e - R, M)]))
    # unspliced reads over every row, beginning and ending one base before, on and after it
    for x in sorted({r_[0] for r_ in tb.rows}):
        for f in (0, 16):
            recs += [(f, x + d, [(40, M)]) for d in (-1, 0, 1)] + [(f, x - 40 + d, [(40, M)]) for d in (-1, 0, 1, 2)]
    table = tb.build()
    rs = reads_from(recs * 4)
    return Case("rivals_" + which, table, [(rs, 0)], "junction table: %s" % which, junction=(L, R), n_rivals=len(table.rivals(L, R)))


RIVAL_CASES = ["once_%d" % RIV_ONCE, "once_%d" % (RIV_ONCE + 1), "twice_%d" % RIV_TWICE, "twice_%d" % (RIV_TWICE + 1),
               "multirow", "complex", "rival_is_end"]


# ---- list overflow ------------------------------------------------------------------------------------------------------------

def _overflow_table():
    """Junctions (L_k, R_k) with two rivals each (one flanking, one under the second block): every read below has a flagged end."""
    tb = TableBuilder(77)
    juncs = []
    for k in range(6):
        L = 50000 + 2000 * k
        R = L + 500
        l, r = tb.row(L, "+"), tb.row(R, "+-"[k % 2])
        tb.link(l, r)
        for t in (L + 200, R + 40):
            tb.rival(tb.row(t, "+-"[(t // 10) % 2]), l, R)
        juncs.append((L, R))
    return tb, juncs


def overflow_case(which, n=CHUNK_BIG):
    """Chunks of nothing but reads the waves list (spl_device.h: what makes a list full and push_direct take over):
      twice: flagged twice-spliced reads whose junctions the table decides (back list; nothing queued while the lists have room);
      once: flagged once-spliced reads with RIV_ONCE + 1 rivals (front list, through the range kernel's rival pass);
      front_first: placed flag-0x4 reads (front list) in the first half of the chunk, flagged twice-spliced reads after them;
      back_first: the same the other way round."""
    tb, juncs = _overflow_table()
    if which == "once":
        L, R = juncs[0]
        l = [i for i, r in enumerate(tb.rows) if r[0] == L][0]
        for k in range(RIV_ONCE + 1 - 2):
            tb.rival(tb.row(L + 250 + 11 * k, "+"), l, R)
    table = tb.build()
    rng = np.random.default_rng(len(which))
    recs = []
    for i in range(n):
        k = int(rng.integers(0, len(juncs) - 1))
        L, R = juncs[k]
        f = int(rng.choice([0, 16, 99, 147]))
        if which == "once":
            L, R = juncs[0]
            recs.append((f, L - 40, [(41, M), (R - L, N), (int(rng.integers(10, 80)), M)]))
            continue
        L2, R2 = juncs[k + 1]                               # (the middle block is 1500 bases: far inside the class)
        twice = (f, L - 30, [(31, M), (R - L, N), (L2 - R, M), (R2 - L2, N), (int(rng.integers(5, 60)), M)])
        literal = (f | 4, R - 10, [(int(rng.integers(20, 90)), M)])
        if which == "twice":
            recs.append(twice)
        elif which == "front_first":
            recs.append(literal if i < n // 2 else twice)
        else:
            recs.append(twice if i < n // 2 else literal)
    rs = reads_from(recs)
    return Case("overflow_" + which, table, [(rs, 0)], "wave lists of %d / %d entries" % (WAVE_READS, WAVE_READS_FUSED),
                n_literal=int(np.count_nonzero(rs.flag & 4)))


def listed_reads(case, combine):
    """Per read: 'front' / 'back' / None -- which list of its wave the range kernel puts it on (ignoring room)."""
    table, ends = case.table, case.table.junction_ends()
    out = []
    for f, p, ops in records(case.reads):
        cls = read_class(ops, f)
        if cls == 3:
            out.append("front" if f & 4 else None)
            continue
        juncs, cur = [], p
        for ln, code in ops:
            if code == N:
                juncs.append((cur - 1, cur + ln - 1))
            cur += ln if code in (M, N, D, EQ, X) else 0
        flagged = any(a in ends or b in ends for a, b in juncs)
        if cls == 1 and flagged:
            out.append("front" if combine or len(table.rivals(*juncs[0])) > RIV_ONCE else None)
        elif cls == 2 and flagged:
            out.append("front" if combine else "back")
        else:
            out.append(None)
    return out


def simulate_lists(case, fused, chunk):
    """The waves' lists outside combine mode, as the range kernel fills them: the iterations of a chunk (64 K reads of one run, K by
    run) are dealt round-robin to its waves -- in the fused pass per tile of TILE reads, whose back lists start empty while the front
    lists go on through the chunk.  Within a tile the twice-spliced run pushes to the back list, then the other run to the front
    list, a wave-iteration's entries at a time; a batch that does not fit goes straight to the literal queue (push_direct).
    -> (the most entries a wave would hold if its lists had room for all, the back-list entries that went to the queue)."""
    listed = listed_reads(case, 0)
    classes = [read_class(ops, f) for f, _, ops in records(case.reads)]
    nw, seg = (WAVES_FUSED, WAVE_READS_FUSED) if fused else (WAVES, WAVE_READS)
    demand = extra = 0
    for c0 in range(0, len(listed), chunk):
        c1 = min(c0 + chunk, len(listed))
        want = [0] * nw                                   # (with room for all)
        front = [0] * nw
        for t0 in range(c0, c1, TILE if fused else chunk):
            idx = range(t0, min(t0 + (TILE if fused else chunk), c1))
            back = [0] * nw
            tile_want = [0] * nw
            batches, g0 = [], 0
            for run in range(4):
                mine = [i for i in idx if classes[i] == run]
                per = 64 * K_RUN[run]
                for g in range((len(mine) + per - 1) // per):
                    part = mine[g * per:(g + 1) * per]
                    batches.append(((g0 + g) % nw, sum(listed[i] == "back" for i in part), sum(listed[i] == "front" for i in part)))
                g0 += (len(mine) + per - 1) // per
            for w, nb, nf in batches:
                tile_want[w] += nb + nf
                demand = max(demand, want[w] + tile_want[w])
                if nb:
                    if front[w] + back[w] + nb > seg:
                        extra += nb
                    else:
                        back[w] += nb
                if nf and front[w] + back[w] + nf <= seg:
                    front[w] += nf
            # front entries carry over to the next tile (fused); the back lists are through
            for w, nb, nf in batches:
                want[w] += nf
    return demand, extra


# ---- tiles of the fused pass ----------------------------------------------------------------------------------------------------

def _tile_table():
    tb = TableBuilder(91)
    rows = [tb.row(30000 + 7 * k, "+-"[k % 2]) for k in range(400)]
    for k in range(0, 400, 2):
        tb.link(rows[k], rows[k + 1])
    for k in range(10, 390, 40):                           # a few junctions with rivals
        tb.rival(rows[k + 3], rows[k], 30000 + 7 * (k + 9))
    return tb.build()


def _mixed_read(rng, cls, flagged_ok=True):
    """A read of class cls (0 simple, 1 once-, 2 twice-spliced, 3 other, 4 wide, 5 placed flag 0x4) over _tile_table's sites."""
    f = int(rng.choice([0, 16, 99, 147]))
    p = 30000 + int(rng.integers(-40, 2700))
    if cls == 0:
        return (f, p, [(int(rng.integers(20, 150)), M)])
    if cls == 1:
        return (f, p, [(int(rng.integers(5, 60)), M), (7 * int(rng.integers(1, 12)), N), (int(rng.integers(5, 60)), M)])
    if cls == 2:
        return (f, p, [(int(rng.integers(5, 40)), M), (7 * int(rng.integers(1, 9)), N), (int(rng.integers(3, 30)), M),
                       (7 * int(rng.integers(1, 9)), N), (int(rng.integers(5, 40)), M)])
    if cls == 3:
        return (f, p, [(int(rng.integers(5, 40)), M), (2, D), (int(rng.integers(5, 40)), M)])
    if cls == 4:
        return (f, p, [(3, S), (int(rng.integers(5, 30)), M), (1, I), (int(rng.integers(5, 30)), M), (7 * int(rng.integers(1, 9)), N),
                       (int(rng.integers(5, 30)), M), (2, D), (int(rng.integers(5, 30)), M), (4, S)])
    return (f | 4, p, [(int(rng.integers(20, 90)), M)])


def tile_case(which):
    """class_change_<k>: reads 0 .. k-1 of every chunk simple, then once-spliced, twice-spliced, other and placed 0x4 reads in
    runs, so that a run ends at read k of a tile (k = TILE - 1, TILE, TILE + 1);
    all_wide: tiles of nothing but WIDE reads (the largest records a tile can hold);
    last_tile_<n>: n reads, so that a chunk's last tile holds one read;
    two_segments: two segments with different non-zero shifts in one set of arrays, queued reads (placed 0x4, deletions next to
    flagged junctions) in the second tile of the later segment's cells."""
    table = _tile_table()
    rng = np.random.default_rng(sum(map(ord, which)))
    if which.startswith("class_change_"):
        k = int(which.rsplit("_", 1)[1])
        recs = []
        for c0 in range(0, 2 * CHUNK_BIG, CHUNK):
            cls = [0] * k + [1] * 300 + [2] * 200 + [3] * 100 + [5] * 50
            cls += [int(rng.integers(0, 6)) for _ in range(CHUNK - len(cls))]
            recs += [_mixed_read(rng, c) for c in cls[:CHUNK]]
        return Case("tile_" + which, table, [(reads_from(recs), 0)], "class runs change at read %d" % k, change_at=k)
    if which == "all_wide":
        recs = [_mixed_read(rng, 4) for _ in range(CHUNK_BIG + CHUNK)]
        return Case("tile_all_wide", table, [(reads_from(recs), 0)], "tiles of WIDE reads only")
    if which.startswith("last_tile_"):
        n = int(which.rsplit("_", 1)[1])
        recs = [_mixed_read(rng, int(rng.integers(0, 6))) for _ in range(n)]
        return Case("tile_" + which, table, [(reads_from(recs), 0)], "a last tile of one read", n_reads=n)
    # two segments: their reads in their own coordinates, the shifts move both over the same sites
    s0 = [_mixed_read(rng, int(rng.integers(0, 5))) for _ in range(CHUNK - 300)]
    s1 = [_mixed_read(rng, int(rng.integers(0, 5))) if i < TILE + 200 else _mixed_read(rng, int(rng.choice([3, 5, 2, 1])))
          for i in range(CHUNK_BIG + 700)]
    sh0, sh1 = 1000, 20000
    seg0 = reads_from([(f, p - sh0, ops) for f, p, ops in s0])
    seg1 = reads_from([(f, p - sh1, ops) for f, p, ops in s1])
    return Case("tile_two_segments", table, [(seg0, sh0), (seg1, sh1)], "queue entries through s_idx in shifted segments")


TILE_CASES = (["class_change_%d" % k for k in (TILE - 1, TILE, TILE + 1)] + ["all_wide"]
              + ["last_tile_%d" % n for n in (TILE + 1, CHUNK + 1, CHUNK_BIG + 1)] + ["two_segments"])


# ---- scan / SSE edges -----------------------------------------------------------------------------------------------------------

def scan_case(n_dpos, shared=False):
    """n_dpos distinct positions (the scan kernels take SCAN_BLOCK a workgroup); shared: every fifth position holds a + and a - row,
    every seventh one more row without strand.  Partner pairs with edge counts, rows with alpha 0 and betas 0, a few rivals; alpha,
    edge counts and partner rows all given, so that the counting pass computes SSE in its scan."""
    tb = TableBuilder(n_dpos + shared)
    P0 = 5000
    rows = [tb.row(P0 + 5 * k, "+-"[(k // 2) % 2]) for k in range(n_dpos)]
    if shared:
        for k in range(0, n_dpos, 5):
            tb.link(tb.row(P0 + 5 * k, "-+"[(k // 2) % 2]), rows[k])
        for k in range(0, n_dpos, 7):
            tb.row(P0 + 5 * k, "")
    for k in range(0, n_dpos - 1, 2):
        tb.link(rows[k], rows[k + 1])
    for k in range(2, n_dpos - 3, 9):
        tb.rival(rows[k], rows[k + 1], P0 + 5 * (k + 3))
    table = tb.build()
    rng = np.random.default_rng(n_dpos)
    n_reads = min(4 * n_dpos + 50, 40000)
    span = 5 * n_dpos
    recs = []
    for _ in range(n_reads):
        f = int(rng.choice([0, 16, 99, 147]))
        a = P0 + int(rng.integers(-30, span))
        if rng.random() < 0.5:
            recs.append((f, a, [(int(rng.integers(3, 60)), M)]))
        else:
            recs.append((f, a, [(int(rng.integers(3, 30)), M), (5 * int(rng.integers(1, 6)), N), (int(rng.integers(3, 30)), M)]))
    recs.sort(key=lambda r: r[1])
    # the last rows get no reads at all and alpha 0: a zero denominator
    recs = [r for r in recs if r[1] + sum(ln for ln, _ in r[2]) < P0 + span - 40] or recs[:1]
    table.alpha[-3:] = 0
    return Case("scan_%d%s" % (n_dpos, "_shared" if shared else ""), table, [(reads_from(recs), 0)],
                "%d distinct positions" % n_dpos, n_dpos=n_dpos)


SCAN_SIZES = [1, SCAN_BLOCK - 1, SCAN_BLOCK, SCAN_BLOCK + 1, 2 * SCAN_BLOCK - 1, 2 * SCAN_BLOCK + 1, 65537]


# ---- counting on the device -----------------------------------------------------------------------------------------------------

class DeviceCount(object):
    pass


def count_device(ctx, sites, segments, stranded, combine=0, cryptic=False):
    """What `process` does with BAM-native arrays on the device: upload_soa -> begin_reads / add_soa -> finish -> count_launch ->
    sse_launch; then relayout and count again, which must give the same counters.  -> DeviceCount: counters, sse, lds (bytes of
    the range kernel's launch), fused (no records were written), queued (literal queue of the first pass)."""
    out = DeviceCount()
    with ctx.upload_soa([native.ReadArrays(rs.pos, rs.flag, rs.cig_off, rs.cigar) for rs, _ in segments]) as soa:
        with ctx.upload_sites(sites) as ds:
            dr = ctx.begin_reads(0)
            try:
                for k, (_, shift) in enumerate(segments):
                    dr.add_soa(soa, k, shift)
                dr.finish()
                out.fused = dr.layout_bytes()[1] == 0
                ctx.count_launch(ds, dr, stranded, combine)
                out.lds = ctx.launch_info()["lds_bytes"]
                out.counters = ds.counters()
                out.queued = dr.literal_queue_size()
                ctx.sse_launch(ds, cryptic)
                out.sse = ds.sse_results()
                dr.relayout()
                ctx.count_launch(ds, dr, stranded, combine)
                again = ds.counters()
            finally:
                dr.free()
    for a, b in zip(out.counters, again):
        assert np.array_equal(a, b), "counters differ after relayout"
    return out
