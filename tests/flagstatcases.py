"""Inputs and the restatement for the flagstat tests (``spl_bam_set_flagstat``; csrc/spl_flagstat.h).  No tests in here.

``restate`` is the table of the counters said once more, as sixteen boolean masks over numpy arrays of (flag, tid, next_tid,
mapq) -- column by column from the table, no loop over records and no bit tricks, so that it shares nothing with the C function
but the table.  ``restate_filtered`` takes the records a read filter drops out first (``filtercases.keep_mask``: the filter's own
restatement), every record judged, placed or not.

Files are built from ``scancases.record`` and ``scancases.bam_header`` as BGZF blocks cut where the case says -- ``samio.write_bam``
writes next_refID = -1 for every record and cannot make them.  A ``Built`` keeps the records' fields beside their bytes."""
import numpy as np

import filtercases as F
import scancases as sc
from spliser_amd import samio

N_CAT = 16
NAMES = ("total", "primary", "secondary", "supplementary", "duplicates", "primary duplicates", "mapped", "primary mapped", "paired", "read1", "read2",
         "properly paired", "both mapped", "singletons", "mate elsewhere", "mate elsewhere mapq>=5")


def masks(flag, tid, next_tid, mapq):
    """-> (bool (16, n): record k belongs to category c; bool (n): record k failed quality control, FLAG 0x200)."""
    flag, tid, next_tid, mapq = (np.asarray(a).astype(np.int64) for a in (flag, tid, next_tid, mapq))

    def has(bit):
        return (flag & bit) != 0
    everything = np.ones(flag.shape, bool)
    primary = ~has(0x100) & ~has(0x800)
    paired = primary & has(0x1)
    both = paired & ~has(0x4) & ~has(0x8)
    elsewhere = both & (next_tid != tid)
    rows = [everything, primary, has(0x100), has(0x800) & ~has(0x100), has(0x400), primary & has(0x400), ~has(0x4), primary & ~has(0x4), paired, paired & has(0x40),
            paired & has(0x80), paired & has(0x2) & ~has(0x4), both, paired & has(0x8) & ~has(0x4), elsewhere, elsewhere & (mapq >= 5)]
    assert len(rows) == N_CAT
    return np.array(rows, bool).reshape(N_CAT, -1), has(0x200)


def restate(flag, tid, next_tid, mapq):
    """-> int64 (16, 2): [category, 0] QC-passed records, [category, 1] QC-failed ones (FLAG 0x200)."""
    rows, failed = masks(flag, tid, next_tid, mapq)
    return np.array([[int((r & ~failed).sum()), int((r & failed).sum())] for r in rows], np.int64)


def restate_filtered(flag, tid, next_tid, mapq, filt):
    """The counters of the file with the records taken out that ``filt`` = (min_mapq, require, exclude) drops."""
    keep = F.keep_mask(flag, mapq, filt)[0]
    return restate(*(np.asarray(a)[keep] for a in (flag, tid, next_tid, mapq)))


class Built(object):
    """header + records and their fields; ``write`` cuts the stream into BGZF blocks of the given payload lengths."""

    def __init__(self, n_ref, records, fields, text_len=0):
        self.n_ref = n_ref
        self.header = sc.bam_header(n_ref, text_len)
        self.records = list(records)
        self.flag, self.tid, self.next_tid, self.mapq = (np.array([f[k] for f in fields], np.int64) for k in range(4))
        self.offsets = np.concatenate(([len(self.header)], len(self.header) + np.cumsum([len(r) for r in self.records]))).astype(np.int64)
        self.stream = self.header + b"".join(self.records)
        self.n_records = len(self.records)

    def fields(self):
        return self.flag, self.tid, self.next_tid, self.mapq

    def want(self, filt=(0, 0, 0)):
        return restate_filtered(self.flag, self.tid, self.next_tid, self.mapq, filt)

    def tiles(self, length, first=None):
        return sc.tile(len(self.stream), length, first=first)

    def cut_points(self, lens):
        return np.cumsum(np.asarray(lens, np.int64))[:-1]

    def straddled(self, at):
        """Does a record begin before stream offset ``at`` and end behind it?"""
        k = int(np.searchsorted(self.offsets, at, side="right")) - 1
        return 0 <= k < self.n_records and self.offsets[k] < at < self.offsets[k + 1]

    def block_of_record(self, lens):
        """-> per record the index of the block its first byte lies in."""
        ends = np.cumsum(np.asarray(lens, np.int64))
        return np.searchsorted(ends, self.offsets[:-1], side="right")

    def want_packed(self, lens, filt=(0, 0, 0)):
        """-> uint32 (blocks, 16): what the scan leaves per block -- QC-passed in the low half, QC-failed in the high half."""
        owner = self.block_of_record(lens)
        out = np.zeros((len(lens), N_CAT), np.uint32)
        for b in np.unique(owner):
            m = owner == b
            c = restate_filtered(self.flag[m], self.tid[m], self.next_tid[m], self.mapq[m], filt)
            assert c.max() <= 0xFFFF
            out[b] = (c[:, 0] | (c[:, 1] << 16)).astype(np.uint32)
        return out

    def write(self, path, lens, level=1):
        lens = [int(n) for n in lens]
        assert sum(lens) == len(self.stream) and max(lens) <= 65536
        at = 0
        with open(path, "wb") as fh:
            for n in lens:
                fh.write(samio._bgzf_block(self.stream[at:at + n], level))
                at += n
            fh.write(samio._BGZF_EOF)
        return path


def _rec(tid, pos, flag, mapq, next_tid, body=0, rng=None, cigar=None):
    """A record of about 40 + 1.5 * body bytes: SEQ and QUAL of ``body`` bases, a CIGAR that fits them."""
    if cigar is None:
        cigar = [sc.op(body, sc.M)] if body and tid >= 0 and pos >= 0 else []
    seq = bytes(rng.integers(0, 256, (body + 1) // 2, dtype=np.uint8)) if body else b""
    qual = bytes(rng.integers(0, 64, body, dtype=np.uint8)) if body else b""
    name = b"q%d\x00" % int(rng.integers(0, 10 ** 6)) if rng is not None else b"r\x00"
    return sc.record(tid=tid, pos=pos, name=name, mapq=mapq, flag=flag, cigar=cigar, seq=seq, qual=qual, next_tid=next_tid, next_pos=pos + 150 if next_tid >= 0 else -1)


# flags that reach every category, each once QC-passed and once (| 0x200) QC-failed; (flag, next_tid relative: 0 same, 1 other, -1 none, mapq)
_KINDS = [
    (0x0, -1, 60),                                   # single-end, mapped
    (0x1 | 0x2 | 0x40, 0, 60),                       # read1 of a proper pair
    (0x1 | 0x2 | 0x80 | 0x10, 0, 60),                # read2
    (0x1 | 0x40, 1, 4),                              # mate on another chromosome, MAPQ 4
    (0x1 | 0x80, 1, 5),                              # ... and MAPQ 5
    (0x1 | 0x40, 1, 255),
    (0x1 | 0x8 | 0x40, 0, 30),                       # singleton
    (0x1 | 0x4 | 0x80, 0, 0),                        # unmapped, placed at its mate (0x4 with a reference and a position)
    (0x1 | 0x2 | 0x4 | 0x40, 0, 0),                  # unmapped and "properly paired": not counted as such
    (0x100, -1, 1),                                  # secondary
    (0x100 | 0x800, -1, 1),                          # secondary + supplementary: secondary only
    (0x800 | 0x1 | 0x40, 1, 60),                     # supplementary of a pair: no pair category
    (0x400, -1, 60),                                 # duplicate
    (0x400 | 0x1 | 0x2 | 0x80, 0, 60),
    (0x400 | 0x100, -1, 3),                          # duplicate, not primary
    (0x1 | 0x40, -1, 60),                            # paired and mapped, the flag says the mate is mapped, no mate reference
    (0x1 | 0x2 | 0x40 | 0x80, 0, 60),                # both read1 and read2
]


def mix(seed=1, n=400, n_ref=3, body=0, tail=12, text_len=0):
    """The "all categories" record mix: ``n`` records sorted by reference, drawn from _KINDS with 0x200 on a third, then ``tail``
    records without a reference (tid -1: unmapped pairs and single reads, some with MAPQ that a filter keeps).  ``body`` > 0:
    SEQ / QUAL of about that many bases, so that records are a few hundred bytes and straddle blocks and windows."""
    rng = np.random.default_rng(seed)
    recs, fields = [], []
    kinds = [k for k in range(len(_KINDS))] * 2      # (every kind at least twice: once passing, once failing quality control)
    kinds += [int(x) for x in rng.integers(0, len(_KINDS), max(0, n - len(kinds)))]
    fails = [False] * len(_KINDS) + [True] * len(_KINDS) + [bool(x) for x in rng.random(max(0, n - 2 * len(_KINDS))) < 0.33]
    order = rng.permutation(len(kinds))
    pos = 0
    for j, k in enumerate(order):
        flag, rel, mapq = _KINDS[kinds[k]]
        flag |= 0x200 if fails[k] else 0
        tid = min(j * n_ref // len(order), n_ref - 1)
        next_tid = tid if rel == 0 else (tid + 1) % n_ref if rel == 1 else -1
        pos += int(rng.integers(0, 50))
        b = int(body + rng.integers(-body // 4, body // 4 + 1)) if body else 0
        recs.append(_rec(tid, pos, flag, mapq, next_tid, b, rng))
        fields.append((flag, tid, next_tid, mapq))
    for j in range(tail):
        flag = (0x4 | 0x1 | 0x8 | (0x40 if j % 2 else 0x80), 0x4, 0x4 | 0x200, 0x4 | 0x1 | 0x8 | 0x40 | 0x200)[j % 4]
        mapq = (0, 0, 255, 3)[j % 4]
        recs.append(_rec(-1, -1, flag, mapq, -1, body // 2 if body else 0, rng, cigar=[]))
        fields.append((flag, -1, -1, mapq))
    built = Built(n_ref, recs, fields, text_len)
    w = built.want()
    assert np.all(w > 0), "the mix misses a category: %s" % [NAMES[c] for c in np.flatnonzero((w == 0).any(axis=1))]
    return built


def full_blocks(n_blocks, flag=0x1 | 0x2 | 0x40 | 0x80 | 0x200 | 0x400, mapq=60):
    """``n_blocks`` blocks of 65 536 bytes of nothing but 37-byte records, all QC-failed, each in every category a primary record can
    be in (its mate on the next reference): the first block begins with a record, so that 1 772 begin in it."""
    header = sc.bam_header(2, text_len=50)
    n = (n_blocks * 65536 - len(header)) // 37
    one = {t: sc.record(tid=t, pos=5, name=b"\x00", mapq=mapq, flag=flag, next_tid=1 - t, next_pos=9) for t in (0, 1)}
    tids = [0 if k < n // 2 else 1 for k in range(n)]
    built = Built(2, [one[t] for t in tids], [(flag, t, 1 - t, mapq) for t in tids], text_len=50)
    lens = built.tiles(65536, first=len(header))
    return built, lens


def with_mates(case_name, seed, repeat=4, body=100):
    """A golden read set rebuilt record by record with mates: flags get pair, quality-control, duplicate and secondary bits, MAPQs
    are drawn as ``filtercases`` draws them, next_refID is the read's own reference, another one or none."""
    rng = np.random.default_rng(seed)
    names, sets = F.golden_sets(case_name)
    recs, fields = [], []
    for t, (chrom, rs) in enumerate(sets):
        tid = names.index(chrom)
        idx = np.repeat(np.arange(rs.n), repeat)
        off = rs.cig_off.astype(np.int64)
        for i in idx:
            flag = int(rs.flag[i]) & 0x10
            flag |= int(rng.choice([0, 0x1 | 0x2 | 0x40, 0x1 | 0x2 | 0x80, 0x1 | 0x40, 0x1 | 0x8 | 0x80, 0x1 | 0x4 | 0x40]))
            for bit, p in ((0x100, 0.05), (0x200, 0.1), (0x400, 0.08), (0x800, 0.05)):
                flag |= bit if rng.random() < p else 0
            mapq = int(rng.choice([255, 255, 255, 60, 5, 4, 3, 1, 0]))
            next_tid = int(rng.choice([tid, tid, tid, (tid + 1) % len(names), -1]))
            ops = [int(x) for x in rs.cigar[off[i]:off[i + 1]]]
            recs.append(_rec(tid, int(rs.pos[i]) - 1, flag, mapq, next_tid, body, rng, cigar=ops))
            fields.append((flag, tid, next_tid, mapq))
    for j in range(9):
        flag, mapq = (0x4 | 0x1 | 0x8 | 0x40, 0) if j % 3 else (0x4 | 0x200, 255)
        recs.append(_rec(-1, -1, flag, mapq, -1, body, rng, cigar=[]))
        fields.append((flag, -1, -1, mapq))
    built = Built(len(names), recs, fields)
    # (the header's names are c0, c1, ...: the golden names are not needed, only the order of the references)
    return built
