"""Inputs of the read-filter tests (--minMapQ / --requireFlags / --excludeFlags; ``spl_bam_set_filter``): a golden read set X with
a MAPQ drawn per read -- {255, 3, 1, 0} weighted like STAR's, and a few values around the threshold -- and the bits 0x100, 0x400,
0x800, 0x200 set in some flags; X' = X without the reads the filter drops, taken out in numpy (``keep_mask`` is the rule's
restatement: flags first, MAPQ as a number).  Whoever is tested gets X and the filter; the oracle only ever sees X'.

A case is only a case if it drops a read by flags and one by MAPQ, keeps a spliced read, and if the oracle's beta1 differs
between X and X' at some site: ``Case`` asserts all four, so that nothing passes vacuously."""
import os

import numpy as np

import helpers
from spliser_amd import samio

GOLDEN = helpers.GOLDEN
FILTER_A = (255, 0, 0x900)        # what STAR pipelines run samtools for: unique, primary, not supplementary
FILTER_B = (3, 0x1, 0x400)        # paired reads, no duplicates, MAPQ 3 and more
EXTRA_BITS = (0x100, 0x400, 0x800, 0x200)


def keep_mask(flag, mapq, filt):
    """-> (kept, dropped by flags, dropped by MAPQ alone) as boolean arrays: samtools view -q / -f / -F."""
    q, req, exc = filt
    flag = np.asarray(flag).astype(np.int64)
    by_flags = ((flag & exc) != 0) | ((flag & req) != req)
    by_mapq = ~by_flags & (np.asarray(mapq).astype(np.int64) < q)
    return ~by_flags & ~by_mapq, by_flags, by_mapq


def subset(rs, mask):
    """The reads of ``rs`` where ``mask`` holds, as a ReadSet of their own."""
    return gather(rs, np.flatnonzero(mask))


def gather(rs, idx):
    """Reads ``idx`` of ``rs``, in that order."""
    off = rs.cig_off.astype(np.int64)
    lens = (off[1:] - off[:-1])[idx]
    new_off = np.concatenate(([0], np.cumsum(lens)))
    ops = np.concatenate([rs.cigar[off[i]:off[i + 1]] for i in idx]) if len(idx) else np.zeros(0, np.uint32)
    return samio.ReadSet(rs.pos[idx], rs.flag[idx], new_off, ops)


def golden_sets(case):
    """-> (reference names, [(chrom, ReadSet)] in the header's order) of a golden case's reads.sam."""
    names, sets = samio.read_sam(os.path.join(GOLDEN, case, "reads.sam"))
    return names, [(c, sets[c]) for c in names if c in sets]


class Case(object):
    """X, its MAPQs and X' for one golden read set, one seed and one filter."""

    def __init__(self, case, seed, filt, repeat=1, all_fail=None):
        """``repeat``: every read that many times over (files of many BGZF blocks).  ``all_fail``: a chromosome whose
        every read gets MAPQ 0 and the flag 0x800 -- whole blocks of dropped records."""
        self.name, self.filt = case, tuple(filt)
        self.dir = os.path.join(GOLDEN, case)
        self.names, base = golden_sets(case)
        self.lengths = [10 ** 8] * len(self.names)
        rng = np.random.default_rng(seed)
        q = self.filt[0]
        values = np.array([255, 3, 1, 0] + sorted({max(q - 1, 0), q, min(q + 1, 255)}))
        weights = np.array([0.84, 0.06, 0.03, 0.01] + [0.06 / (len(values) - 4)] * (len(values) - 4))
        self.x, self.mapq, self.x_kept, self.mapq_kept = [], [], [], []
        self.by_flags = self.by_mapq = 0
        self.spliced_kept = 0
        for chrom, rs in base:
            if repeat > 1:      # (every read that many times, the file still sorted by position)
                rs = gather(rs, np.repeat(np.arange(rs.n), repeat))
            flag = rs.flag.astype(np.int64)
            for bit in EXTRA_BITS:
                flag |= np.where(rng.random(rs.n) < 0.07, bit, 0)
            mapq = rng.choice(values, size=rs.n, p=weights / weights.sum())
            if chrom == all_fail:
                mapq[:] = 0
                flag |= 0x800
            full = samio.ReadSet(rs.pos, flag, rs.cig_off, rs.cigar)
            kept, by_flags, by_mapq = keep_mask(flag, mapq, self.filt)
            sub = subset(full, kept)
            self.x.append((chrom, full))
            self.mapq.append(mapq)
            self.x_kept.append((chrom, sub))
            self.mapq_kept.append(mapq[kept])
            self.by_flags += int(by_flags.sum())
            self.by_mapq += int(by_mapq.sum())
            self.spliced_kept += int(((sub.cigar & 15) == 3).sum() > 0) if sub.n else 0
        self.n_all = sum(rs.n for _, rs in self.x)
        self.n_kept = sum(rs.n for _, rs in self.x_kept)
        assert self.by_flags >= 1, "the case drops no read by its flags"
        assert self.by_mapq >= 1, "the case drops no read by its MAPQ"
        assert self.spliced_kept >= 1, "the case keeps no spliced read"
        assert self.n_kept + self.by_flags + self.by_mapq == self.n_all

    def write(self, prefix, **kw):
        """-> (path of X as BAM, path of X' as BAM), by the same writer."""
        full, kept = prefix + ".x.bam", prefix + ".kept.bam"
        samio.write_bam(full, self.names, self.lengths, self.x, mapq=self.mapq, **kw)
        samio.write_bam(kept, self.names, self.lengths, self.x_kept, mapq=self.mapq_kept, **kw)
        return full, kept

    def assert_beta1_differs(self, oracle, stranded=None):
        """The oracle's beta1 over the case's junction file differs between X and X' at some site: the filter matters."""
        table = helpers.build_table(self.dir, {"stranded": stranded})
        for (chrom, full), (_, sub) in zip(self.x, self.x_kept):
            if chrom not in table.chrom_index:
                continue
            arr = table.chrom_arrays(chrom)
            if arr.n == 0:
                continue
            a, b = (oracle.check_bam(arr.pos, arr.strand, arr.part_off, arr.part_pos, arr.comp_off, arr.comp_pos, rs.pos, rs.flag,
                                     rs.cig_off, rs.cigar, helpers.STRANDED[stranded], 0)[0] for rs in (full, sub))
            if not np.array_equal(a, b):
                return
        raise AssertionError("the oracle's beta1 is the same for X and X': the filter changes nothing here")


def same_reads(got, want, what=""):
    """A decoder's arrays of one reference against a ReadSet: pos, flag, cig_off, cigar and max_end."""
    if want.n == 0:
        assert got is None or got.n == 0, what
        return
    assert got.n == want.n, (what, got.n, want.n)
    assert np.array_equal(got.pos, want.pos), what
    assert np.array_equal(got.flag, want.flag), what
    assert np.array_equal(np.asarray(got.cig_off, np.int64) - int(got.cig_off[0]), want.cig_off.astype(np.int64)), what
    assert np.array_equal(got.cigar[:len(want.cigar)], want.cigar), what
    assert got.max_end == want.max_end, (what, got.max_end, want.max_end)
