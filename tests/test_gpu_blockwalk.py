"""The per-read kernels on the reads of ``blockwalkcases.py`` -- every CIGAR of one, two and three ops -- and the predicate tally
(``csrc/spl_tally_dev.h``) at its edges, both held EXACTLY to the sums of the host hooks of the same rule headers.

The enumerated reads go up once as one read set, POS cycling through 1 .. 4 under a shift of -2 into a reference of 3 bases, so that
blocks lose bases at both ends, and once more paired i with i + 1 under mate keys.  Both sets go through ``coverage``,
``coverage(fragments=True)``, ``gene_counts`` and ``exon_counts`` with their fragment forms, and ``strand_tally`` with a cover map.
The per-read sums come from the per-read hooks, a read a call; the paired set's from the fragment hooks over the whole arrays.

The tally: sets of 1, 63, 64, 65 (a wave and its neighbours), 255, 256, 257 (a workgroup and its neighbours) and 1024 * 256 + 1
reads (the first read of a workgroup's second grid-stride step), one-op reads whose FLAG, POS, strand byte and mate keys cycle so
that every counter of ``strand_tally`` (14), ``coverage`` (3 and the bases) and ``coverage(fragments=True)`` (4 and the bases) is
non-zero in the large set; every counter is compared."""
import ctypes

import numpy as np
import pytest

import blockwalkcases as W
import covcases as C
from spliser_amd import native, samio

pytestmark = pytest.mark.gpu

MANY = native.GENE_MANY
SHIFT, LENGTH = -2, 3
GENE_MAP, N_GENES = (np.array([0, 3, 4, 6], np.int32), np.array([1, MANY, 2, 0], np.uint32)), 2
BIN_MAP = (np.arange(8, dtype=np.int32), np.array([1, 2, 3, MANY, 4, 5, 6, 0], np.uint32))          # width-1 bins, one base shared
BIN_GENE = np.array([0, 0, 0, 1, 0, 0], np.uint32)
COVER = (np.array([-1, 1, 2, 5], np.int32), np.array([1, 2, 1, 0], np.uint8))


@pytest.fixture(scope="module")
def ctx():
    with native.Context(0) as c:
        yield c


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _per_read(rs, shift, length, xs=None, cover=None, maps=True):
    """The per-read hooks over every read of ``rs``, called as they are exported: -> dict of depth (per base), cov (seen,
    contributed, past the end, bases), gene (int64[N_GENES + 3]), exon (int64[bins + 4]), strand (int64[14])."""
    lib = native.lib()
    n_bins = BIN_GENE.shape[0]
    diff, cov = np.zeros(length + 1, np.int64), [rs.n, 0, 0, 0]
    gene, exon, strand = np.zeros(N_GENES + 3, np.int64), np.zeros(n_bins + 4, np.int64), np.zeros(14, np.int64)
    cap = int(np.diff(rs.cig_off.astype(np.int64)).max()) if rs.n else 1
    s, e, bins = np.zeros(cap, np.int64), np.zeros(cap, np.int64), np.zeros(64, np.int64)
    n, past, result, verdict, n_hits = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0)
    zero, c_shift = ctypes.c_int(0), ctypes.c_int32(shift)
    cov_args = (c_shift, ctypes.c_int64(length), zero, zero, ctypes.c_int(cap), _ptr(s), _ptr(e), ctypes.byref(n), ctypes.byref(past))
    no_b = (ctypes.c_int64(0), None, None)
    gene_args = (c_shift, zero, ctypes.c_int64(GENE_MAP[0].shape[0]), _ptr(GENE_MAP[0]), _ptr(GENE_MAP[1])) + no_b + (ctypes.c_int64(N_GENES), ctypes.byref(result))
    exon_args = (c_shift, zero, ctypes.c_int64(BIN_MAP[0].shape[0]), _ptr(BIN_MAP[0]), _ptr(BIN_MAP[1])) + no_b + (
        ctypes.c_int64(n_bins), _ptr(BIN_GENE), ctypes.byref(verdict), _ptr(bins), ctypes.c_int64(64), ctypes.byref(n_hits))
    strand_args = None if cover is None else (ctypes.c_int64(cover[0].shape[0]), _ptr(cover[0]), _ptr(cover[1]), _ptr(strand))
    base, off = rs.cigar.ctypes.data, rs.cig_off.tolist()
    pos, flag, tags = rs.pos.tolist(), rs.flag.tolist(), [0] * rs.n if xs is None else xs.tolist()
    for i in range(rs.n):
        head = (ctypes.c_uint32(flag[i]), ctypes.c_int32(pos[i]), ctypes.c_void_p(base + 4 * off[i]), ctypes.c_uint32(off[i + 1] - off[i]))
        assert lib.spl_coverage_rule_host(*(head + cov_args)) == 0
        for a, z in zip(s[:n.value].tolist(), e[:n.value].tolist()):
            diff[a] += 1
            diff[z] -= 1
            cov[3] += z - a
        cov[1] += n.value > 0
        cov[2] += past.value
        if maps:
            assert lib.spl_gene_count_rule_host(*(head + gene_args)) == 0
            gene[result.value if result.value >= 0 else N_GENES - 1 - result.value] += 1
            assert lib.spl_exon_count_rule_host(*(head + exon_args)) == 0
            exon[n_bins - verdict.value] += 1
            for b in bins[:n_hits.value].tolist():
                exon[b] += 1
        if strand_args:
            assert lib.spl_strand_rule_host(head[0], ctypes.c_int32(pos[i] + shift), head[2], head[3], ctypes.c_uint8(tags[i]), *strand_args) == 0
    return dict(depth=np.cumsum(diff)[:length], cov=cov, gene=gene, exon=exon, strand=strand)


def _per_fragment(rs, shift, length, maps=True):
    """The fragment hooks over the whole arrays, mates by the host's mate table: -> dict of depth, cov (... and the pairs), gene, exon."""
    mate, _ = native.mate_table_host(rs, rs.name_key)
    _, _, _, intervals, totals = native.coverage_fragment_rule_host(rs, mate, length, shift, cap=4 * rs.n + 4)
    diff = np.zeros(length + 1, np.int64)
    for a, z in intervals:
        diff[a] += 1
        diff[z] -= 1
    out = dict(depth=np.cumsum(diff)[:length], cov=[totals[k] for k in native.COVERAGE_FRAGMENT_TOTALS[1:]], mate=mate)
    if maps:
        n_bins = BIN_GENE.shape[0]
        result = native.gene_fragment_rule_host(rs, mate, N_GENES, GENE_MAP, shift=shift)
        out["gene"] = np.bincount(np.where(result >= 0, result, N_GENES - 1 - result)[result != -4], minlength=N_GENES + 3)
        verdict, n_hits, bins = native.exon_fragment_rule_host(rs, mate, BIN_GENE, BIN_MAP, shift=shift, cap=16 * rs.n)
        assert bins.shape[0] == int(n_hits.sum())
        out["exon"] = np.bincount(np.concatenate((bins, n_bins - verdict[verdict != -4])), minlength=n_bins + 4)
    return out


class _Set(object):
    """The reads as one finished, fused set added with ``shift``; with their strand bytes and name keys where they have them."""

    def __init__(self, ctx, rs, shift, xs=None):
        self.ctx, self.rs, self.shift, self.xs = ctx, rs, shift, xs

    def __enter__(self):
        arrays = native.ReadArrays(self.rs.pos, self.rs.flag, self.rs.cig_off, self.rs.cigar, xs=self.xs, name_key=self.rs.name_key)
        self.soa = self.ctx.upload_soa([arrays], with_strand=self.xs is not None, with_keys=self.rs.name_key is not None)
        self.dr = self.ctx.begin_reads()
        self.dr.add_soa(self.soa, 0, self.shift)
        self.dr.finish()
        assert self.dr.layout_bytes()[1] == 0          # (the set stays fused)
        return self.dr

    def __exit__(self, *exc):
        self.dr.free()
        self.soa.__exit__(*exc)


def _same_coverage(got, want, fragments=False):
    start, end, depth, totals = got
    runs = C.runs_of(want["depth"])
    names = native.COVERAGE_FRAGMENT_TOTALS if fragments else native.COVERAGE_TOTALS
    assert C.same_runs((start, end, depth), runs)
    assert [totals[k] for k in names] == [runs[0].shape[0]] + [int(v) for v in want["cov"]]


# ---- every CIGAR through the kernels ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def enumerated():
    """The reads, alone and paired i with i + 1 (first and second in pair, one name key a pair; the last read has no partner), and
    the host hooks' sums for both, computed once."""
    cigars = W.all_cigars()
    n = len(cigars)
    pos = 1 + np.arange(n) % 4
    alone = W.read_set(cigars, pos, np.zeros(n, np.uint16))
    keys = ((np.arange(n, dtype=np.uint64) // 2 + 1) << 1)
    paired = W.read_set(cigars, pos, np.where(np.arange(n) % 2 == 0, 0x41, 0x81), name_key=keys)
    want_alone = _per_read(alone, SHIFT, LENGTH, cover=COVER)
    want_strand_paired = _per_read(paired, SHIFT, LENGTH, cover=COVER, maps=False)["strand"]
    want_paired = _per_fragment(paired, SHIFT, LENGTH)
    assert int((want_paired["mate"] != native.MATE_NONE).sum()) == n - 1 and want_paired["cov"][-1] == n // 2
    assert min(want_alone["cov"]) > 5000 and min(want_alone["gene"][:-1]) > 0 and min(want_alone["exon"][:-1]) > 0          # (FLAG 0: every read is counted)
    return dict(alone=alone, paired=paired, want_alone=want_alone, want_paired=want_paired, want_strand_paired=want_strand_paired)


def test_every_cigar_per_read(ctx, enumerated):
    want = enumerated["want_alone"]
    with _Set(ctx, enumerated["alone"], SHIFT) as dr:
        _same_coverage(dr.coverage(LENGTH), want)
        assert dr.gene_counts(N_GENES, GENE_MAP).tolist() == want["gene"].tolist()
        assert dr.exon_counts(BIN_GENE, BIN_MAP).tolist() == want["exon"].tolist()
        assert dr.strand_tally(COVER).tolist() == want["strand"].tolist()


def test_every_cigar_per_fragment(ctx, enumerated):
    """The paired set per fragment; and a set without a mate through the fragment kernels gives the per-read sums."""
    want, alone = enumerated["want_paired"], enumerated["want_alone"]
    with _Set(ctx, enumerated["paired"], SHIFT) as dr:
        assert np.array_equal(dr.mate_table(0, enumerated["paired"].n)[0], want["mate"])
        _same_coverage(dr.coverage(LENGTH, fragments=True), want, fragments=True)
        assert dr.gene_counts(N_GENES, GENE_MAP, fragments=True).tolist() == want["gene"].tolist()
        assert dr.exon_counts(BIN_GENE, BIN_MAP, fragments=True).tolist() == want["exon"].tolist()
        assert dr.strand_tally(COVER).tolist() == enumerated["want_strand_paired"].tolist()
        # the paired reads per read: FLAG 0x41 / 0x81 changes nothing for an unstranded call
        _same_coverage(dr.coverage(LENGTH), alone)
        assert dr.gene_counts(N_GENES, GENE_MAP).tolist() == alone["gene"].tolist()
        assert dr.exon_counts(BIN_GENE, BIN_MAP).tolist() == alone["exon"].tolist()


# ---- the tally at its edges -------------------------------------------------------------------------------------------------------
TALLY_LENGTH = 100
TALLY_COVER = (np.array([1, 50, 99], np.int32), np.array([1, 2, 1], np.uint8))
FLAGS = (0, 16, 0x41, 0x91, 0x51, 0x81, 4)          # unpaired, first and second in pair on both strands; an unmapped read


def _tally_reads(n):
    """n reads of 2M: FLAG cycles through FLAGS, POS through 1, 50, 99 and 100 (a read that loses a base past the end), the strand
    byte through '+', '-' and none; reads 2 j and 2 j + 1 share a name key."""
    i = np.arange(n)
    rs = samio.ReadSet(np.array([1, 50, 99, 100])[i % 4], np.array(FLAGS, np.uint16)[i % 7], np.arange(n + 1), np.full(n, 2 << 4, np.uint32),
                       name_key=(i.astype(np.uint64) // 2 + 1) << 1)
    return rs, np.array([43, 45, 0], np.uint8)[i % 3]


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1024 * 256 + 1])
def test_the_tally_at_its_edges(ctx, n):
    rs, xs = _tally_reads(n)
    per_read = _per_read(rs, 0, TALLY_LENGTH, xs=xs, cover=TALLY_COVER, maps=False)
    per_fragment = _per_fragment(rs, 0, TALLY_LENGTH, maps=False)
    if n > 1000:
        assert min(per_read["strand"]) > 0 and min(per_read["cov"]) > 0 and min(per_fragment["cov"]) > 0          # every counter is non-zero
    with _Set(ctx, rs, 0, xs=xs) as dr:
        assert dr.strand_tally(TALLY_COVER).tolist() == per_read["strand"].tolist()
        _same_coverage(dr.coverage(TALLY_LENGTH), per_read)
        _same_coverage(dr.coverage(TALLY_LENGTH, fragments=True), per_fragment, fragments=True)
