"""Every decode switch at once -- a read filter, ``aux_strand``, ``flagstat`` and ``any_order`` (``spl_bam_decode_opts``) -- and what
the decode counted under them (``spl_bam_totals``), where the suites of the single switches do not look: totals added over many
batches, windows and shares, and an option lost when all are set.  One file of three references, XS-tagged spliced reads, low
MAPQs, secondary and duplicate records and three records without a reference, written in coordinate order and shuffled
(``ordercases``); the expectations are the restatements of ``ordercases``, ``xscases``, ``filtercases`` and ``flagstatcases``.
Everything is exact."""
import numpy as np
import pytest

import filtercases as F
import flagstatcases as fc
import ordercases as O
import xscases as X
from spliser_amd import native, samio

NAMES = ["a", "b", "c"]
FILT = (10, 0, 0x400)      # samtools view -q 10 -F 0x400
BLOCK = 4096               # (BGZF payload: some eighty blocks, so that batches, windows and shares are many)


class Case(object):
    def __init__(self, d):
        rng = np.random.default_rng(20261018)
        sets, tags, mapq = [], [], []
        for _ in NAMES:
            rs = X.make_reads(rng, 1500)        # (0x100 on six reads in a hundred)
            flag = np.asarray(rs.flag, np.int64) | np.where(rng.random(rs.n) < 0.07, 0x400, 0)
            sets.append(samio.ReadSet(rs.pos, flag, rs.cig_off, rs.cigar))
            tags.append(X.make_tags(rng, rs)[0])
            mapq.append(rng.integers(0, 61, rs.n))
        unplaced = [(-1, 0, 0x4, 0, [], b""), (-1, 0, 0x4 | 0x200, 255, [], b""), (-1, 0, 0x4 | 0x1 | 0x8 | 0x40, 30, [], b"")]
        self.in_order = O.records_of(sets, tags=tags, mapq=mapq) + unplaced
        self.mixed = O.shuffled(self.in_order, 7)
        self.sorted_path, self.shuffled_path = str(d / "sorted.bam"), str(d / "shuffled.bam")
        O.write_bam(self.sorted_path, NAMES, [10 ** 6] * 3, self.in_order, so="coordinate", block=BLOCK)
        O.write_bam(self.shuffled_path, NAMES, [10 ** 6] * 3, self.mixed, so="unsorted", block=BLOCK)
        # what does not depend on the records' order: the counts
        tid, pos, flag, q = (np.array([r[k] for r in self.in_order], np.int64) for k in range(4))
        placed = (tid >= 0) & (pos >= 1)
        kept, by_flags, by_mapq = F.keep_mask(flag, q, FILT)
        self.n_records = len(self.in_order)
        self.dropped = (int((by_flags & placed).sum()), int((by_mapq & placed).sum()))
        self.n_placed = int((kept & placed).sum())
        self.flagstat = fc.restate_filtered(flag, tid, np.full(len(tid), -1), q, FILT)      # (ordercases.record: no mate reference)
        assert min(self.dropped) > 0 and int((kept & ~placed).sum()) == 2 and int((flag & 0x100 != 0).sum()) > 0

    def check(self, bam, records, sorted_by):
        """``bam`` decoded the file that holds ``records`` in this order under all four switches.  ``sorted_by``: None = the file
        was in order, False = the host threads had to sort it, True = the device."""
        assert bam.wait_all() is True
        want = O.expected(records, len(NAMES), FILT)
        assert sum(w.n for w, _ in want.values()) == self.n_placed
        for t, name in enumerate(NAMES):
            got = bam.reads(name)
            assert O.same_reads(got, want[t][0]), name
            assert np.array_equal(got.xs, X.expected_xs(want[t][0], want[t][1])), name
        assert bam.filter_counts() == self.dropped
        assert bam.n_records == self.n_records
        assert np.array_equal(bam.flagstat(), self.flagstat)
        assert bam.any_order_sorted() == ((0, False) if sorted_by is None else (self.n_placed, sorted_by))


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    native.build()
    return Case(tmp_path_factory.mktemp("alloptions"))


ALL = dict(min_mapq=FILT[0], require_flags=FILT[1], exclude_flags=FILT[2], aux_strand=True, flagstat=True, any_order=True)


@pytest.mark.parametrize("threads", [1, 4])
@pytest.mark.parametrize("env", [{}, {"SPL_BAM_BATCH_BLOCKS": "1"}, {"SPL_BAM_BATCH_BLOCKS": "2", "SPL_BAM_FORCE_RESYNC": "1"}], ids=["default", "batch=1", "resync"])
def test_host_decode_under_all_switches(case, threads, env, monkeypatch):
    for k, v in env.items():
        monkeypatch.setenv(k, v)      # (batch=1: the totals of some eighty batches added up; resync: every batch through the committing thread's walk)
    for path, records, sorted_by in ((case.shuffled_path, case.mixed, False), (case.sorted_path, case.in_order, None)):
        bam = native.BamFile(path, threads=threads, **ALL)
        try:
            assert (bam.filter, bam.aux_strand, bam.counts_flagstat, bam.any_order) == (FILT, True, True, True)
            case.check(bam, records, sorted_by)
        finally:
            bam.close()


@pytest.fixture(scope="module")
def ctx():
    with native.Context(0) as c:
        yield c


@pytest.mark.gpu
@pytest.mark.parametrize("window", [None, "2"])
def test_device_decode_under_all_switches(case, ctx, window, monkeypatch):
    if window:
        monkeypatch.setenv("SPL_INFLATE_WINDOW_BLOCKS", window)      # (some forty windows: records straddle them, a block that waits is counted once)
    bam = native.BamFile(case.shuffled_path, threads=2, defer=True, **ALL)
    try:
        assert bam.decode_on_device(ctx) is True, bam.decline_reason()
        case.check(bam, case.mixed, True)
    finally:
        bam.close()


@pytest.mark.gpu
def test_shares_add_up_to_the_host_decode(case, ctx):
    """The sorted file in three shares (which refuse ``any_order``): the shares' totals added are the host decoder's."""
    kw = dict(ALL, any_order=False)
    dev, host = native.BamFile(case.sorted_path, threads=2, defer=True, **kw), native.BamFile(case.sorted_path, threads=2, **kw)
    try:
        assert len(dev.decode_on_devices_async([0, 0, 0])) == 3
        assert dev.join_decoders() is True, dev.decline_reason()
        assert dev.filter_counts() == host.filter_counts() == case.dropped
        assert dev.n_records == host.n_records == case.n_records
        assert np.array_equal(dev.flagstat(), host.flagstat()) and np.array_equal(dev.flagstat(), case.flagstat)
        for name in NAMES:
            d, h = dev.reads(name), host.reads(name)
            assert O.same_reads(d, h) and h.n > 0 and np.array_equal(d.xs, h.xs), name
    finally:
        dev.close()
        host.close()
