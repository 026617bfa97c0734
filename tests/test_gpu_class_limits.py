"""The counting kernels on reads at the limits of their record classes (classcases.py: aligned blocks of 65534 ... 70000 bases in
the 16-bit length fields of the SIMPLE, MNM and M2 records and just beyond them, full-word introns and second blocks, reads that
end at SPL_COORD_MAX, each in the spellings that take it through each of the device classifiers), held to the oracle on every
road to the counters: the device path (test_gpu_kernel_limits.run_device: both chunk sizes, layout + range and the fused pass,
every strand and combine mode, relayout and recount, SSE in the scan) and host-packed reads through the range kernel and the pair
kernel, with spl_sse_kernel on the oracle's counters.  Counters bit-equal, SSE as the neighbouring tests hold it."""
import os
import re

import numpy as np
import pytest

import classcases as K
import limitcases as L
from spliser_amd import native
from test_gpu_kernel_limits import _assert_sse, _want, _want_sse, run_device

pytestmark = pytest.mark.gpu

with open(os.path.join(L.ROOT, "include", "spliser.h")) as _fh:
    ERR_RANGE = int(re.search(r"SPL_ERR_RANGE\s*=\s*(-?\d+)", _fh.read()).group(1))


@pytest.fixture(scope="module")
def ctx():
    with native.Context(0) as c:
        yield c


def _host_packed(ctx, oracle_lib, case, wants):
    """The case's reads packed on the host: the range kernel (flags 0) and the pair kernel, every mode; spl_sse_kernel on the
    oracle's counters, with and without beta2Cryptic."""
    sites = case.table.sites()
    r = case.reads
    reads = native.ReadArrays(r.pos, r.flag, r.cig_off, r.cigar)
    for stranded, combine in case.modes:
        want = wants[(stranded, combine)]
        for flags in (0, native.OPT_PAIR_KERNEL):
            for w, g in zip(want, ctx.count(sites, reads, stranded, combine, flags)):
                assert np.array_equal(w, g), (case.name, "host-packed", stranded, combine, flags)
    for stranded in (0, 1):
        want = wants[(stranded, 0)]
        for cryptic in (False, True):
            _assert_sse(ctx.sse(sites, want[0], want[1], want[2], cryptic), _want_sse(oracle_lib, case.table, want, cryptic),
                        (case.name, stranded, cryptic))


class _Once(object):
    """The oracle for one case: every (stranded, combine) counted once and shared by the roads."""

    def __init__(self, lib):
        self.lib, self.memo = lib, {}

    def check_bam(self, *args):
        if args[-2:] not in self.memo:
            self.memo[args[-2:]] = self.lib.check_bam(*args)
        return self.memo[args[-2:]]

    def beta2_sse(self, *args):
        return self.lib.beta2_sse(*args)


def _every_road(ctx, oracle_lib, monkeypatch, case, check=None):
    once = _Once(oracle_lib)
    run_device(ctx, once, monkeypatch, case, check)
    wants = {mode: _want(once, case, *mode) for mode in case.modes}
    _host_packed(ctx, once, case, wants)
    return wants


@pytest.mark.parametrize("name", ["simple", "once_spliced", "twice_spliced", "long_reads"])
def test_reads_at_the_class_limits(name, ctx, oracle_lib, monkeypatch):
    wants = _every_road(ctx, oracle_lib, monkeypatch, K.case(name))
    b1, b2, _ = wants[(0, 0)]
    assert int(b1.sum()) > 0 and int(b2.sum()) > 0


def test_limit_reads_through_the_lists_and_the_literal_queue(ctx, oracle_lib, monkeypatch):
    """`queued`: the limit reads over junctions with more rivals than the range kernel settles, and placed flag-0x4 copies: the
    literal queue (where read_at unpacks the records) holds at least the reads the case declares as listed, in every mode."""
    case = K.case("queued")
    seen = []

    def check(got, stranded, combine, fused, chunk):
        assert got.queued >= case.meta["n_listed"], (stranded, combine, fused, chunk, got.queued, case.meta["n_listed"])
        seen.append(got.queued)
    _every_road(ctx, oracle_lib, monkeypatch, case, check)
    assert len(seen) == 4 * len(case.modes) and case.meta["n_listed"] > 0


def test_reads_that_end_at_the_top_of_the_coordinate_space(ctx, oracle_lib, monkeypatch):
    """`top`: MNM and M2 reads that end at SPL_COORD_MAX, added with a shift against rows placed there.  With their twins that end
    one base later the set is refused with the range error on every road; the same context then counts the good set."""
    case = K.case("top")
    bad_sites = case.table.sites()
    b = L.concat(case.meta["bad_segments"])
    bad_reads = native.ReadArrays(b.pos, b.flag, b.cig_off, b.cigar)
    for chunk in (L.CHUNK, L.CHUNK_BIG):
        for fused in (False, True):
            monkeypatch.setenv("SPL_FORCE_CHUNK", str(chunk))
            monkeypatch.setenv("SPL_FUSED", "1" if fused else "0")
            for stranded, combine in case.modes:
                with pytest.raises(native.SpliserNativeError) as err:
                    L.count_device(ctx, bad_sites, case.meta["bad_segments"], stranded, combine, False)
                assert err.value.code == ERR_RANGE, (chunk, fused, stranded, combine, str(err.value))
    monkeypatch.delenv("SPL_FORCE_CHUNK")
    monkeypatch.delenv("SPL_FUSED")
    for stranded, combine in case.modes:
        for flags in (0, native.OPT_PAIR_KERNEL):
            with pytest.raises(native.SpliserNativeError) as err:
                ctx.count(bad_sites, bad_reads, stranded, combine, flags)
            assert err.value.code == ERR_RANGE, (flags, stranded, combine, str(err.value))
    wants = _every_road(ctx, oracle_lib, monkeypatch, case)
    top_rows = case.table.pos >= K.COORD_MAX - 2
    assert int(wants[(0, 0)][0][top_rows].sum()) > 0 and int(wants[(0, 0)][1].sum()) > 0
