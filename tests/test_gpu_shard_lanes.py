"""The shards of a sample side by side on two lanes (``csrc/spl_lanes.h``): the benchmark's step -- ``relayout``, ``count_launch``,
``sse_launch`` per shard, ``pass_barrier`` -- and its relatives on read sets that went up as ``upload_soa`` + ``layout_read_segments``
(fused: ``relayout`` puts their slots kernel, their range kernel and, on the second lane, their tail on a lane), every result against
the oracle, exactly.  Shapes: A.
thaliana at scale 0.05 (about a million reads, several hundred chunks a chromosome: a range kernel outlasts a launch gap, two of them
really overlap) and one chromosome at 0.002 beside them, whose whole pass ends inside a large one's."""
import numpy as np
import pytest
import torch          # (before the library is loaded: one HIP runtime in the process, as in the other suites that use both)

from spliser_amd import native, sites, synth

pytestmark = pytest.mark.gpu

MODES = [(0, 0), (1, 0), (2, 1), (0, 1), (1, 1), (2, 0)]          # (stranded, combine mode), taking turns between steps


def _table_for(wl, tmp_path):
    bed = str(tmp_path / "j.bed")
    synth.write_bed(bed, wl.genome.chrom_names, wl.junctions)
    table = sites.SiteTable(is_stranded=True)
    table.add_bed(bed)
    table.find_competitors()
    return table


class Want(object):
    """The oracle's counters and SSE results of (table i, reads j), computed on first use and kept."""

    def __init__(self, oracle_lib, arrs, reads):
        self.lib, self.arrs, self.reads, self.counts, self.sses = oracle_lib, arrs, reads, {}, {}

    def counters(self, i, j, st, cb):
        key = (i, j, st, cb)
        if key not in self.counts:
            a, r = self.arrs[i], self.reads[j]
            self.counts[key] = self.lib.check_bam(a.pos, a.strand, a.part_off, a.part_pos, a.comp_off, a.comp_pos, r.pos, r.flag, r.cig_off, r.cigar, st, cb)
        return self.counts[key]

    def sse(self, i, j, st, cb, cryptic):
        key = (i, j, st, cb, bool(cryptic))
        if key not in self.sses:
            a, cnt = self.arrs[i], self.counters(i, j, st, cb)
            self.sses[key] = self.lib.beta2_sse(a.pos, a.part_off, a.part_pos, a.part_site, a.alpha, a.edge_cnt, cnt[0], cnt[1], cnt[2], cryptic)
        return self.sses[key]


@pytest.fixture(scope="module")
def content(tmp_path_factory, oracle_lib):
    """Three chromosomes at 0.05 and one small one at 0.002 (index 3), with their site tables."""
    big = synth.Workload("arabidopsis", scale=0.05, seed=16)
    small = synth.Workload("arabidopsis", scale=0.002, seed=17)
    tb, ts = _table_for(big, tmp_path_factory.mktemp("big")), _table_for(small, tmp_path_factory.mktemp("small"))
    arrs = [tb.chrom_arrays(big.genome.chrom_names[k]) for k in (0, 1, 2)] + [ts.chrom_arrays(small.genome.chrom_names[0])]
    reads = [big.reads[k] for k in (0, 1, 2)] + [small.reads[0]]
    assert all(a.n for a in arrs) and sum(r.n for r in reads[:3]) > 500000 and reads[3].n * 10 < reads[0].n
    return dict(arrs=arrs, reads=reads, want=Want(oracle_lib, arrs, reads))


class Shards(object):
    """Tables and fused read sets of the chosen chromosomes on a context."""

    def __init__(self, ctx, content, which):
        self.ctx, self.content, self.which, self.dev = ctx, content, list(which), []

    def __enter__(self):
        for k in self.which:
            r = self.content["reads"][k]
            soa = self.ctx.upload_soa([native.ReadArrays(r.pos, r.flag, r.cig_off, r.cigar)])
            self.dev.append((self.ctx.upload_sites(native.SiteArrays.from_chrom(self.content["arrs"][k])), self.ctx.layout_read_segments(soa, [0]), soa))
        return self

    def __exit__(self, *exc):
        for ds, dr, soa in self.dev:
            dr.free(); ds.free(); soa.free()

    def step(self, st, cb, cryptic, barrier=True, shards=None):
        for ds, dr, _ in (self.dev if shards is None else [self.dev[k] for k in shards]):
            dr.relayout()
            self.ctx.count_launch(ds, dr, st, cb, 0)
            self.ctx.sse_launch(ds, cryptic)
        if barrier:
            self.ctx.pass_barrier()

    def check(self, n, st, cb, cryptic, reads=None):
        """Shard n's counters and SSE doubles are the oracle's for (its table, `reads` or its own reads) in this mode."""
        i, j = self.which[n], self.which[n] if reads is None else reads
        want = self.content["want"]
        ds = self.dev[n][0]
        for g, w in zip(ds.counters(), want.counters(i, j, st, cb)):
            assert np.array_equal(g, w), (n, st, cb)
        for g, w in zip(ds.sse_results(), want.sse(i, j, st, cb, cryptic)):
            assert np.array_equal(np.asarray(g), np.asarray(w)), (n, st, cb, "sse")


@pytest.mark.parametrize("which", [(0, 1), (0, 3), (3, 0)], ids=["two large", "large then small", "small then large"])
def test_the_bench_step_two_shards(content, which):
    with native.Context(0) as ctx, Shards(ctx, content, which) as sh:
        for step in range(6):
            st, cb = MODES[step]
            if step == 3:                                      # shard 1's pass still queued behind it
                dr = sh.dev[0][1]
                dr.relayout()
                ctx.count_launch(sh.dev[0][0], dr, st, cb, 0)
                ctx.sse_launch(sh.dev[0][0], True)
                dr1 = sh.dev[1][1]
                dr1.relayout()
                ctx.count_launch(sh.dev[1][0], dr1, st, cb, 0)
                ctx.sse_launch(sh.dev[1][0], True)
                sh.check(0, st, cb, True)
                ctx.pass_barrier()
            else:
                sh.step(st, cb, step % 2 == 1)
        st, cb = MODES[5]
        sh.check(1, st, cb, True)
        sh.check(0, st, cb, True)


@pytest.mark.parametrize("which", [(0,), (0, 3, 1)], ids=["one shard", "three shards"])
def test_steps_without_barriers(content, which):
    """``--pipelined``'s shape.  With three shards a set's consecutive passes fall on different lanes."""
    with native.Context(0) as ctx, Shards(ctx, content, which) as sh:
        for step in range(6):
            sh.step(*MODES[step], cryptic=False, barrier=False)
        for n in reversed(range(len(which))):
            sh.check(n, *MODES[5], cryptic=False)
        for step in range(3):
            sh.step(*MODES[step], cryptic=True, barrier=False)
        for n in range(len(which)):
            sh.check(n, *MODES[2], cryptic=True)


def test_one_table_two_sets_and_one_set_two_tables(content):
    with native.Context(0) as ctx, Shards(ctx, content, (0, 3)) as sh:
        (ds0, dr0, _), (ds1, dr1, _) = sh.dev
        for rep in range(5):                                   # one table, two fused read sets taking turns
            for dr in (dr1, dr0):
                dr.relayout()
                ctx.count_launch(ds0, dr, 1, 0, 0)
                ctx.sse_launch(ds0, False)
        sh.check(0, 1, 0, False)
        for rep in range(4):
            for dr in (dr0, dr1):
                dr.relayout()
                ctx.count_launch(ds0, dr, 2, 1, 0)
        ctx.sse_launch(ds0, True)
        sh.check(0, 2, 1, True, reads=3)
        for rep in range(5):                                   # one read set against two tables
            for ds in (ds0, ds1):
                dr1.relayout()
                ctx.count_launch(ds, dr1, 0, 0, 0)
                ctx.sse_launch(ds, False)
        sh.check(1, 0, 0, False)
        sh.check(0, 0, 0, False, reads=3)
        for rep in range(3):                                   # ... and without the layout in between: the set keeps its lane
            for ds in (ds1, ds0):
                ctx.count_launch(ds, dr1, 1, 1, 0)
                ctx.sse_launch(ds, True)
        sh.check(0, 1, 1, True, reads=3)
        sh.check(1, 1, 1, True)


def test_a_range_error_on_one_lane_then_clean_passes_on_both(content):
    far = native.ReadArrays([2147483000], [0], [0, 1], [(1 << 20) << 4])
    with native.Context(0) as ctx, Shards(ctx, content, (0, 3)) as sh:
        with ctx.upload_soa([far]) as soa:
            bad = ctx.layout_read_segments(soa, [0])
            try:
                sh.step(0, 0, False, barrier=False, shards=[0])            # the last range kernel: lane 0, so the bad set takes lane 1
                bad.relayout()
                ctx.count_launch(sh.dev[1][0], bad, 0, 0, 0)
                with pytest.raises(native.SpliserNativeError) as err:
                    sh.dev[1][0].counters()
                assert err.value.code == -6
                sh.check(0, 0, 0, False)
            finally:
                bad.free()
        for step in range(2):                                               # a clean pass on each lane, twice
            sh.step(1, 0, True, barrier=step == 0)
        sh.check(1, 1, 0, True)
        sh.check(0, 1, 0, True)


def test_kernel_timing_has_a_duration_per_launch(content):
    with native.Context(0) as ctx, Shards(ctx, content, (0, 1)) as sh:
        sh.step(0, 0, False)
        ctx.kernel_timing_begin(8)
        for step in range(3):
            sh.step(0, 0, False)
        assert ctx.layout_timing_collect(16) == []             # fused sets: no layout kernel
        ms = ctx.kernel_timing_collect(16)
        assert len(ms) == 6 and all(0 < v < 1000 for v in ms)
        sh.check(0, 0, 0, False)
        sh.check(1, 0, 0, False)


def test_one_stream_gives_the_same_results(content, monkeypatch):
    monkeypatch.setenv("SPL_TAIL_STREAM", "0")
    with native.Context(0) as ctx, Shards(ctx, content, (0, 3)) as sh:
        for step in range(4):
            sh.step(*MODES[step], cryptic=step % 2 == 0, barrier=step % 2 == 0)
        sh.check(1, *MODES[3], cryptic=False)
        sh.check(0, *MODES[3], cryptic=False)


def test_a_context_on_the_callers_stream(content):
    """Behind ``pass_barrier`` the caller's stream stands behind both lanes and the tails: what the caller waits for on ITS stream
    alone is enough for the counters to be finished.  (The library hands out no device pointers: the results are read back through
    it once the caller's own wait is over.)"""
    stream = torch.cuda.Stream()
    with native.Context(0, stream=stream.cuda_stream) as ctx, Shards(ctx, content, (0, 1)) as sh:
        for step in range(4):
            sh.step(*MODES[step], cryptic=True)
        done = torch.cuda.Event()
        done.record(stream)
        done.synchronize()
        sh.check(0, *MODES[3], cryptic=True)
        sh.check(1, *MODES[3], cryptic=True)
        for step in range(2):                                  # ... and work the caller queues in between does not get in the way
            x = torch.zeros(1 << 20, device="cuda")
            with torch.cuda.stream(stream):
                x += 1
            sh.step(*MODES[step], cryptic=False)
        stream.synchronize()
        assert float(x.sum().item()) == float(1 << 20)
        sh.check(1, *MODES[1], cryptic=False)
        sh.check(0, *MODES[1], cryptic=False)
