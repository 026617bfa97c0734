"""``exoncounts`` on the device: ``spl_exon_count`` on fused sets against the yardstick of ``exoncases.py`` -- exactly, the sums being
integers -- at the sizes where the kernel's geometry changes, on a bin that takes every read and on a bin change every lane, on
reads of more bins than a wave has lanes, on verdicts that fall with a read's last block, on maps below and beyond the LDS top
level, on reads in any order, stranded and not; its refusals; its agreement with ``spl_gene_count``; the decodes through
``counts_of_source``; the command line, whose two files are compared byte for byte."""
import re

import numpy as np
import pytest

import exoncases as X
import genecases as G
import ordercases as O
from spliser_amd import cli, exoncounts as xc, genecounts as gc, native, process as proc, samio

pytestmark = pytest.mark.gpu


def _constant(name):
    """A geometry constant of csrc/spl_exoncount.h, read from the header."""
    import os
    text = open(os.path.join(os.path.dirname(os.path.abspath(native.__file__)), "csrc", "spl_exoncount.h")).read()
    return int(re.search(r"#define %s (\d+)" % name, text).group(1))


# A workgroup takes TILE reads a grid-stride step, a read a lane, and a launch has at most GRID_MAX workgroups: LARGE gives every
# workgroup a second step and the first one a third.  TOP entries of a map's top level are in LDS; a map beyond it is searched in
# global memory too.
TILE, GRID_MAX, TOP = _constant("SPL_EXON_TILE"), _constant("SPL_EXON_GRID_MAX"), _constant("SPL_EXON_TOP")
LARGE = 2 * GRID_MAX * TILE + 1
BYTE = {"+": 43, "-": 45, ".": 46}


@pytest.fixture(scope="module")
def ctx():
    with native.Context(0) as c:
        yield c


def _device(ctx, rs, bin_gene, a, b=None, stranded=0, shift=0):
    n_bins = len(bin_gene)
    with ctx.upload_soa([native.ReadArrays(rs.pos, rs.flag, rs.cig_off, rs.cigar)]) as soa:
        with ctx.begin_reads() as dr:
            dr.add_soa(soa, 0, shift)
            dr.finish()
            got = dr.exon_counts(bin_gene, a, b, stranded)
            if rs.n:
                assert dr.layout_bytes()[1] == 0          # (the set stays fused)
            assert got.dtype == np.int64 and got.shape == (n_bins + 4,) and int(got[n_bins:].sum()) == rs.n
            return got.tolist()


def _arrays(features):
    return (np.array([f[0] for f in features], np.int64), np.array([f[1] for f in features], np.int64), np.array([BYTE[f[2]] for f in features], np.uint8),
            np.array([f[3] for f in features], np.int64))


def _permuted(rs, perm):
    n_ops = np.diff(rs.cig_off.astype(np.int64))[perm]
    off = np.concatenate(([0], np.cumsum(n_ops)))
    take = np.repeat(rs.cig_off.astype(np.int64)[perm] - off[:-1], n_ops) + np.arange(int(off[-1]))
    return samio.ReadSet(rs.pos[perm], rs.flag[perm], off, rs.cigar[take])


def _short_reads(pos, length=2):
    """Reads of one aligned op of ``length`` bases, built as arrays."""
    n = len(pos)
    return samio.ReadSet(np.asarray(pos, np.int32), np.zeros(n, np.uint16), np.arange(n + 1), np.full(n, (length << 4) | 0, np.uint32))


def _maps_of(features, stranded):
    a, b, (bin_gene, bin_start, bin_end) = xc.exon_maps(*_arrays(features), stranded=bool(stranded))
    return a, b, bin_gene.astype(np.uint32), list(zip(bin_start.tolist(), bin_end.tolist(), bin_gene.tolist()))


N_GENES, LENGTH = 9, 6000


@pytest.fixture(scope="module")
def content():
    """Random features of every kind on 6000 bases with their bin maps, 4000 random reads of every kind, and the yardstick's verdict
    and hit list per read (unstranded, fr, rf), computed once."""
    rng = np.random.default_rng(20261020)
    features = G.random_features(rng, LENGTH - 700, N_GENES, 30)
    rs = samio.ReadSet.from_records(G.random_records(rng, 4000, LENGTH - 700))
    plain, both = _maps_of(features, False), _maps_of(features, True)
    labels = X.labels_of_features(features, LENGTH)
    strands = {w: X.labels_of_features(features, LENGTH, w) for w in "+-"}
    assert plain[3] == X.bins_of([labels]) and both[3] == X.bins_of([strands["+"], strands["-"]])
    shared_by_both = set(X.bins_of([strands["+"]])) & set(X.bins_of([strands["-"]]))
    assert shared_by_both and len(shared_by_both) < len(both[3])                                   # two maps that share bins, and differ
    results = {0: X.reads_of(rs, labels), 1: X.reads_of(rs, strands, 1), 2: X.reads_of(rs, strands, 2)}
    assert {0, 16, 99, 147, 83, 163, 4, 256, 512, 1024, 2048} == set(rs.flag.tolist()) and int(rs.pos.min()) == 0 and int(np.diff(rs.cig_off.astype(np.int64)).min()) == 0
    want = {s: X.counts_of(results[s], {k: i for i, k in enumerate((plain if s == 0 else both)[3])}, len((plain if s == 0 else both)[3])) for s in (0, 1, 2)}
    return dict(features=features, rs=rs, plain=plain, both=both, results=results, want=want)


# ---- 1: sizes -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, TILE - 1, TILE, TILE + 1])
def test_sizes_around_a_wave_and_a_tile(ctx, content, n):
    a, _, bin_gene, bins = content["plain"]
    rs = content["rs"].take(1000, 1000 + n)
    want = X.counts_of(content["results"][0][1000:1000 + n], {k: i for i, k in enumerate(bins)}, len(bins))
    assert sum(want[len(bins):]) == n
    assert _device(ctx, rs, bin_gene, a) == want


# ---- 2, 3, 4: hot bins, changing bins, run boundaries ----------------------------------------------------------------------------
def test_a_bin_that_takes_every_read_of_a_set_that_gives_every_workgroup_more_than_one_step(ctx):
    """The hot bin: LARGE reads of two bases, sorted, all inside bin 3 of 5.  The count is exact, and a wave makes one add."""
    rng = np.random.default_rng(7)
    a = (np.array([1000, 3000], np.int32), np.array([4, 0], np.uint32))
    bin_gene = np.arange(5, dtype=np.uint32)
    rs = _short_reads(np.sort(rng.integers(1001, 2990, LARGE)))
    results = X.reads_of(rs, X.MapLabels(a[0], a[1], bin_gene))
    assert results[0] == results[-1] == (X.COUNTED, [3]) and X.adds_of(results) == ((LARGE + 63) // 64, LARGE)
    assert X.counts_of(results, None, 5) == [0, 0, 0, LARGE, 0, LARGE, 0, 0, 0]
    assert _device(ctx, rs, bin_gene, a) == [0, 0, 0, LARGE, 0, LARGE, 0, 0, 0]


def test_a_bin_change_every_lane_at_the_same_size(ctx):
    """Neighbouring reads in 2000 bins of four bases in turn: every lane is a head, one add a read."""
    n_bins = 2000
    a = ((1000 + 4 * np.arange(n_bins + 1)).astype(np.int32), np.concatenate((np.arange(1, n_bins + 1), [0])).astype(np.uint32))
    bin_gene = np.full(n_bins, 5, np.uint32)
    rs = _short_reads(1001 + 4 * (np.arange(LARGE) % n_bins))                  # read i lies in bin i % 2000
    results = X.reads_of(rs, X.MapLabels(a[0], a[1], bin_gene))
    assert [r[1] for r in results[:3]] == [[0], [1], [2]] and X.adds_of(results) == (LARGE, LARGE)
    want = X.counts_of(results, None, n_bins)
    assert want[n_bins] == LARGE and max(want[:n_bins]) - min(want[:n_bins]) == 1
    assert _device(ctx, rs, bin_gene, a) == want


def test_runs_that_cross_a_wave_and_a_tile_boundary_in_the_first_and_the_last_bin(ctx):
    """Sorted reads over stretches of 1000 bins' codes in turn: runs of 60, 10, 190, 3, 64, 1, 250, ... reads, so that runs end
    before, on and behind lanes 63 / 64 and the tile's edge, in bin 0 and in bin n_bins - 1 among others.  (A test's map may name a
    bin in two stretches: the yardstick keys a hit by its bin, and no read here reaches two stretches.)"""
    n_bins = 1000
    lengths = [60, 10, 190, 3, 64, 1, TILE - 6, 62, 128, TILE, 65, 2 * TILE - 65, 63, 1, 1, 2 * TILE - 2]
    which = [0, n_bins - 1, 5, 0, 17, n_bins - 1, 400, 0, 1, n_bins - 1, 2, 998, 0, 999, 0, 999]
    a = ((100 * np.arange(1, len(lengths) + 2)).astype(np.int32), np.array([b + 1 for b in which] + [0], np.uint32))
    bin_gene = (np.arange(n_bins) % 7).astype(np.uint32)
    rs = _short_reads(np.concatenate([np.sort(100 * (k + 1) + 1 + (np.arange(n) % 90)) for k, n in enumerate(lengths)]))
    results = X.reads_of(rs, X.MapLabels(a[0], a[1], bin_gene))
    want = X.counts_of(results, None, n_bins)
    assert [want[0], want[n_bins - 1]] == [sum(n for n, b in zip(lengths, which) if b == 0), sum(n for n, b in zip(lengths, which) if b == n_bins - 1)]
    assert rs.n > 6 * TILE and _device(ctx, rs, bin_gene, a) == want


# ---- 5, 6, 7: many hits, late verdicts, deduplication ----------------------------------------------------------------------------
# gene 0: bins 0 (100..200) and 1 (200..300; they abut); gene 1: bin 2 (400..500); shared 600..700; gene 0 again: 70 bins of ten
# bases from 1000 on
CASE_START = [100, 200, 300, 400, 500, 600, 700] + [1000 + 10 * k for k in range(71)]
CASE_CODE = [1, 2, 0, 3, 0, G.MANY, 0] + [4 + k for k in range(70)] + [0]
CASE_GENE = np.array([0, 0, 1] + [0] * 70, np.uint32)
CASE_MAP = (np.array(CASE_START, np.int32), np.array(CASE_CODE, np.uint32))


def _case_labels():
    return X.MapLabels(CASE_START, CASE_CODE, CASE_GENE)


@pytest.mark.parametrize("where", [0, 63])
def test_a_read_over_70_bins_in_a_wave_of_one_bin_reads(ctx, where):
    """More bins than a wave has lanes, from one single-op read: its wave goes 70 rounds, the others' bins unharmed."""
    recs = [(0, 1051, "5M")] * 64 + [(0, 151, "10M")] * 70
    recs[where] = (0, 991, "800M")
    rs = samio.ReadSet.from_records(recs)
    results = X.reads_of(rs, _case_labels())
    assert results[where] == (X.COUNTED, list(range(3, 73))) and results[1] == (X.COUNTED, [8])
    want = X.counts_of(results, None, 73)
    assert want[8] == 64 and want[0] == 70 and want[73:] == [134, 0, 0, 0] and sum(want[:73]) == 63 + 70 + 70
    assert _device(ctx, rs, CASE_GENE, CASE_MAP) == want


def test_verdicts_that_fall_with_the_last_block_add_to_no_bin(ctx):
    recs = [(0, 151, "10M239N10M"),             # the first block in gene 0 (bin 0), the last in gene 1 (bin 2)
            (0, 151, "10M439N10M"),             # the last block in the shared stretch
            (0, 1001, "700M"), (0, 451, "10M540N700M")]          # 70 bins of gene 0 counted; gene 1 and then the same 70: ambiguous
    rs = samio.ReadSet.from_records(recs)
    results = X.reads_of(rs, _case_labels())
    assert [r[0] for r in results] == [X.AMBIGUOUS, X.AMBIGUOUS, X.COUNTED, X.AMBIGUOUS]
    want = X.counts_of(results, None, 73)
    assert want == [0, 0, 0] + [1] * 70 + [1, 0, 3, 0]
    assert _device(ctx, rs, CASE_GENE, CASE_MAP) == want
    two = samio.ReadSet.from_records(recs[:2])
    assert _device(ctx, two, CASE_GENE, CASE_MAP) == [0] * 73 + [0, 0, 2, 0]          # both add to no bin


def test_a_stretch_is_taken_once_and_stretch_edges_are_exact(ctx):
    cases = [("a deletion and an intron inside one bin: once", "10M5D10M20N10M", 111, [0]),
             ("two blocks in abutting bins of one gene: each once", "5M10N5M", 191, [0, 1]),
             ("three blocks over the two", "4M2N4M2N4M", 193, [0, 1]),
             ("a block that ends exactly at a stretch's start", "10M", 91, None),
             ("a block that begins exactly there", "10M", 101, [0]),
             ("a block on a bin's last base", "10M", 300, [1]),
             ("a block that begins exactly where the bins end", "10M", 301, None)]
    rs = samio.ReadSet.from_records([(0, pos, cigar) for _, cigar, pos, _ in cases])
    results = X.reads_of(rs, _case_labels())
    assert results == [(X.COUNTED, bins) if bins else (X.NO_FEATURE, []) for _, _, _, bins in cases]
    want = X.counts_of(results, None, 73)
    assert want[:3] == [4, 3, 0] and want[73:] == [5, 2, 0, 0]
    assert _device(ctx, rs, CASE_GENE, CASE_MAP) == want
    for k, case in enumerate(cases):
        one = samio.ReadSet.from_records([(0, case[2], case[1])])
        assert _device(ctx, one, CASE_GENE, CASE_MAP) == X.counts_of(results[k:k + 1], None, 73), case[0]


# ---- 8: maps ------------------------------------------------------------------------------------------------------------------
def _map_of(rng, n):
    """n entries of which a read can still lie in a stretch: clusters of forty entries a base apart, each followed by a stretch
    of a hundred bases or more -- of a large map the top level in LDS finds the cluster, the search in global memory the entry.
    Entry k is nothing, shared, or bin k of gene (k // 90) % 3: reads over two clusters meet one gene or two."""
    clusters = (n + 39) // 40
    anchors = 140 * np.arange(1, clusters + 1) + rng.integers(0, 50, clusters)
    start = (anchors[:, None] + np.arange(40)[None, :]).ravel()[:n]
    kind = rng.choice(3, n, p=[0.3, 0.65, 0.05])
    code = np.where(kind == 0, 0, np.where(kind == 1, np.arange(1, n + 1), G.MANY)).astype(np.uint32)
    if n <= 2:
        code = np.array([n, G.MANY], np.uint32)[:n]          # (the last bin from the first entry on; then shared to the end)
    assert (np.diff(start) > 0).all()
    return (start.astype(np.int32), code), ((np.arange(n) // 90) % 3).astype(np.uint32)


@pytest.mark.parametrize("n_map", [0, 1, 2, TOP - 1, TOP, TOP + 1, 40000])
def test_maps_below_at_and_beyond_the_top_level(ctx, n_map):
    """Reads lie below the first entry and beyond the last, too."""
    rng = np.random.default_rng(300 + n_map)
    a, bin_gene = _map_of(rng, n_map)
    span = int(a[0][-1]) + 300 if n_map else 5000
    edges = [(0, 5, "30M"), (0, 50, "20M5000N20M"), (0, span - 310, "50M"), (16, span + 500, "30M")]          # below the first entry, over it, over the last, beyond it
    rs = samio.ReadSet.from_records(sorted(G.random_records(rng, 3000, span) + edges, key=lambda r: r[1]))
    results = X.reads_of(rs, X.MapLabels(a[0], a[1], bin_gene))
    want = X.counts_of(results, None, n_map)
    if n_map == 0:
        assert want == [0, want[1], 0, want[3]] and want[1] > 2000          # every eligible read: no feature
    elif n_map > 2:
        assert min(want[n_map:]) > 0 and max(len(r[1]) for r in results) > 20
    assert _device(ctx, rs, bin_gene, a) == want
    perm = rng.permutation(rs.n)
    assert _device(ctx, _permuted(rs, perm), bin_gene, a) == want


# ---- 9: content, strandedness and shift -------------------------------------------------------------------------------------------
def test_reads_of_every_kind_and_in_any_order(ctx, content):
    a, _, bin_gene, bins = content["plain"]
    rs, want = content["rs"], content["want"][0]
    assert min(want[len(bins):]) > 0 and sum(1 for c in want[:len(bins)] if c) >= 10 and max(len(r[1]) for r in content["results"][0]) >= 3
    assert _device(ctx, rs, bin_gene, a) == want
    prs = _permuted(rs, np.random.default_rng(5).permutation(rs.n))
    assert not np.array_equal(prs.pos, rs.pos)
    assert _device(ctx, prs, bin_gene, a) == want


def test_a_set_moved_by_a_shift_is_counted_where_it_lies(ctx, content):
    """Map coordinates are the set's: a segment added with a shift meets the map moved by as much."""
    a, _, bin_gene, _ = content["plain"]
    rs, want, shift = content["rs"], content["want"][0], 5000000
    assert _device(ctx, rs, bin_gene, (a[0] + shift, a[1]), shift=shift) == want
    assert _device(ctx, rs, bin_gene, a, shift=shift) != want          # (the map left where it was: the reads are elsewhere)


@pytest.mark.parametrize("stranded", [1, 2])
def test_stranded_with_two_maps_that_share_bins(ctx, content, stranded):
    a, b, bin_gene, _ = content["both"]
    rs, want = content["rs"], content["want"][stranded]
    assert want != content["want"][3 - stranded]
    assert _device(ctx, rs, bin_gene, a, b, stranded) == want
    assert _device(ctx, rs, bin_gene, b, a, 3 - stranded) == want          # rf is fr with the maps exchanged


# ---- 10: the ABI --------------------------------------------------------------------------------------------------------------
def test_counts_are_added_to_what_the_caller_holds(ctx, content):
    a, _, bin_gene, bins = content["plain"]
    rs, want = content["rs"], content["want"][0]
    with ctx.upload_soa([native.ReadArrays(rs.pos, rs.flag, rs.cig_off, rs.cigar)]) as soa:
        with ctx.begin_reads() as dr:
            dr.add_soa(soa, 0)
            dr.finish()
            out = np.arange(len(bins) + 4, dtype=np.int64) * 1000
            assert dr.exon_counts(bin_gene, a, out=out) is out
            dr.exon_counts(bin_gene, a, out=out)
            assert out.tolist() == [1000 * k + 2 * w for k, w in enumerate(want)]


def test_refusals_leave_the_context_working(ctx, content):
    a, _, bin_gene, bins = content["plain"]
    rs, want, n_bins = content["rs"], content["want"][0], len(content["plain"][3])
    arrays = native.ReadArrays(rs.pos, rs.flag, rs.cig_off, rs.cigar)
    dr = ctx.upload_reads(arrays)                  # (packed on the host: records, not arrays)
    try:
        with pytest.raises(native.SpliserNativeError, match="fused") as err:
            dr.exon_counts(bin_gene, a)
        assert err.value.code == -1
    finally:
        dr.free()
    with ctx.upload_soa([arrays]) as soa:
        with ctx.begin_reads() as dr:
            with pytest.raises(native.SpliserNativeError, match="not finished") as err:
                dr.exon_counts(bin_gene, a)
            assert err.value.code == -1
            dr.add_soa(soa, 0)
            dr.finish()
            out = np.zeros(n_bins + 4, np.int64)
            for bad in ((np.array([30, 20, 10], np.int32), np.array([1, 2, 1], np.uint32)), (np.array([10, 20, 20], np.int32), np.array([1, 2, 1], np.uint32))):
                for maps in ((bad, None), (a, bad)):
                    with pytest.raises(native.SpliserNativeError, match="ascending") as err:
                        dr.exon_counts(bin_gene, *maps, out=out)
                    assert err.value.code == -1
            for code in (n_bins + 1, 0xFFFFFFFE, 2 ** 31):
                for maps in (((np.array([10, 20], np.int32), np.array([1, code], np.uint32)), None), (a, (np.array([10, 20], np.int32), np.array([1, code], np.uint32)))):
                    with pytest.raises(native.SpliserNativeError, match="code") as err:
                        dr.exon_counts(bin_gene, *maps, out=out)
                    assert err.value.code == -1
            for stranded in (-1, 3):
                with pytest.raises(native.SpliserNativeError, match="stranded") as err:
                    dr.exon_counts(bin_gene, a, None, stranded, out=out)
                assert err.value.code == -1
            i64, none, genes = native.ctypes.c_int64, None, native._ptr(bin_gene)
            for args, match in (((ctx._h, dr._h, 0, i64(0), none, none, i64(0), none, none, i64(n_bins), genes, none), "null"),                      # no counts
                                ((ctx._h, dr._h, 0, i64(2), none, none, i64(0), none, none, i64(n_bins), genes, native._ptr(out)), "null"),          # a map of two entries that is not there
                                ((ctx._h, none, 0, i64(0), none, none, i64(0), none, none, i64(n_bins), genes, native._ptr(out)), "null"),           # no read set
                                ((ctx._h, dr._h, 0, i64(0), none, none, i64(0), none, none, i64(n_bins), none, native._ptr(out)), "null"),           # bins without their genes
                                ((ctx._h, dr._h, 0, i64(0), none, none, i64(0), none, none, i64(0xFFFFFFF1), genes, native._ptr(out)), "n_bins"),    # above SPL_GENE_INDEX_MAX
                                ((ctx._h, dr._h, 0, i64(0), none, none, i64(0), none, none, i64(-1), genes, native._ptr(out)), "n_bins")):
                with pytest.raises(native.SpliserNativeError, match=match) as err:
                    native._check(native.lib().spl_exon_count(*args))
                assert err.value.code == -1
            assert not out.any()                                   # (a refusal adds nothing)
            top = (np.array([10, 3000], np.int32), np.array([n_bins, G.MANY], np.uint32))                          # the greatest code there is
            want_top = X.counts_of(X.reads_of(rs, X.MapLabels(top[0], top[1], bin_gene)), None, n_bins)
            assert want_top[n_bins - 1] == want_top[n_bins] > 0 and want_top[n_bins + 2] > 0 and dr.exon_counts(bin_gene, top).tolist() == want_top
            assert dr.exon_counts(np.zeros(0, np.uint32), None).tolist() == [0, want[n_bins] + want[n_bins + 1] + want[n_bins + 2], 0, want[n_bins + 3]]      # no bin: no feature
            assert dr.exon_counts(bin_gene, a).tolist() == want
    assert _device(ctx, rs, bin_gene, a) == want


# ---- 11: equivalence with spl_gene_count ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("stranded", [0, 1, 2])
def test_the_verdicts_are_spl_gene_counts_on_the_gene_maps_of_the_same_features(ctx, content, stranded):
    features, rs = content["features"], content["rs"]
    a, b, bin_gene, bins = content["both"] if stranded else content["plain"]
    ga, gb = gc.gene_maps(*_arrays(features), stranded=bool(stranded))
    with ctx.upload_soa([native.ReadArrays(rs.pos, rs.flag, rs.cig_off, rs.cigar)]) as soa:
        with ctx.begin_reads() as dr:
            dr.add_soa(soa, 0)
            dr.finish()
            genes = dr.gene_counts(N_GENES, ga, gb, stranded).tolist()
            exons = dr.exon_counts(bin_gene, a, b, stranded).tolist()
    assert exons[len(bins):] == [sum(genes[:N_GENES])] + genes[N_GENES:] and min(exons[len(bins):]) > 0
    # ... and read by read on the host, whose rule is the kernel's: a counted read's bins are its gene's
    both = {w: G.bases_of_features(features, LENGTH, w) for w in "+-"} if stranded else G.bases_of_features(features, LENGTH)
    for (verdict, keys), gene in zip(content["results"][stranded], G.results_of(rs, both, stranded)):
        assert verdict == (X.COUNTED if gene >= 0 else gene) and all(k[2] == gene for k in keys)


# ---- 12: the decodes and the command ------------------------------------------------------------------------------------------
NAMES, LENGTHS = ["c1", "c2", "c3"], [10 ** 6] * 3
IDS = ["gene%02d" % k for k in range(12)]
SPAN = 20000


def _gtf_text(features_by_chrom):
    text = "##gtf of the tests\n"
    for chrom in ("c2", "c1"):                     # (the annotation's order is not the alignment file's)
        for k, (left, right, strand, gene) in enumerate(features_by_chrom.get(chrom, [])):
            attrs = ('gene_id "%s"; transcript_id "t%d";' % (IDS[gene], k)) if k % 2 else ("ID=e%d;gene_id=%s" % (k, IDS[gene]))
            text += "%s\tsynth\texon\t%d\t%d\t.\t%s\t.\t%s\n" % (chrom, left + 1, right, strand, attrs)
            if k % 5 == 0:
                text += "%s\tsynth\tCDS\t%d\t%d\t.\t%s\t0\tgene_id \"other\";\n" % (chrom, left + 1, right, strand)
    return text


@pytest.fixture(scope="module")
def decode_files(tmp_path_factory):
    """Three chromosomes of 3000 reads (more than eight BGZF blocks: a file of fewer is not cut into shares); genes 0..7 on c1,
    4..11 on c2 (four genes have bins on both), none on c3; as a sorted BAM, its SAM text and a shuffled BAM.  The yardstick's
    bins per chromosome and verdicts and hit lists per read for unstranded, fr and rf, computed once."""
    d = tmp_path_factory.mktemp("xdec")
    rng = np.random.default_rng(37)
    sets, features = [], {}
    for k, chrom in enumerate(NAMES):
        recs = [r for r in G.random_records(rng, 3200, SPAN) if r[1] >= 1 and r[2]][:3000]
        sets.append((chrom, samio.ReadSet.from_records(recs)))
        if k < 2:
            features[chrom] = [(l, r, s, g + 4 * k) for l, r, s, g in G.random_features(rng, SPAN, 8, 40)]
    bam, sam, mixed, gtf = str(d / "d.bam"), str(d / "d.sam"), str(d / "mixed.bam"), str(d / "genes.gtf")
    samio.write_bam(bam, NAMES, LENGTHS, sets, with_seq=True, unplaced=3)
    with open(sam, "w") as fh:
        fh.write("@HD\tVN:1.6\tSO:coordinate\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % (n, ln) for n, ln in zip(NAMES, LENGTHS)))
        for chrom, rs in sets:
            for k in range(rs.n):
                fh.write("\t".join(["r", str(rs.flag[k]), chrom, str(rs.pos[k]), "60", samio.cigar_string(rs.cigar[rs.cig_off[k]:rs.cig_off[k + 1]]), "*", "0", "0", "*", "*"]) + "\n")
    O.write_bam(mixed, NAMES, LENGTHS, O.shuffled(O.records_of([rs for _, rs in sets]), 11))
    text = _gtf_text(features)
    open(gtf, "w").write(text)
    ids, by_chrom = G.features_of_text(text)
    assert ids == IDS and list(by_chrom) == ["c2", "c1"]
    bins, results = {}, {}
    for stranded in (0, 1, 2):
        for chrom, rs in sets:
            f = by_chrom.get(chrom, [])
            labels = {w: X.labels_of_features(f, SPAN + 2100, w) for w in "+-"} if stranded else X.labels_of_features(f, SPAN + 2100)
            bins[(stranded, chrom)] = X.bins_of([labels["+"], labels["-"]] if stranded else [labels])
            results[(stranded, chrom)] = X.reads_of(rs, labels, stranded)
    return dict(dir=str(d), bam=bam, sam=sam, mixed=mixed, gtf=gtf, sets=sets, by_chrom=by_chrom, bins=bins, results=results)


def _want(f, stranded=0, chroms=NAMES, exclude=0):
    """-> ({chrom: the bins' reads}, the four verdict sums) of the yardstick."""
    per_bin, verdicts = {}, [0, 0, 0, 0]
    for chrom, rs in f["sets"]:
        if chrom in chroms:
            bins = f["bins"][(stranded, chrom)]
            c = X.counts_of(f["results"][(stranded, chrom)], {k: i for i, k in enumerate(bins)}, len(bins), keep=((rs.flag & exclude) == 0).tolist())
            per_bin[chrom], verdicts = c[:len(bins)], [x + y for x, y in zip(verdicts, c[len(bins):])]
    return per_bin, verdicts


def _files(f, stranded=0, chroms=NAMES, exclude=0, only=None):
    per_bin, verdicts = _want(f, stranded, chroms, exclude)
    rows = X.rows_of(IDS, ["c2", "c1"], {c: f["bins"][(stranded, c)] for c in NAMES}, only)
    return X.bins_text(rows), X.counts_text(rows, per_bin, verdicts)


@pytest.mark.parametrize("exclude", [0, 0x110])
@pytest.mark.parametrize("how", ["device", "host", "shares", "sam"])
def test_counts_after_every_decode(ctx, decode_files, how, exclude):
    f = decode_files
    options = proc.DecodeOptions((0, 0, exclude))
    if how == "sam":
        source = proc.open_alignments(f["sam"], options=options)
    else:
        source = native.BamFile(f["bam"], threads=2, defer=True, exclude_flags=exclude)
    features = gc.read_features(f["gtf"])
    try:
        devices = (0,)
        if how == "device":
            assert source.decode_on_device(ctx) is True, source.decline_reason()
        elif how == "host":
            source.start_host_decode()
        elif how == "shares":
            devices = (0, 0)
            source.decode_on_devices_async([0, 0])
            assert source.join_decoders() is True, source.decline_reason()
            assert len(source.shares) == 2
            assert any(sum(1 for k in range(2) if source.share_ref(k, c)[0] > 0) == 2 for c in NAMES)      # (a chromosome is cut)
        want_bins, want = _want(f, exclude=exclude)
        assert min(want) > 0 and sum(want) == sum(int(((rs.flag & exclude) == 0).sum()) for _, rs in f["sets"])
        per_chrom = {}
        got_bins, got = xc.counts_of_source(source, devices, NAMES, xc.Bins(features), 0, per_chrom)
        assert got.tolist() == want and {c: v.tolist() for c, v in got_bins.items()} == want_bins and want_bins["c3"] == []
        assert {c: int(v.sum()) for c, v in per_chrom.items()} == {c: int(((rs.flag & exclude) == 0).sum()) for c, rs in f["sets"]}
        one_bins, one = xc.counts_of_source(source, devices, ["c2"], xc.Bins(features, True), 2)          # (-c, rf)
        want_bins, want_one = _want(f, 2, ["c2"], exclude)
        assert one.tolist() == want_one and {c: v.tolist() for c, v in one_bins.items()} == want_bins
    finally:
        if hasattr(source, "close"):
            source.close()
    if exclude:
        assert want != _want(f)[1]


def _both(prefix):
    return open(prefix + ".exonbins.tsv").read(), open(prefix + ".exoncounts.tsv").read()


def test_command_on_bam_sam_text_a_shuffled_file_one_chromosome_and_stranded(decode_files, capsys):
    f = decode_files
    d = f["dir"]
    n_reads = sum(rs.n for _, rs in f["sets"])
    assert cli.main(["exoncounts", "-B", f["bam"], "-A", f["gtf"], "-o", d + "/plain"]) == 0
    log = capsys.readouterr().out
    want = _files(f)
    verdicts = _want(f)[1]
    assert _both(d + "/plain") == want
    rows = [line.split("\t") for line in want[1].splitlines()]
    assert [r[0] for r in rows[-3:]] == list(X.SPECIALS) and sum(int(r[1]) for r in rows[-3:]) + verdicts[0] == n_reads          # unplaced reads are in no set
    assert [line.split("\t")[0] for line in want[0].splitlines()[1:]] == [r[0] for r in rows[:-3]] and any(r[1] == "0" for r in rows)          # the same order; zeros included
    assert all("  %s: " % c in log for c in NAMES) and "Annotation: " in log and ("Bins: %d exon counting bins" % (len(rows) - 3)) in log
    assert ("%d reads counted, %d without a feature, %d ambiguous, %d not counted" % tuple(verdicts)) in log
    for name, argv in (("sam", ["-B", f["sam"]]), ("host", ["-B", f["bam"], "--hostDecode"]), ("mixed", ["-B", f["mixed"], "--anyOrder"])):
        assert cli.main(["exoncounts", "-A", f["gtf"], "-o", d + "/" + name] + argv) == 0
        assert _both(d + "/" + name) == want, name
    assert "is not in coordinate order: %d reads sorted" % n_reads in capsys.readouterr().out
    # -c: that chromosome's reads, and only the bins on it, under the ids they have in the whole annotation
    assert cli.main(["exoncounts", "-B", f["bam"], "-A", f["gtf"], "-o", d + "/one", "-c", "c1"]) == 0
    one = _files(f, 0, ["c1"], only="c1")
    assert _both(d + "/one") == one and set(one[0].splitlines()[1:]) < set(want[0].splitlines()[1:])
    firsts = {}
    for line in one[0].splitlines()[1:]:
        firsts.setdefault(line.split("\t")[1], line.split("\t")[0])
    assert firsts["gene00"] == "gene00:001" and any(not v.endswith(":001") for v in firsts.values())          # (a gene's bins on c2 rank before its bins on c1)
    # a chromosome without a feature: no bin row, its reads are in the three rows
    assert cli.main(["exoncounts", "-B", f["sam"], "-A", f["gtf"], "-o", d + "/none", "-c", "c3"]) == 0
    none = _files(f, 0, ["c3"], only="c3")
    assert _both(d + "/none") == none and none[0] == "id\tgene\tchrom\tstart\tend\n" and none[1].count("\n") == 3
    # stranded, under a filter
    for s, code in (("fr", 1), ("rf", 2)):
        assert cli.main(["exoncounts", "-B", f["bam"] if code == 1 else f["mixed"], "-A", f["gtf"], "-o", d + "/" + s, "--isStranded", "-s", s, "--excludeFlags", "0x400"] +
                        (["--anyOrder"] if code == 2 else [])) == 0
        assert _both(d + "/" + s) == _files(f, code, exclude=0x400) and _both(d + "/" + s) != want
    assert _both(d + "/fr")[0] == _both(d + "/rf")[0] and _both(d + "/fr")[1] != _both(d + "/rf")[1]          # the same bins, other reads
    # another feature type
    assert cli.main(["exoncounts", "-B", f["bam"], "-A", f["gtf"], "-o", d + "/cds", "-t", "CDS"]) == 0
    bins_text, counts_text = _both(d + "/cds")
    assert all(line.startswith("other:") for line in counts_text.splitlines()[:-3]) and bins_text.count("\n") == counts_text.count("\n") - 2
