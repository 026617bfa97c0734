"""``exoncounts --countReadPairs`` on the device: ``exon_counts(fragments=True)`` (``spl_exon_count_fragments`` on the mate table of
``spl_mate_table``) against the yardstick of ``exonfragcases.py`` -- exactly, the sums being integers -- on generated paired sets
whose coverage is asserted, unstranded, fr, rf and moved by a shift; at the sizes where the kernel's geometry changes; on hand cases
whose answers can be read off the rule, with leader and mate in one wave, in different waves and in different workgroups; on reads in
any order and on a segment that does not begin the arrays; on maps below and beyond the LDS top level; its refusals; its agreement
with ``spl_gene_count_fragments``; and through every decode, where one paired file goes in as BAM on the device, BAM on the host
threads, SAM text, BGZF SAM text and the BAM shuffled, and the command writes one and the same pair of files."""
import re

import numpy as np
import pytest

import exoncases as X
import exonfragcases as F
import genecases as G
import matecases as M
import samzcases as Z
from spliser_amd import cli, exoncounts as xc, genecounts as gc, native, samio

pytestmark = pytest.mark.gpu


def _constant(name):
    """A geometry constant of csrc/spl_exoncount.h, read from the header."""
    import os
    text = open(os.path.join(os.path.dirname(os.path.abspath(native.__file__)), "csrc", "spl_exoncount.h")).read()
    return int(re.search(r"#define %s (\d+)" % name, text).group(1))


TILE, GRID_MAX, TOP = _constant("SPL_EXON_TILE"), _constant("SPL_EXON_GRID_MAX"), _constant("SPL_EXON_TOP")
LARGE = 2 * GRID_MAX * TILE + 1          # every workgroup gets a second step, the first one a third
BYTE = {"+": 43, "-": 45, ".": 46}
N_GENES, LENGTH = 9, 6000


@pytest.fixture(scope="module")
def ctx():
    with native.Context(0) as c:
        yield c


def _arrays(features):
    return (np.array([f[0] for f in features], np.int64), np.array([f[1] for f in features], np.int64), np.array([BYTE[f[2]] for f in features], np.uint8),
            np.array([f[3] for f in features], np.int64))


def _labels(features, length, stranded):
    return {w: X.labels_of_features(features, length, w) for w in "+-"} if stranded else X.labels_of_features(features, length)


def _maps_of(features, stranded):
    a, b, (bin_gene, bin_start, bin_end) = xc.exon_maps(*_arrays(features), stranded=bool(stranded))
    return a, b, bin_gene.astype(np.uint32), list(zip(bin_start.tolist(), bin_end.tolist(), bin_gene.tolist()))


def _device(ctx, rs, keys, bin_gene, a, b=None, stranded=0, shift=0, fragments=True):
    n_bins = len(bin_gene)
    with ctx.upload_soa([native.ReadArrays(rs.pos, rs.flag, rs.cig_off, rs.cigar, name_key=np.asarray(keys, np.uint64))], with_keys=True) as soa:
        with ctx.begin_reads() as dr:
            dr.add_soa(soa, 0, shift)
            dr.finish()
            got = dr.exon_counts(bin_gene, a, b, stranded, fragments=fragments)
            pairs = dr.mate_table(0)[1]["paired"] // 2
            assert got.dtype == np.int64 and got.shape == (n_bins + 4,) and int(got[n_bins:].sum()) == rs.n - (pairs if fragments else 0)          # the verdicts sum to reads - pairs
            if rs.n:
                assert dr.layout_bytes()[1] == 0          # (the set stays fused)
            return got.tolist()


def _permuted(rs, keys, perm):
    n_ops = np.diff(rs.cig_off.astype(np.int64))[perm]
    off = np.concatenate(([0], np.cumsum(n_ops)))
    take = np.repeat(rs.cig_off.astype(np.int64)[perm] - off[:-1], n_ops) + np.arange(int(off[-1]))
    return samio.ReadSet(rs.pos[perm], rs.flag[perm], off, rs.cigar[take]), np.asarray(keys, np.uint64)[perm]


def _want(rs, keys, labels, bins, stranded=0):
    """The yardstick's n_bins + 4 numbers for one segment."""
    return F.counts_of(F.fragment_results(rs, keys, labels, stranded), {key: k for k, key in enumerate(bins)}, len(bins))


@pytest.fixture(scope="module")
def content():
    """A generated paired set of every kind -- ``matecases``' coverage asserted -- on random features and three genes of seven exons,
    their bin maps, and the yardstick's counts (unstranded, fr, rf), computed once."""
    rng = np.random.default_rng(20261021)
    features = G.random_features(rng, 2200, N_GENES, 16) + [(2400 + 770 * g + 110 * j, 2480 + 770 * g + 110 * j, "+-."[g], g) for g in range(3) for j in range(7)]
    records, names, kinds = M.paired_records(rng, 1500, LENGTH - 1200)
    rs = samio.ReadSet.from_records(records)
    keys = np.array([M.name_key(n) for n in names], np.uint64)
    M.assert_covers(kinds, rs.flag, rs.pos, np.diff(rs.cig_off.astype(np.int64)), keys)
    assert rs.n > 8 * TILE
    out = dict(rs=rs, keys=keys, features=features)
    for stranded in (0, 1, 2):
        labels = _labels(features, LENGTH, stranded)
        a, b, bin_gene, bins = _maps_of(features, stranded)
        assert bins == X.bins_of([labels["+"], labels["-"]] if stranded else [labels])
        out[stranded] = dict(labels=labels, a=a, b=b, bin_gene=bin_gene, bins=bins, want=_want(rs, keys, labels, bins, stranded))
    return out


# ---- generated sets -----------------------------------------------------------------------------------------------------------
def test_generated_pairs_unstranded_and_per_read_as_before(ctx, content):
    rs, keys, c = content["rs"], content["keys"], content[0]
    n = len(c["bins"])
    assert min(c["want"][n:]) > 0 and sum(1 for v in c["want"][:n] if v) >= 10
    assert _device(ctx, rs, keys, c["bin_gene"], c["a"]) == c["want"]
    # without the switch: the per-read yardstick, on the very same set -- a bin both mates overlap takes two there
    per_read = X.counts_of(X.reads_of(rs, c["labels"]), {key: k for k, key in enumerate(c["bins"])}, n)
    assert sum(per_read[n:]) == rs.n and sum(per_read[:n]) > sum(c["want"][:n])
    assert _device(ctx, rs, keys, c["bin_gene"], c["a"], fragments=False) == per_read
    with ctx.upload_soa([native.ReadArrays(rs.pos, rs.flag, rs.cig_off, rs.cigar)]) as soa:          # ... and on a set without keys, as before
        with ctx.begin_reads() as dr:
            dr.add_soa(soa, 0)
            dr.finish()
            assert dr.exon_counts(c["bin_gene"], c["a"]).tolist() == per_read


@pytest.mark.parametrize("stranded", [1, 2])
def test_generated_pairs_stranded_with_two_maps_that_share_bins(ctx, content, stranded):
    c = content[stranded]
    assert c["want"] != content[3 - stranded]["want"]
    assert _device(ctx, content["rs"], content["keys"], c["bin_gene"], c["a"], c["b"], stranded) == c["want"]
    assert _device(ctx, content["rs"], content["keys"], c["bin_gene"], c["b"], c["a"], 3 - stranded) == c["want"]          # rf is fr with the maps exchanged


def test_a_set_moved_by_a_shift(ctx, content):
    c, shift = content[0], 5000000
    assert _device(ctx, content["rs"], content["keys"], c["bin_gene"], (c["a"][0] + shift, c["a"][1]), shift=shift) == c["want"]
    assert _device(ctx, content["rs"], content["keys"], c["bin_gene"], c["a"], shift=shift) != c["want"]


@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, TILE - 1, TILE, TILE + 1])
def test_sizes_around_a_wave_and_a_tile(ctx, content, n):
    """A slice of the content: mates fall off its ends and their reads count alone."""
    c = content[0]
    rs, keys = content["rs"].take(1000, 1000 + n), content["keys"][1000:1000 + n]
    assert _device(ctx, rs, keys, c["bin_gene"], c["a"]) == _want(rs, keys, c["labels"], c["bins"])


def test_a_permuted_set_gives_the_same_counts(ctx, content):
    """Leaders lie right of their mates as often as left: the table is in the segment's order, the bins ascend whatever it is.  (Of
    the content, the reads whose names name one first and one second read at most: who pairs with whom in a larger group is a matter
    of the order.)"""
    rs, keys = content["rs"], content["keys"]
    n_ops = np.diff(rs.cig_off.astype(np.int64))
    groups = {}
    for i in range(rs.n):
        if M.pairable(int(rs.flag[i]), int(rs.pos[i]), int(n_ops[i]), int(keys[i])):
            groups.setdefault((int(keys[i]) >> 1, int(rs.flag[i]) & 0x80), []).append(i)
    drop = {i for members in groups.values() if len(members) > 1 for i in members}
    keep = np.array([i for i in range(rs.n) if i not in drop])
    assert 0 < len(drop) < rs.n // 4
    srs, skeys = _permuted(rs, keys, keep)
    prs, pkeys = _permuted(srs, skeys, np.random.default_rng(5).permutation(srs.n))
    mate = M.mate_table_of(prs, pkeys)[0]
    assert sum(1 for i, m in enumerate(mate) if m != M.NONE and m > i and prs.pos[m] < prs.pos[i]) > 100          # leaders whose mate lies to their left
    for stranded in (0, 1):
        c = content[stranded]
        want = _want(srs, skeys, c["labels"], c["bins"], stranded)
        assert _want(prs, pkeys, c["labels"], c["bins"], stranded) == want and min(want[len(c["bins"]):]) > 0
        assert _device(ctx, srs, skeys, c["bin_gene"], c["a"], c["b"], stranded) == want
        assert _device(ctx, prs, pkeys, c["bin_gene"], c["a"], c["b"], stranded) == want


def test_a_segment_that_does_not_begin_the_arrays(ctx, content):
    """Two segments of one fused set: the mate table is the segment's own, its indexes relative to the segment's first read; a pair
    cut by the segments' border counts as two."""
    c, rs, keys = content[0], content["rs"], content["keys"]
    cut = 1111
    parts = [(rs.take(0, cut), keys[:cut]), (rs.take(cut, rs.n), keys[cut:])]
    wants = [_want(p, k, c["labels"], c["bins"]) for p, k in parts]
    want = [x + y for x, y in zip(*wants)]
    assert want != c["want"] and sum(want[len(c["bins"]):]) > sum(c["want"][len(c["bins"]):])
    with ctx.upload_soa([native.ReadArrays(p.pos, p.flag, p.cig_off, p.cigar, name_key=k) for p, k in parts], with_keys=True) as soa:
        with ctx.begin_reads() as dr:
            dr.add_soa(soa, 0)
            dr.add_soa(soa, 1)
            dr.finish()
            assert dr.exon_counts(c["bin_gene"], c["a"], fragments=True).tolist() == want
        with ctx.begin_reads() as dr:          # the second segment alone: it begins at read `cut` of the arrays
            dr.add_soa(soa, 1)
            dr.finish()
            assert dr.exon_counts(c["bin_gene"], c["a"], fragments=True).tolist() == wants[1]


# ---- hand cases ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stranded", [0, 1])
@pytest.mark.parametrize("spread", [0, 70, 300])
def test_hand_cases_with_the_mates_adjacent_in_other_waves_and_in_other_workgroups(ctx, spread, stranded):
    labels = _labels(F.HAND_FEATURES, F.HAND_LENGTH, stranded)
    a, b, bin_gene, bins = _maps_of(F.HAND_FEATURES, stranded)
    number_of = {key: k for k, key in enumerate(bins)}
    names = sorted(F.HAND_CASES)
    for group in [names] + [[n] for n in names]:          # all together, and each alone: a fragment's answer does not depend on its neighbours
        records, keys, where = F.hand_set(group, spread)
        rs = samio.ReadSet.from_records(records)
        results = F.fragment_results(rs, keys, labels, stranded)
        answers = [F.HAND_CASES[n][2 + stranded] for n in group]
        assert [results[w] for w in where] == [(v, sorted(k)) for v, k in answers]          # the rule's text, read off by hand
        want = F.counts_of(results, number_of, len(bins))
        by_hand = [0] * (len(bins) + 4)
        for verdict, hit in answers:
            by_hand[len(bins) - verdict] += 1
            for key in hit:
                by_hand[number_of[key]] += 1
        by_hand[len(bins) + 3] = spread * len(group)          # the fillers
        assert want == by_hand
        assert _device(ctx, rs, keys, bin_gene, a, b, stranded) == want, group
    one = F.HAND_CASES["both mates wholly in one bin: + 1, not + 2"]
    rs = samio.ReadSet.from_records(list(one[:2]))
    assert _device(ctx, rs, [8, 8], bin_gene, a, b, stranded)[number_of[F.A]] == 1 and _device(ctx, rs, [8, 8], bin_gene, a, b, stranded, fragments=False)[number_of[F.A]] == 2


@pytest.mark.parametrize("lead_at", [0, 63])
@pytest.mark.parametrize("name", ["a mate over 70 bins, a one-bin leader", "a leader over 70 bins, a one-bin mate"])
def test_over_70_bins_on_either_mate_at_lane_0_and_lane_63(ctx, name, lead_at):
    """More bins than a wave has lanes, through the merge: the wave goes 75 rounds beside one-bin fragments."""
    labels = _labels(F.HAND_FEATURES, F.HAND_LENGTH, 0)
    a, b, bin_gene, bins = _maps_of(F.HAND_FEATURES, 0)
    one = F.HAND_CASES["both mates wholly in one bin: + 1, not + 2"][:2]
    records, keys = [F.FILLER] * (lead_at % 2), [0] * (lead_at % 2)
    for k in range(40):
        records += list(F.HAND_CASES[name][:2] if len(records) == lead_at else one)
        keys += [2 * k + 2] * 2
    rs = samio.ReadSet.from_records(records)
    results = F.fragment_results(rs, keys, labels)
    assert results[lead_at][0] == F.COUNTED and len(results[lead_at][1]) == F.MANY_BINS > 70 and results[lead_at + 1][0] == F.SILENT
    want = F.counts_of(results, {key: k for k, key in enumerate(bins)}, len(bins))
    assert want[0] == 39 and sum(want[:len(bins)]) == 39 + F.MANY_BINS
    assert _device(ctx, rs, keys, bin_gene, a) == want


def test_a_set_that_gives_every_workgroup_a_second_step(ctx):
    """LARGE reads of two bases inside bin 3 of 5, neighbours mates but where the second read was dropped from pairing (every
    1000th: no 0x1): the bin takes every fragment once."""
    rng = np.random.default_rng(7)
    a = (np.array([1000, 3000], np.int32), np.array([4, 0], np.uint32))
    bin_gene = np.arange(5, dtype=np.uint32)
    i = np.arange(LARGE)
    flag = np.where(i % 2 == 0, 99, 147).astype(np.uint16)
    flag[1::1000] = 16
    keys = ((i // 2 + 1).astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15)) & np.uint64(0xFFFFFFFFFFFFFFFE)
    rs = samio.ReadSet(np.sort(rng.integers(1001, 2990, LARGE)), flag, np.arange(LARGE + 1), np.full(LARGE, (2 << 4), np.uint32))
    results = F.fragment_results(rs, keys, X.MapLabels(a[0], a[1], bin_gene))
    want = F.counts_of(results, None, 5)
    pairs = sum(1 for v, _ in results if v == F.SILENT)
    assert pairs > 250000 and want == [0, 0, 0, LARGE - pairs, 0, LARGE - pairs, 0, 0, 0] and LARGE - pairs > pairs + 500
    assert _device(ctx, rs, keys, bin_gene, a) == want


# ---- maps ---------------------------------------------------------------------------------------------------------------------
def _map_of(rng, n):
    """n entries of which a read can still lie in a stretch: clusters of forty entries a base apart, each followed by a stretch of
    a hundred bases or more.  Entry k is nothing, shared, or bin k of gene (k // 90) % 3."""
    clusters = (n + 39) // 40
    anchors = 140 * np.arange(1, clusters + 1) + rng.integers(0, 50, clusters)
    start = (anchors[:, None] + np.arange(40)[None, :]).ravel()[:n]
    kind = rng.choice(3, n, p=[0.3, 0.65, 0.05])
    code = np.where(kind == 0, 0, np.where(kind == 1, np.arange(1, n + 1), G.MANY)).astype(np.uint32)
    if n <= 2:
        code = np.array([n, G.MANY], np.uint32)[:n]          # (the last bin from the first entry on; then shared to the end)
    return (start.astype(np.int32), code), ((np.arange(n) // 90) % 3).astype(np.uint32)


@pytest.mark.parametrize("n_map", [0, 1, TOP - 1, TOP, TOP + 1, 40000])
def test_maps_below_at_and_beyond_the_top_level(ctx, n_map):
    rng = np.random.default_rng(300 + n_map)
    a, bin_gene = _map_of(rng, n_map)
    span = max(int(a[0][-1]) + 300 if n_map else 0, 5000)
    records, names, _ = M.paired_records(rng, 1200, span)
    rs = samio.ReadSet.from_records(records)
    keys = [M.name_key(n) for n in names]
    results = F.fragment_results(rs, keys, X.MapLabels(a[0], a[1], bin_gene))
    want = F.counts_of(results, None, n_map)
    if n_map == 0:
        assert want[0] == want[2] == 0 and want[1] > 500          # every fragment: no feature
    elif n_map > 2:
        assert min(want[n_map:]) > 0 and max(len(r[1]) for r in results) > 20
    assert _device(ctx, rs, keys, bin_gene, a) == want
    if n_map > 2:
        assert _device(ctx, rs, keys, bin_gene, None, a, 1) != want          # fr: some mates see the empty map


# ---- the ABI ------------------------------------------------------------------------------------------------------------------
def test_counts_are_added_to_what_the_caller_holds(ctx, content):
    c, rs = content[0], content["rs"]
    with ctx.upload_soa([native.ReadArrays(rs.pos, rs.flag, rs.cig_off, rs.cigar, name_key=content["keys"])], with_keys=True) as soa:
        with ctx.begin_reads() as dr:
            dr.add_soa(soa, 0)
            dr.finish()
            out = np.arange(len(c["bins"]) + 4, dtype=np.int64) * 1000
            assert dr.exon_counts(c["bin_gene"], c["a"], out=out, fragments=True) is out
            dr.exon_counts(c["bin_gene"], c["a"], out=out, fragments=True)
            assert out.tolist() == [1000 * k + 2 * w for k, w in enumerate(c["want"])]


def test_refusals_leave_the_context_working(ctx, content):
    c, rs, keys = content[0], content["rs"], content["keys"]
    a, bin_gene, n_bins = c["a"], c["bin_gene"], len(c["bins"])
    arrays = native.ReadArrays(rs.pos, rs.flag, rs.cig_off, rs.cigar)
    dr = ctx.upload_reads(arrays)                  # (packed on the host: records, not arrays)
    try:
        with pytest.raises(native.SpliserNativeError, match="fused") as err:
            dr.exon_counts(bin_gene, a, fragments=True)
        assert err.value.code == -1
    finally:
        dr.free()
    with ctx.upload_soa([arrays]) as soa:          # a set without keys
        with ctx.begin_reads() as dr:
            dr.add_soa(soa, 0)
            dr.finish()
            with pytest.raises(native.SpliserNativeError, match="name keys") as err:
                dr.exon_counts(bin_gene, a, fragments=True)
            assert err.value.code == -1
    with ctx.upload_soa([native.ReadArrays(rs.pos, rs.flag, rs.cig_off, rs.cigar, name_key=keys)], with_keys=True) as soa:
        with ctx.begin_reads() as dr:
            with pytest.raises(native.SpliserNativeError, match="not finished") as err:
                dr.exon_counts(bin_gene, a, fragments=True)
            assert err.value.code == -1
            dr.add_soa(soa, 0)
            dr.finish()
            out = np.zeros(n_bins + 4, np.int64)
            for code in (n_bins + 1, 0xFFFFFFFE):
                for maps in (((np.array([10, 20], np.int32), np.array([1, code], np.uint32)), None), (a, (np.array([10, 20], np.int32), np.array([1, code], np.uint32)))):
                    with pytest.raises(native.SpliserNativeError, match="code") as err:
                        dr.exon_counts(bin_gene, *maps, out=out, fragments=True)
                    assert err.value.code == -1
            with pytest.raises(native.SpliserNativeError, match="ascending"):
                dr.exon_counts(bin_gene, (np.array([30, 20], np.int32), np.array([1, 2], np.uint32)), out=out, fragments=True)
            with pytest.raises(native.SpliserNativeError, match="stranded"):
                dr.exon_counts(bin_gene, a, None, 3, out=out, fragments=True)
            i64, none, genes = native.ctypes.c_int64, None, native._ptr(bin_gene)
            for args, match in (((ctx._h, dr._h, 0, i64(0), none, none, i64(0), none, none, i64(n_bins), genes, none), "null"),
                                ((ctx._h, none, 0, i64(0), none, none, i64(0), none, none, i64(n_bins), genes, native._ptr(out)), "null"),
                                ((ctx._h, dr._h, 0, i64(0), none, none, i64(0), none, none, i64(n_bins), none, native._ptr(out)), "null"),
                                ((ctx._h, dr._h, 0, i64(0), none, none, i64(0), none, none, i64(0xFFFFFFF1), genes, native._ptr(out)), "n_bins")):
                with pytest.raises(native.SpliserNativeError, match=match) as err:
                    native._check(native.lib().spl_exon_count_fragments(*args))
                assert err.value.code == -1
            assert not out.any()                                   # (a refusal adds nothing)
            assert dr.exon_counts(bin_gene, a, fragments=True).tolist() == c["want"]
    assert _device(ctx, rs, keys, bin_gene, a) == c["want"]


@pytest.mark.parametrize("stranded", [0, 1, 2])
def test_the_verdicts_are_spl_gene_count_fragments_on_the_gene_maps_of_the_same_features(ctx, content, stranded):
    c, rs = content[stranded], content["rs"]
    ga, gb = gc.gene_maps(*_arrays(content["features"]), stranded=bool(stranded))
    with ctx.upload_soa([native.ReadArrays(rs.pos, rs.flag, rs.cig_off, rs.cigar, name_key=content["keys"])], with_keys=True) as soa:
        with ctx.begin_reads() as dr:
            dr.add_soa(soa, 0)
            dr.finish()
            genes = dr.gene_counts(N_GENES, ga, gb, stranded, fragments=True).tolist()
            exons = dr.exon_counts(c["bin_gene"], c["a"], c["b"], stranded, fragments=True).tolist()
    n = len(c["bins"])
    assert exons[n:] == [sum(genes[:N_GENES])] + genes[N_GENES:] and min(exons[n:]) > 0


# ---- the decodes and the command ------------------------------------------------------------------------------------------------
NAMES, LENGTHS = ["c1", "c2"], [10 ** 6] * 2
IDS = ["gene%02d" % k for k in range(8)]
SPAN = 6000


@pytest.fixture(scope="module")
def paired_files(tmp_path_factory):
    """Two chromosomes of generated paired reads with names and MAPQs, one pair split over the two, one pair whose second mate has
    MAPQ 3; genes on both.  The one content as BAM, the BAM shuffled record by record, SAM text and BGZF SAM text."""
    d = tmp_path_factory.mktemp("xfdec")
    rng = np.random.default_rng(43)
    sets, names, mapq, features = [], [], [], {}
    for k, chrom in enumerate(NAMES):
        records, nm, _ = M.paired_records(rng, 600, SPAN)
        keep = [j for j, r in enumerate(records) if r[1] >= 1]          # (a file has no POS 0 on a reference)
        records, nm = [records[j] for j in keep], [nm[j] for j in keep]
        records += [(99, SPAN + 45, "20M"), ((99, 147)[k], SPAN + 50, "30M"), (147, SPAN + 60, "30M")]          # the MAPQ pair, and between its mates the split pair's mate
        nm += [b"lowq%d" % k, b"split/pair", b"lowq%d" % k]
        sets.append((chrom, samio.ReadSet.from_records(records)))
        names.append(nm)
        q = np.full(len(records), 60, np.int64)
        q[-1] = 3
        mapq.append(q)
        features[chrom] = ([(l, r, s, g) for l, r, s, g in G.random_features(rng, 2500, 8, 14)] + [(3000 + 110 * j, 3080 + 110 * j, "+-."[k], 4 + k) for j in range(12)] +
                           [(SPAN + 40, SPAN + 70, "+", k), (SPAN + 70, SPAN + 100, "+", k)])          # the MAPQ pair's mates overlap in the first bin; the second mate alone reaches the second
    bam, shuffled, sam, samz, gtf = str(d / "p.bam"), str(d / "s.bam"), str(d / "p.sam"), str(d / "p.sam.gz"), str(d / "genes.gtf")
    samio.write_bam(bam, NAMES, LENGTHS, sets, with_seq=True, unplaced=3, names=names, mapq=mapq)
    singles = [(chrom, rs.take(j, j + 1), [nm[j]], q[j:j + 1]) for (chrom, rs), nm, q in zip(sets, names, mapq) for j in range(rs.n)]
    order = rng.permutation(len(singles))
    samio.write_bam(shuffled, NAMES, LENGTHS, [singles[j][:2] for j in order], with_seq=True, names=[singles[j][2] for j in order], mapq=[singles[j][3] for j in order])
    samio.write_sam(sam, NAMES, LENGTHS, sets, names=names, mapq=mapq)
    with open(sam, "rb") as fh, open(samz, "wb") as out:
        out.write(Z.bgzf(fh.read(), block=0xff00))
    text = "##gtf of the tests\n"
    for chrom in NAMES:
        for j, (left, right, strand, gene) in enumerate(features[chrom]):
            text += "%s\tsynth\texon\t%d\t%d\t.\t%s\t.\tgene_id \"%s\"; transcript_id \"t%d\";\n" % (chrom, left + 1, right, strand, IDS[gene], j)
    open(gtf, "w").write(text)
    ids, by_chrom = G.features_of_text(text)
    assert ids == IDS
    keys = [np.array([M.name_key(n) for n in nm], np.uint64) for nm in names]
    return dict(dir=str(d), bam=bam, shuffled=shuffled, sam=sam, samz=samz, gtf=gtf, sets=sets, keys=keys, mapq=mapq, by_chrom=by_chrom)


def _files(f, stranded=0, fragments=True, min_mapq=0):
    """The yardstick's two files over the file's reads that pass ``min_mapq`` (pairing is among the reads the decode keeps), and
    the number of pairs."""
    per_bin, verdicts, bins_by_chrom, pairs = {}, [0, 0, 0, 0], {}, 0
    for (chrom, rs), keys, q in zip(f["sets"], f["keys"], f["mapq"]):
        keep = np.flatnonzero(q >= min_mapq)
        n_ops = np.diff(rs.cig_off.astype(np.int64))
        kept = samio.ReadSet.from_records([(int(rs.flag[j]), int(rs.pos[j]), samio.cigar_string(rs.cigar[rs.cig_off[j]:rs.cig_off[j + 1]]) if n_ops[j] else "") for j in keep])
        labels = _labels(f["by_chrom"].get(chrom, []), SPAN + 2100, stranded)
        bins = X.bins_of([labels["+"], labels["-"]] if stranded else [labels])
        number_of = {key: k for k, key in enumerate(bins)}
        if fragments:
            mate, counts = M.mate_table_of(kept, keys[keep])
            pairs += counts["paired"] // 2
            c = F.counts_of(F.fragment_results(kept, keys[keep], labels, stranded, mate=mate), number_of, len(bins))
        else:
            c = X.counts_of(X.reads_of(kept, labels, stranded), number_of, len(bins))
        bins_by_chrom[chrom], per_bin[chrom], verdicts = bins, c[:len(bins)], [x + y for x, y in zip(verdicts, c[len(bins):])]
    rows = X.rows_of(IDS, NAMES, bins_by_chrom)
    return (X.bins_text(rows), X.counts_text(rows, per_bin, verdicts)), verdicts, pairs


def _both(prefix):
    return open(prefix + ".exonbins.tsv").read(), open(prefix + ".exoncounts.tsv").read()


def test_the_command_writes_the_same_files_for_five_inputs(paired_files, capsys):
    f, d = paired_files, paired_files["dir"]
    want, verdicts, pairs = _files(f)
    n_reads = sum(rs.n for _, rs in f["sets"])
    assert sum(verdicts) == n_reads - pairs and pairs > 600 and min(verdicts) > 0
    runs = [("bam", ["-B", f["bam"]]), ("host", ["-B", f["bam"], "--hostDecode"]), ("sam", ["-B", f["sam"]]), ("samz", ["-B", f["samz"]]), ("shuffled", ["-B", f["shuffled"], "--anyOrder"])]
    logs = {}
    for tag, args in runs:
        assert cli.main(["exoncounts", "-A", f["gtf"], "-o", d + "/" + tag, "--countReadPairs"] + args) == 0
        logs[tag] = capsys.readouterr().out
        assert _both(d + "/" + tag) == want, tag
    assert ("%d pairs" % pairs) in logs["bam"] and "  mates: " in logs["bam"] and all("  %s: " % c in logs["bam"] for c in NAMES)
    assert ("%d fragments counted, %d without a feature, %d ambiguous, %d not counted" % tuple(verdicts)) in logs["bam"] and "reads counted" not in logs["bam"]
    # stranded
    for s, code in (("fr", 1), ("rf", 2)):
        assert cli.main(["exoncounts", "-B", f["bam"] if code == 1 else f["sam"], "-A", f["gtf"], "-o", d + "/" + s, "--isStranded", "-s", s, "--countReadPairs"]) == 0
        assert _both(d + "/" + s) == _files(f, code)[0]
    assert _both(d + "/fr")[1] != _both(d + "/rf")[1]
    # several devices asked for: decoded and counted on the first, and said
    assert cli.main(["exoncounts", "-B", f["bam"], "-A", f["gtf"], "-o", d + "/two", "--countReadPairs", "--devices", "0,0"]) == 0
    assert "--countReadPairs: the alignment file is decoded and counted on device 0 alone" in capsys.readouterr().out and _both(d + "/two") == want


def test_min_mapq_turns_a_pair_into_a_singleton(paired_files, capsys):
    f, d = paired_files, paired_files["dir"]
    want, verdicts, pairs = _files(f, min_mapq=10)
    all_want, all_verdicts, all_pairs = _files(f)
    assert pairs == all_pairs - 2 and sum(verdicts) == sum(all_verdicts) and want[0] == all_want[0] and want[1] != all_want[1]          # two reads fewer, two pairs fewer
    for tag, args in (("q_bam", ["-B", f["bam"]]), ("q_sam", ["-B", f["sam"]])):
        assert cli.main(["exoncounts", "-A", f["gtf"], "-o", d + "/" + tag, "--countReadPairs", "--minMapQ", "10"] + args) == 0
        assert _both(d + "/" + tag) == want, tag
    capsys.readouterr()


def test_without_the_switch_the_command_writes_what_it_wrote(paired_files, capsys):
    f, d = paired_files, paired_files["dir"]
    want, verdicts, _ = _files(f, fragments=False)
    assert sum(verdicts) == sum(rs.n for _, rs in f["sets"]) and want[1] != _files(f)[0][1]
    for tag, args in (("r_bam", ["-B", f["bam"]]), ("r_sam", ["-B", f["sam"]]), ("r_host", ["-B", f["bam"], "--hostDecode"])):
        assert cli.main(["exoncounts", "-A", f["gtf"], "-o", d + "/" + tag] + args) == 0
        assert _both(d + "/" + tag) == want, tag
    log = capsys.readouterr().out
    assert ("%d reads counted, %d without a feature, %d ambiguous, %d not counted" % tuple(verdicts)) in log and "pairs" not in log and "fragments" not in log
