"""``genecounts`` on the device: ``spl_gene_count`` on fused sets against the yardstick of ``genecases.py`` -- exactly, the sums being
integers -- at the sizes where the kernel's geometry changes, on a gene that takes every read and on a gene change every lane, on
maps below and beyond the LDS top level, on reads in any order, stranded and not; its refusals; the decodes through
``counts_of_source``; the command line, whose file is compared byte for byte."""
import numpy as np
import pytest

import genecases as G
from spliser_amd import cli, genecounts as gc, native, process as proc, samio

pytestmark = pytest.mark.gpu

# The kernel's geometry (csrc/spl_genecount.h): a workgroup takes SPL_GENE_TILE = 256 reads a grid-stride step, a read a lane, and a
# launch has at most SPL_GENE_GRID_MAX = 1024 workgroups.  EVERY workgroup takes a second step from 524 033 reads on;
# 2 * 1024 * 256 + 1 gives the first one a third.  SPL_GENE_TOP = 1024 entries of a map's top level are in LDS; a map beyond it is
# searched in global memory too.
TILE, GRID_MAX, TOP = 256, 1024, 1024
LARGE = 2 * GRID_MAX * TILE + 1
BYTE = {"+": 43, "-": 45, ".": 46}


@pytest.fixture(scope="module")
def ctx():
    with native.Context(0) as c:
        yield c


def _device(ctx, rs, n_genes, a, b=None, stranded=0, shift=0):
    with ctx.upload_soa([native.ReadArrays(rs.pos, rs.flag, rs.cig_off, rs.cigar)]) as soa:
        with ctx.begin_reads() as dr:
            dr.add_soa(soa, 0, shift)
            dr.finish()
            got = dr.gene_counts(n_genes, a, b, stranded)
            if rs.n:
                assert dr.layout_bytes()[1] == 0          # (the set stays fused)
            assert got.dtype == np.int64 and got.shape == (n_genes + 3,) and int(got.sum()) == rs.n
            return got.tolist()


def _arrays(features):
    return (np.array([f[0] for f in features], np.int64), np.array([f[1] for f in features], np.int64), np.array([BYTE[f[2]] for f in features], np.uint8),
            np.array([f[3] for f in features], np.int64))


def _permuted(rs, perm):
    n_ops = np.diff(rs.cig_off.astype(np.int64))[perm]
    off = np.concatenate(([0], np.cumsum(n_ops)))
    take = np.repeat(rs.cig_off.astype(np.int64)[perm] - off[:-1], n_ops) + np.arange(int(off[-1]))
    return samio.ReadSet(rs.pos[perm], rs.flag[perm], off, rs.cigar[take])


def _short_reads(pos, flag=None, length=2):
    """Reads of one aligned op of ``length`` bases, built as arrays."""
    n = len(pos)
    return samio.ReadSet(np.asarray(pos, np.int32), np.zeros(n, np.uint16) if flag is None else flag, np.arange(n + 1), np.full(n, (length << 4) | 0, np.uint32))


N_GENES, LENGTH = 9, 6000


@pytest.fixture(scope="module")
def content():
    """Random features of every kind on 6000 bases with their three maps, 4000 random reads of every kind, and the yardstick's
    results per read (unstranded, fr, rf), computed once."""
    rng = np.random.default_rng(20261019)
    features = G.random_features(rng, LENGTH - 700, N_GENES, 30)
    rs = samio.ReadSet.from_records(G.random_records(rng, 4000, LENGTH - 700))
    a, _ = gc.gene_maps(*_arrays(features))
    plus, minus = gc.gene_maps(*_arrays(features), stranded=True)
    assert not (np.array_equal(plus[0], minus[0]) and np.array_equal(plus[1], minus[1]))
    bases = G.bases_of_features(features, LENGTH)
    both = {w: G.bases_of_features(features, LENGTH, w) for w in "+-"}
    results = {0: G.results_of(rs, bases), 1: G.results_of(rs, both, 1), 2: G.results_of(rs, both, 2)}
    assert {0, 16, 99, 147, 83, 163, 4, 256, 512, 1024, 2048} == set(rs.flag.tolist()) and int(rs.pos.min()) == 0 and int(np.diff(rs.cig_off.astype(np.int64)).min()) == 0
    return dict(features=features, rs=rs, a=a, plus=plus, minus=minus, bases=bases, both=both, results=results)


# ---- sizes --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, TILE - 1, TILE, TILE + 1])
def test_sizes_around_a_wave_and_a_tile(ctx, content, n):
    rs = content["rs"].take(1000, 1000 + n)
    want = G.counts_of(content["results"][0][1000:1000 + n], N_GENES)
    assert sum(want) == n
    assert _device(ctx, rs, N_GENES, content["a"]) == want


def test_a_gene_that_takes_every_read_of_a_set_that_gives_every_workgroup_more_than_one_step(ctx):
    """The hot gene: LARGE reads of two bases, sorted, all inside the one exon of gene 3 of 5.  The count is exact."""
    rng = np.random.default_rng(7)
    a = (np.array([1000, 900000], np.int32), np.array([4, 0], np.uint32))
    rs = _short_reads(np.sort(rng.integers(1001, 899990, LARGE)))
    results = G.results_of(rs, G.bases_of_map(*a))
    assert results == [3] * LARGE and G.run_heads(results) == (LARGE + 63) // 64          # one add a wave
    assert _device(ctx, rs, 5, a) == [0, 0, 0, LARGE, 0, 0, 0, 0]


def test_a_gene_change_every_lane_at_the_same_size(ctx):
    """Neighbouring reads in two genes that alternate exon by exon, four bases each: every lane is a head, one add a read."""
    n_genes = 7
    start = 1000 + 4 * np.arange(2001)
    code = np.where(np.arange(2001) % 2 == 0, 1, n_genes).astype(np.uint32)
    code[-1] = 0
    a = (start.astype(np.int32), code)
    i = np.arange(LARGE)
    rs = _short_reads(1001 + 4 * (i % 2000))                  # read i lies in stretch i % 2000
    results = G.results_of(rs, G.bases_of_map(*a))
    assert results[:4] == [0, n_genes - 1, 0, n_genes - 1] and G.run_heads(results) == LARGE
    want = G.counts_of(results, n_genes)
    assert want[0] + want[n_genes - 1] == LARGE and abs(want[0] - want[n_genes - 1]) <= 2000
    assert _device(ctx, rs, n_genes, a) == want


def test_runs_that_cross_a_wave_and_a_tile_boundary_and_the_first_and_the_last_gene(ctx):
    """Sorted reads over exons of 1000 genes in turn: runs of 60, 10, 190, 3, 64, 1, 250, ... reads, so that runs end before, on
    and behind lanes 63 / 64 and reads 255 / 256, in gene 0 and in gene n_genes - 1 among others."""
    n_genes = 1000
    lengths = [60, 10, 190, 3, 64, 1, 250, 62, 128, 256, 65, 447, 63, 1, 1, 510]
    genes = [0, n_genes - 1, 5, 0, 17, n_genes - 1, 400, 0, 1, n_genes - 1, 2, 998, 0, 999, 0, 999]
    start = 100 * np.arange(1, len(lengths) + 2)
    a = (start.astype(np.int32), np.array([g + 1 for g in genes] + [0], np.uint32))
    rs = _short_reads(np.concatenate([np.sort(100 * (k + 1) + 1 + (np.arange(n) % 90)) for k, n in enumerate(lengths)]))
    results = G.results_of(rs, G.bases_of_map(*a))
    assert [results.count(g) for g in (0, n_genes - 1)] == [sum(n for n, g in zip(lengths, genes) if g == 0), sum(n for n, g in zip(lengths, genes) if g == n_genes - 1)]
    assert rs.n > 8 * TILE and _device(ctx, rs, n_genes, a) == G.counts_of(results, n_genes)


# ---- maps ---------------------------------------------------------------------------------------------------------------------
def _map_of(rng, n, n_genes):
    """n entries of which a read can still lie in a stretch: clusters of forty entries a base apart, each followed by a stretch
    of a hundred bases or more -- of a large map the top level in LDS finds the cluster, the search in global memory the entry."""
    clusters = (n + 39) // 40
    anchors = 140 * np.arange(1, clusters + 1) + rng.integers(0, 50, clusters)
    start = (anchors[:, None] + np.arange(40)[None, :]).ravel()[:n]
    code = rng.choice(np.array([0] + list(range(1, n_genes + 1)) + [G.MANY], np.uint32), n, p=[0.3] + [0.65 / n_genes] * n_genes + [0.05])
    if n <= 2:
        code = np.array([n_genes, G.MANY], np.uint32)[:n]          # (the last gene from the first entry on; then many to the end)
    assert (np.diff(start) > 0).all()
    return start.astype(np.int32), code


@pytest.mark.parametrize("n_map", [0, 1, 2, TOP - 1, TOP, TOP + 1, 40000])
def test_maps_below_at_and_beyond_the_top_level(ctx, n_map):
    rng = np.random.default_rng(300 + n_map)
    n_genes = 4
    a = _map_of(rng, n_map, n_genes)
    span = int(a[0][-1]) + 300 if n_map else 5000
    rs = samio.ReadSet.from_records(G.random_records(rng, 3000, span))
    results = G.results_of(rs, G.bases_of_map(*a))
    want = G.counts_of(results, n_genes)
    if n_map == 0:
        assert not any(want[:n_genes]) and want[n_genes + 1] == 0 and want[n_genes] > 2000          # every eligible read: no feature
    elif n_map > 2:
        assert min(want) > 0
    assert _device(ctx, rs, n_genes, a) == want
    perm = rng.permutation(rs.n)
    assert _device(ctx, _permuted(rs, perm), n_genes, a) == want


def test_a_map_that_says_many_everywhere(ctx, content):
    rs = content["rs"]
    for a in ((np.array([0], np.int32), np.array([G.MANY], np.uint32)), (np.array([0, 700, 701, 3000], np.int32), np.full(4, G.MANY, np.uint32))):
        want = G.counts_of(G.results_of(rs, G.bases_of_map(*a)), N_GENES)
        assert not any(want[:N_GENES]) and want[N_GENES + 1] > 2000 and want[N_GENES] > 0 and want[N_GENES + 2] > 0
        assert _device(ctx, rs, N_GENES, a) == want


# ---- content ------------------------------------------------------------------------------------------------------------------
def test_reads_of_every_kind_and_in_any_order(ctx, content):
    rs, want = content["rs"], G.counts_of(content["results"][0], N_GENES)
    assert min(want[N_GENES:]) > 0 and sum(1 for c in want[:N_GENES] if c) >= 5
    assert _device(ctx, rs, N_GENES, content["a"]) == want
    prs = _permuted(rs, np.random.default_rng(5).permutation(rs.n))
    assert not np.array_equal(prs.pos, rs.pos)
    assert G.counts_of(G.results_of(prs, content["bases"]), N_GENES) == want
    assert _device(ctx, prs, N_GENES, content["a"]) == want


def test_a_set_moved_into_a_shard_is_counted_where_it_lies(ctx, content):
    """Map coordinates are the set's: a segment added with a shift meets the map moved by as much."""
    rs, a = content["rs"], content["a"]
    shift = 5000000
    want = G.counts_of(content["results"][0], N_GENES)
    assert _device(ctx, rs, N_GENES, (a[0] + shift, a[1]), shift=shift) == want
    assert _device(ctx, rs, N_GENES, a, shift=shift) != want          # (the map left where it was: the reads are elsewhere)


@pytest.mark.parametrize("stranded", [1, 2])
def test_stranded_with_two_different_maps(ctx, content, stranded):
    rs = content["rs"]
    want = G.counts_of(content["results"][stranded], N_GENES)
    assert want != G.counts_of(content["results"][0], N_GENES) and want != G.counts_of(content["results"][3 - stranded], N_GENES)
    assert _device(ctx, rs, N_GENES, content["plus"], content["minus"], stranded) == want
    # rf is fr with the maps exchanged
    assert _device(ctx, rs, N_GENES, content["minus"], content["plus"], 3 - stranded) == want


@pytest.mark.parametrize("stranded", [0, 1, 2])
def test_the_corner_cases_on_the_device(ctx, stranded):
    """The host's corner cases as one set, and each alone: a read's answer does not depend on its neighbours."""
    left, right, strand, gene = G.corner_arrays()
    n_genes = len(G.CORNER_IDS)
    if stranded:
        a, b = gc.gene_maps(left, right, strand, gene, stranded=True)
    else:
        a, b = gc.gene_maps(left, right, strand, gene)
    assert a[0].shape[0] > TOP
    bases = G.corner_bases(stranded)
    recs = [(flag, pos, cigar) for _, flag, pos, cigar, _ in G.CORNERS]
    rs = samio.ReadSet.from_records(recs)
    assert int(np.diff(rs.cig_off.astype(np.int64)).max()) == 2203
    results = G.results_of(rs, bases, stranded)
    if not stranded:
        assert results == [c[4] for c in G.CORNERS]
    assert _device(ctx, rs, n_genes, a, b, stranded) == G.counts_of(results, n_genes)
    for k, rec in enumerate(recs):
        one = samio.ReadSet.from_records([rec])
        assert _device(ctx, one, n_genes, a, b, stranded) == G.counts_of(results[k:k + 1], n_genes), G.CORNERS[k][0]


def test_counts_are_added_to_what_the_caller_holds(ctx, content):
    rs, a = content["rs"], content["a"]
    want = G.counts_of(content["results"][0], N_GENES)
    with ctx.upload_soa([native.ReadArrays(rs.pos, rs.flag, rs.cig_off, rs.cigar)]) as soa:
        with ctx.begin_reads() as dr:
            dr.add_soa(soa, 0)
            dr.finish()
            out = np.arange(N_GENES + 3, dtype=np.int64) * 1000
            assert dr.gene_counts(N_GENES, a, out=out) is out
            dr.gene_counts(N_GENES, a, out=out)
            assert out.tolist() == [1000 * k + 2 * w for k, w in enumerate(want)]


# ---- errors -------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_working(ctx, content):
    rs, a = content["rs"], content["a"]
    want = G.counts_of(content["results"][0], N_GENES)
    arrays = native.ReadArrays(rs.pos, rs.flag, rs.cig_off, rs.cigar)
    dr = ctx.upload_reads(arrays)                  # (packed on the host: records, not arrays)
    try:
        with pytest.raises(native.SpliserNativeError, match="fused") as err:
            dr.gene_counts(N_GENES, a)
        assert err.value.code == -1
    finally:
        dr.free()
    with ctx.upload_soa([arrays]) as soa:
        with ctx.begin_reads() as dr:
            dr.add_soa(soa, 0)
            dr.finish()
            out = np.zeros(N_GENES + 3, np.int64)
            for bad in ((np.array([30, 20, 10], np.int32), np.array([1, 2, 1], np.uint32)), (np.array([10, 20, 20], np.int32), np.array([1, 2, 1], np.uint32))):
                for maps in ((bad, None), (a, bad)):
                    with pytest.raises(native.SpliserNativeError, match="ascending") as err:
                        dr.gene_counts(N_GENES, *maps, out=out)
                    assert err.value.code == -1
            for code in (N_GENES + 1, 0xFFFFFFFE, 2 ** 31):
                with pytest.raises(native.SpliserNativeError, match="code") as err:
                    dr.gene_counts(N_GENES, (np.array([10, 20], np.int32), np.array([1, code], np.uint32)), out=out)
                assert err.value.code == -1
            for stranded in (-1, 3):
                with pytest.raises(native.SpliserNativeError, match="stranded") as err:
                    dr.gene_counts(N_GENES, a, None, stranded, out=out)
                assert err.value.code == -1
            i64, none = native.ctypes.c_int64, None
            for args in ((ctx._h, dr._h, 0, i64(0), none, none, i64(0), none, none, i64(N_GENES), none),                      # no counts
                         (ctx._h, dr._h, 0, i64(2), none, none, i64(0), none, none, i64(N_GENES), native._ptr(out)),          # a map of two entries that is not there
                         (ctx._h, none, 0, i64(0), none, none, i64(0), none, none, i64(N_GENES), native._ptr(out))):          # no read set
                with pytest.raises(native.SpliserNativeError, match="null") as err:
                    native._check(native.lib().spl_gene_count(*args))
                assert err.value.code == -1
            assert not out.any()                                   # (a refusal adds nothing)
            assert dr.gene_counts(N_GENES, (np.array([10, 20], np.int32), np.array([N_GENES, G.MANY], np.uint32))).sum() == rs.n      # the greatest code there is
            assert dr.gene_counts(N_GENES, a).tolist() == want
    assert _device(ctx, rs, N_GENES, a) == want


# ---- the decodes --------------------------------------------------------------------------------------------------------------
NAMES, LENGTHS = ["c1", "c2", "c3"], [10 ** 6] * 3
IDS = ["gene%02d" % k for k in range(12)]
SPAN = 20000


def _gtf_text(features_by_chrom):
    text = "##gtf of the tests\n"
    for chrom in NAMES:
        for k, (left, right, strand, gene) in enumerate(features_by_chrom.get(chrom, [])):
            attrs = ('gene_id "%s"; transcript_id "t%d";' % (IDS[gene], k)) if k % 2 else ("ID=e%d;gene_id=%s" % (k, IDS[gene]))
            text += "%s\tsynth\texon\t%d\t%d\t.\t%s\t.\t%s\n" % (chrom, left + 1, right, strand, attrs)
            if k % 5 == 0:
                text += "%s\tsynth\tCDS\t%d\t%d\t.\t%s\t0\tgene_id \"other\";\n" % (chrom, left + 1, right, strand)
    return text


@pytest.fixture(scope="module")
def decode_files(tmp_path_factory):
    """Three chromosomes of 3000 reads (more than eight BGZF blocks: a file of fewer is not cut into shares); genes 0..7 on c1, 4..11 on c2 (four genes lie on both), none on c3.  The yardstick's
    results per read for unstranded, fr and rf, computed once."""
    d = tmp_path_factory.mktemp("gdec")
    rng = np.random.default_rng(31)
    sets, features = [], {}
    for k, chrom in enumerate(NAMES):
        recs = [r for r in G.random_records(rng, 3200, SPAN) if r[1] >= 1 and r[2]][:3000]
        sets.append((chrom, samio.ReadSet.from_records(recs)))
        if k < 2:
            features[chrom] = [(l, r, s, g + 4 * k) for l, r, s, g in G.random_features(rng, SPAN, 8, 40)]
    bam, sam, gtf = str(d / "d.bam"), str(d / "d.sam"), str(d / "genes.gtf")
    samio.write_bam(bam, NAMES, LENGTHS, sets, with_seq=True, unplaced=3)
    with open(sam, "w") as fh:
        fh.write("@HD\tVN:1.6\tSO:coordinate\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % (n, ln) for n, ln in zip(NAMES, LENGTHS)))
        for chrom, rs in sets:
            for k in range(rs.n):
                fh.write("\t".join(["r", str(rs.flag[k]), chrom, str(rs.pos[k]), "60", samio.cigar_string(rs.cigar[rs.cig_off[k]:rs.cig_off[k + 1]]), "*", "0", "0", "*", "*"]) + "\n")
    text = _gtf_text(features)
    open(gtf, "w").write(text)
    ids, by_chrom = G.features_of_text(text)
    assert ids == IDS and set(by_chrom) == {"c1", "c2"}
    results = {}
    for stranded in (0, 1, 2):
        for chrom, rs in sets:
            f = by_chrom.get(chrom, [])
            bases = {w: G.bases_of_features(f, SPAN + 2100, w) for w in "+-"} if stranded else G.bases_of_features(f, SPAN + 2100)
            results[(stranded, chrom)] = G.results_of(rs, bases, stranded)
    return dict(dir=str(d), bam=bam, sam=sam, gtf=gtf, sets=sets, by_chrom=by_chrom, results=results)


def _want(f, stranded=0, chroms=NAMES, exclude=0):
    out = [0] * (len(IDS) + 3)
    for chrom, rs in f["sets"]:
        if chrom in chroms:
            out = [a + b for a, b in zip(out, G.counts_of(f["results"][(stranded, chrom)], len(IDS), keep=((rs.flag & exclude) == 0).tolist()))]
    return out


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
        want = _want(f, exclude=exclude)
        assert min(want[len(IDS):]) > 0 and sum(want) == sum(int(((rs.flag & exclude) == 0).sum()) for _, rs in f["sets"])
        per_chrom = {}
        got = gc.counts_of_source(source, devices, NAMES, gc.maps_of(features, NAMES), len(IDS), 0, per_chrom)
        assert got.tolist() == want
        assert {c: int(v.sum()) for c, v in per_chrom.items()} == {c: int(((rs.flag & exclude) == 0).sum()) for c, rs in f["sets"]}
        one = gc.counts_of_source(source, devices, ["c2"], gc.maps_of(features, ["c2"], True), len(IDS), 2)          # (-c, rf)
        assert one.tolist() == _want(f, 2, ["c2"], exclude)
    finally:
        if hasattr(source, "close"):
            source.close()
    if exclude:
        assert want != _want(f)


# ---- the command --------------------------------------------------------------------------------------------------------------
def test_command_on_bam_and_sam_text_one_chromosome_and_stranded(decode_files, capsys):
    f = decode_files
    d = f["dir"]
    n_reads = sum(rs.n for _, rs in f["sets"])
    assert cli.main(["genecounts", "-B", f["bam"], "-A", f["gtf"], "-o", d + "/plain"]) == 0
    log = capsys.readouterr().out
    want = _want(f)
    text = open(d + "/plain.genecounts.tsv").read()
    assert text == G.file_text(IDS, want)
    rows = [line.split("\t") for line in text.splitlines()]
    assert [r[0] for r in rows] == IDS + list(G.SPECIALS) and sum(int(r[1]) for r in rows) == n_reads          # zeros included; unplaced reads are in no set
    assert all("  %s: " % c in log for c in NAMES) and "reads counted" in log and ("%d ambiguous" % want[len(IDS) + 1]) in log
    assert cli.main(["genecounts", "-B", f["sam"], "-A", f["gtf"], "-o", d + "/sam"]) == 0
    assert open(d + "/sam.genecounts.tsv").read() == text
    assert cli.main(["genecounts", "-B", f["bam"], "-A", f["gtf"], "-o", d + "/host", "--hostDecode"]) == 0
    assert open(d + "/host.genecounts.tsv").read() == text
    # -c: that chromosome's reads, and only the genes with a feature on it
    assert cli.main(["genecounts", "-B", f["bam"], "-A", f["gtf"], "-o", d + "/one", "-c", "c2"]) == 0
    on_c2 = {g for _, _, _, g in f["by_chrom"]["c2"]}
    assert on_c2 == set(range(4, 12))
    one = open(d + "/one.genecounts.tsv").read()
    assert one == G.file_text(IDS, _want(f, 0, ["c2"]), only=on_c2) and one.count("\n") == 8 + 3
    assert sum(int(line.split("\t")[1]) for line in one.splitlines()) == f["sets"][1][1].n
    # a chromosome without a feature: every gene row is left out, its reads are in the three rows
    assert cli.main(["genecounts", "-B", f["sam"], "-A", f["gtf"], "-o", d + "/none", "-c", "c3"]) == 0
    none = _want(f, 0, ["c3"])
    assert open(d + "/none.genecounts.tsv").read() == G.file_text(IDS, none, only=set()) and not any(none[:len(IDS)]) and none[len(IDS)] > 1000
    # stranded, under a filter
    for s, code in (("fr", 1), ("rf", 2)):
        assert cli.main(["genecounts", "-B", f["bam"] if code == 1 else f["sam"], "-A", f["gtf"], "-o", d + "/" + s, "--isStranded", "-s", s, "--excludeFlags", "0x400"]) == 0
        got = open("%s/%s.genecounts.tsv" % (d, s)).read()
        assert got == G.file_text(IDS, _want(f, code, exclude=0x400)) and got != text
    assert open(d + "/fr.genecounts.tsv").read() != open(d + "/rf.genecounts.tsv").read()
    # another feature type and attribute
    assert cli.main(["genecounts", "-B", f["bam"], "-A", f["gtf"], "-o", d + "/cds", "-t", "CDS"]) == 0
    cds = [line.split("\t") for line in open(d + "/cds.genecounts.tsv").read().splitlines()]
    assert [r[0] for r in cds] == ["other"] + list(G.SPECIALS) and sum(int(r[1]) for r in cds) == n_reads and int(cds[0][1]) > 0
