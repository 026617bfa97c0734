"""GPU parity: the HIP path (through the C ABI) against the oracle and the reference goldens."""
import os

import numpy as np
import pytest

from conftest import golden_cases
import helpers
import limitcases
from spliser_amd import native, samio, shard, sites, synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = native.Context(0)
    yield c
    c.close()


# (ranges_agg: SPL_OPT_WAVE_AGGREGATION selects nothing -- ABI v1 callers that set it must get the default pass and its counters)
KERNELS = {"ranges": 0, "pairs": native.OPT_PAIR_KERNEL, "ranges_agg": native.OPT_WAVE_AGGREGATION}


def gpu_engine(ctx, flags=0):
    def count(arr, reads, stranded, combine_mode):
        s = native.SiteArrays.from_chrom(arr)
        r = native.ReadArrays(reads.pos, reads.flag, reads.cig_off, reads.cigar)
        return ctx.count(s, r, stranded, combine_mode, flags)

    def sse(arr, beta1, b2s_reads, dbl, cryptic):
        return ctx.sse(native.SiteArrays.from_chrom(arr), beta1, b2s_reads, dbl, cryptic)
    return count, sse


@pytest.mark.parametrize("kernel", sorted(KERNELS))
@pytest.mark.parametrize("case,variant,opts", golden_cases(), ids=lambda v: v if isinstance(v, str) else "")
def test_gpu_reproduces_reference_goldens(case, variant, opts, kernel, ctx):
    text, rows = helpers.run_case(case, opts, gpu_engine(ctx, KERNELS[kernel]))
    ref_text, ref_rows = helpers.expected(case, variant)
    assert text == ref_text
    helpers.assert_rows_match(rows, ref_rows, bool(opts.get("cryptic")))


@pytest.mark.parametrize("case", ["cigar_corners", "random_b", "kat1", "random_unstranded_q"])
@pytest.mark.parametrize("stranded", [0, 1, 2])
@pytest.mark.parametrize("combine", [0, 1])
@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_gpu_counters_match_oracle_all_modes(case, stranded, combine, kernel, ctx, oracle_lib):
    table = helpers.build_table(os.path.join(helpers.GOLDEN, case), {"stranded": "fr" if stranded else None})
    _, reads = samio.read_sam(os.path.join(helpers.GOLDEN, case, "reads.sam"))
    ocount, _ = helpers.oracle_engine(oracle_lib)
    gcount, _ = gpu_engine(ctx, KERNELS[kernel])
    for chrom in table.chrom_index:
        arr = table.chrom_arrays(chrom)
        rs = reads.get(chrom, samio.ReadSet.empty())
        for w, g in zip(ocount(arr, rs, stranded, combine), gcount(arr, rs, stranded, combine)):
            assert np.array_equal(w, g)


def _table_for(wl, tmp_path, stranded):
    bed = str(tmp_path / "j.bed")
    synth.write_bed(bed, wl.genome.chrom_names, wl.junctions)
    table = sites.SiteTable(is_stranded=stranded)
    table.add_bed(bed)
    table.find_competitors()
    return table


@pytest.mark.parametrize("kernel", sorted(KERNELS))
@pytest.mark.parametrize("stranded,cryptic", [(0, False), (1, True), (2, True)])
def test_gpu_matches_oracle_on_synthetic_genome(stranded, cryptic, kernel, ctx, oracle_lib, tmp_path):
    """~400k reads over 5 chromosomes, packed into one shard (one launch) vs per-chromosome oracle."""
    wl = synth.Workload("arabidopsis", scale=0.02, seed=21 + stranded)
    table = _table_for(wl, tmp_path, bool(stranded))
    names = wl.genome.chrom_names
    items = [(c, table.chrom_arrays(c), wl.reads[i]) for i, c in enumerate(names) if table.chrom_arrays(c).n]
    shards = shard.pack(items)
    assert len(shards) == 1
    sh = shards[0]
    ds, dr = ctx.upload_sites(sh.sites), ctx.upload_reads(sh.reads)
    ctx.count_launch(ds, dr, stranded, 0, KERNELS[kernel])
    ctx.sse_launch(ds, cryptic)
    beta1, b2s_reads, dbl = ds.counters()
    b2s, b2c, b2w, sse = ds.sse_results()
    dr.free()
    ds.free()
    total = 0
    for (chrom, arr, reads), (r0, r1), (e0, e1) in zip(items, sh.site_rows, sh.edge_rows):
        w1, w2, w3 = oracle_lib.check_bam(arr.pos, arr.strand, arr.part_off, arr.part_pos, arr.comp_off, arr.comp_pos,
                                          reads.pos, reads.flag, reads.cig_off, reads.cigar, stranded, 0)
        assert np.array_equal(beta1[r0:r1], w1) and np.array_equal(b2s_reads[r0:r1], w2) and np.array_equal(dbl[e0:e1], w3)
        ws = oracle_lib.beta2_sse(arr.pos, arr.part_off, arr.part_pos, arr.part_site, arr.alpha, arr.edge_cnt, w1, w2, w3, cryptic)
        for g, w in zip((b2s[r0:r1], b2c[r0:r1], b2w[r0:r1], sse[r0:r1]), ws):
            assert np.array_equal(g, w)
        assert np.all(np.abs(sse[r0:r1] - ws[3]) <= 1e-9)
        total += int(w1.sum()) + int(w2.sum())
    assert total > 10000


def test_gpu_reads_with_non_consuming_ops(ctx, oracle_lib):
    """Soft clips, hard clips, insertions and padding change nothing for checkBam; the pack kernel drops them from short
    CIGARs (so that "5S95M100N50M" takes the once-spliced path).  Random decorations of spliced and unspliced reads on a
    table with rivals, against the oracle, all kernels, all strand modes."""
    arr, rs = limitcases.non_consuming_ops_case()
    deco = native.ReadArrays(rs.pos, rs.flag, rs.cig_off, rs.cigar)
    sites_c = native.SiteArrays.from_chrom(arr)
    for stranded in (0, 1, 2):
        want = oracle_lib.check_bam(arr.pos, arr.strand, arr.part_off, arr.part_pos, arr.comp_off, arr.comp_pos, deco.pos, deco.flag,
                                    deco.cig_off, deco.cigar, stranded, 0)
        for flags in KERNELS.values():
            got = ctx.count(sites_c, deco, stranded, 0, flags)
            for g, w in zip(got, want):
                assert np.array_equal(g, w)
    assert int(want[0].sum()) > 1000 and int(want[1].sum()) > 100


def test_gpu_twice_spliced_class_limits(ctx, oracle_lib):
    """The twice-spliced class packs five lengths into three words (aligned < 4096, introns < 2^28): reads on and just beyond
    those limits, with =/X blocks, soft clips, a deletion instead of an intron, in every neighbourhood (alone, in waves of
    other classes), all modes, against the oracle."""
    sites_c, reads_c = limitcases.twice_spliced_limits_case()
    pos, strand, part_off, part_pos, comp_off, comp_pos = (sites_c.pos, sites_c.strand, sites_c.part_off, sites_c.part_pos,
                                                           sites_c.comp_off, sites_c.comp_pos)
    seen = np.zeros(3, np.int64)
    for stranded in (0, 1, 2):
        for combine in (0, 1):
            want = oracle_lib.check_bam(pos, strand, part_off, part_pos, comp_off, comp_pos, reads_c.pos, reads_c.flag, reads_c.cig_off,
                                        reads_c.cigar, stranded, combine)
            for name, flags in KERNELS.items():
                got = ctx.count(sites_c, reads_c, stranded, combine, flags)
                for g, w in zip(got, want):
                    assert np.array_equal(g, w), (stranded, combine, name)
            seen += [int(w.sum()) for w in want]
    assert seen[0] > 1000 and seen[1] > 1000 and seen[2] > 0   # beta1, beta2Simple and double counts all exercised


def test_gpu_back_to_back_passes_on_one_table(ctx, tmp_path, oracle_lib):
    """The counter region of a device table exists twice and is cleared on the side by the previous pass (or by a clearing
    launch after a pair-kernel pass): a sequence of passes with changing modes and kernels on ONE uploaded table and read set
    must give the oracle's counters every time, and the device error word must not leak from one pass to the next."""
    wl = synth.Workload("arabidopsis", scale=0.003, seed=41)
    table = _table_for(wl, tmp_path, True)
    name = wl.genome.chrom_names[1]
    arr, reads = table.chrom_arrays(name), wl.reads[1]
    sites_c = native.SiteArrays.from_chrom(arr)
    reads_c = native.ReadArrays(reads.pos, reads.flag, reads.cig_off, reads.cigar)
    ds, dr = ctx.upload_sites(sites_c), ctx.upload_reads(reads_c)
    want = {}
    for stranded in (0, 1, 2):
        for combine in (0, 1):
            want[(stranded, combine)] = oracle_lib.check_bam(arr.pos, arr.strand, arr.part_off, arr.part_pos, arr.comp_off, arr.comp_pos,
                                                             reads.pos, reads.flag, reads.cig_off, reads.cigar, stranded, combine)
    sequence = [(0, 0, "ranges"), (1, 0, "ranges"), (1, 0, "pairs"), (0, 0, "ranges"), (2, 1, "ranges"), (2, 1, "ranges"),
                (0, 1, "pairs"), (0, 1, "pairs"), (1, 1, "ranges"), (0, 0, "ranges"), (0, 0, "ranges")]
    for stranded, combine, kernel in sequence:
        ctx.count_launch(ds, dr, stranded, combine, KERNELS[kernel])
        for g, w in zip(ds.counters(), want[(stranded, combine)]):
            assert np.array_equal(g, w), (stranded, combine, kernel)
    # a pass that trips the range check, then a clean one on the same table
    far = ctx.upload_reads(native.ReadArrays([2147483000], [0], [0, 1], [(1 << 20) << 4]))
    ctx.count_launch(ds, far, 0, 0)
    with pytest.raises(native.SpliserNativeError):
        ds.counters()
    far.free()
    ctx.count_launch(ds, dr, 0, 0)
    for g, w in zip(ds.counters(), want[(0, 0)]):
        assert np.array_equal(g, w)
    dr.free()
    ds.free()


@pytest.mark.parametrize("tail_stream", ["1", "0"])
def test_gpu_tail_stream_pipelined_passes(tmp_path, oracle_lib, monkeypatch, tail_stream):
    """The literal kernel and the scan of a pass run on a stream of their own while the next pass's range kernel is under way
    (three counter copies per table, two queue buffers per read set; SPL_TAIL_STREAM=0: everything on one stream).  Passes
    launched back to back without a download in between, on two tables and read sets taking turns, with changing modes and
    kernels: whatever is downloaded, whenever, must be the oracle's result for the last pass on that table."""
    monkeypatch.setenv("SPL_TAIL_STREAM", tail_stream)
    wl = synth.Workload("arabidopsis", scale=0.004, seed=43)
    table = _table_for(wl, tmp_path, True)
    with native.Context(0) as piped:
        dev, want = [], []
        for k in (0, 1):
            name = wl.genome.chrom_names[k]
            arr, reads = table.chrom_arrays(name), wl.reads[k]
            dev.append((piped.upload_sites(native.SiteArrays.from_chrom(arr)),
                        piped.upload_reads(native.ReadArrays(reads.pos, reads.flag, reads.cig_off, reads.cigar))))
            want.append({(st, cb): (oracle_lib.check_bam(arr.pos, arr.strand, arr.part_off, arr.part_pos, arr.comp_off, arr.comp_pos,
                                                         reads.pos, reads.flag, reads.cig_off, reads.cigar, st, cb), arr)
                         for st in (0, 1, 2) for cb in (0, 1)})
        def check(k, st, cb, cryptic):
            ds = dev[k][0]
            cnt, arr = want[k][(st, cb)]
            for g, w in zip(ds.counters(), cnt):
                assert np.array_equal(g, w), (k, st, cb)
            piped.sse_launch(ds, cryptic)
            w_sse = oracle_lib.beta2_sse(arr.pos, arr.part_off, arr.part_pos, arr.part_site, arr.alpha, arr.edge_cnt,
                                         cnt[0], cnt[1], cnt[2], cryptic)
            for g, w in zip(ds.sse_results(), w_sse):
                assert np.array_equal(np.asarray(g), np.asarray(w)), (k, st, cb, "sse")
        # bursts of passes, nothing read back until the end of a burst
        for burst, (st, cb) in enumerate([(0, 0), (1, 0), (2, 1), (0, 1)]):
            for rep in range(7):
                for k in (0, 1):
                    piped.count_launch(dev[k][0], dev[k][1], st, cb, 0)
            check(1, st, cb, burst % 2 == 1)
            check(0, st, cb, burst % 2 == 0)
        # the other kernels in between (they run on the main stream alone), the tables and read sets crossed over
        piped.count_launch(dev[0][0], dev[0][1], 1, 0, KERNELS["pairs"])
        piped.count_launch(dev[1][0], dev[1][1], 1, 0, 0)
        piped.count_launch(dev[0][0], dev[0][1], 2, 0, 0)
        piped.count_launch(dev[1][0], dev[1][1], 2, 0, 0)
        check(0, 2, 0, False)
        check(1, 2, 0, True)
        for rep in range(5):
            piped.count_launch(dev[0][0], dev[0][1], 0, 0, 0)
        check(0, 0, 0, False)
        assert dev[0][1].literal_queue_size() >= 0
        # one table, two read sets taking turns (what `combine` does with a sample's gap-fill queries): the counter copies
        # cycle with the table, the queue buffers with the read set
        arr0, r1 = table.chrom_arrays(wl.genome.chrom_names[0]), wl.reads[1]
        crossed = oracle_lib.check_bam(arr0.pos, arr0.strand, arr0.part_off, arr0.part_pos, arr0.comp_off, arr0.comp_pos,
                                       r1.pos, r1.flag, r1.cig_off, r1.cigar, 1, 0)
        for rep in range(5):
            piped.count_launch(dev[0][0], dev[1][1], 1, 0, 0)
            piped.count_launch(dev[0][0], dev[0][1], 1, 0, 0)
        check(0, 1, 0, True)
        for rep in range(4):
            piped.count_launch(dev[0][0], dev[0][1], 1, 0, 0)
            piped.count_launch(dev[0][0], dev[1][1], 1, 0, 0)
        for g, w in zip(dev[0][0].counters(), crossed):
            assert np.array_equal(g, w), "one table, the other read set"
        for ds, dr in dev:
            dr.free()
            ds.free()


def test_gpu_segment_upload_equals_packed_upload(ctx, tmp_path):
    """spl_reads_upload_segments (per-chromosome arrays shifted on the device) against the host-packed shard."""
    wl = synth.Workload("arabidopsis", scale=0.01, seed=77)
    table = _table_for(wl, tmp_path, False)
    names = wl.genome.chrom_names
    items = [(c, table.chrom_arrays(c), wl.reads[i]) for i, c in enumerate(names) if table.chrom_arrays(c).n]
    items.insert(2, (names[0] + "_empty", table.chrom_arrays(names[0]), None))   # a chromosome without reads
    sh, = shard.pack(items)
    assert len(sh.read_segments) == len(items) - 1
    ds = ctx.upload_sites(sh.sites)
    got = []
    for dr in (ctx.upload_reads(sh.reads), ctx.upload_read_segments(sh.read_segments)):
        assert dr.n == sh.reads.n
        ctx.count_launch(ds, dr, 0, 0)
        ctx.sse_launch(ds, True)
        got.append(ds.counters() + ds.sse_results())
        dr.free()
    ds.free()
    for a, b in zip(*got):
        assert np.array_equal(a, b)
    assert int(got[0][0].sum()) > 1000
    empty = ctx.upload_read_segments([])
    assert empty.n == 0
    empty.free()


def test_gpu_long_introns_and_hot_sites(ctx, oracle_lib):
    """Skew: reads whose introns span thousands of sites (wave-cooperative path), one site hit by 200k reads
    (LDS counter contention), sites outside the LDS window (global-atomic path), unsorted reads."""
    sites_c, reads_c, hot_row = limitcases.long_introns_hot_sites_case()
    pos, strand, part_off, part_pos, comp_off, comp_pos = (sites_c.pos, sites_c.strand, sites_c.part_off, sites_c.part_pos,
                                                           sites_c.comp_off, sites_c.comp_pos)
    for stranded, flags in ((0, 0), (1, 0), (0, native.OPT_PAIR_KERNEL), (2, native.OPT_PAIR_KERNEL)):
        got = ctx.count(sites_c, reads_c, stranded, 0, flags)
        want = oracle_lib.check_bam(pos, strand, part_off, part_pos, comp_off, comp_pos, reads_c.pos, reads_c.flag,
                                    reads_c.cig_off, reads_c.cigar, stranded, 0)
        for g, w in zip(got, want):
            assert np.array_equal(g, w)
    assert int(want[0][hot_row]) >= 50000
    # a table without part_site (or with one-way partner links) must silently take the pair kernel
    one_way = native.SiteArrays(pos, strand, part_off, part_pos, comp_off, comp_pos)
    got = ctx.count(one_way, reads_c, 1, 0)
    want = oracle_lib.check_bam(pos, strand, part_off, part_pos, comp_off, comp_pos, reads_c.pos, reads_c.flag,
                                reads_c.cig_off, reads_c.cigar, 1, 0)
    for g, w in zip(got, want):
        assert np.array_equal(g, w)


def test_gpu_read_with_more_ops_than_the_packed_count_holds(ctx, oracle_lib):
    """A read of 70 000 CIGAR ops (the packed op count saturates at 65 535) between ordinary reads: the kernels must find
    its true op count although the chunk-local partition moves it away from its place in the input."""
    sites_c, reads_c = limitcases.more_ops_than_the_packed_count_case()
    pos, strand, part_off, part_pos, comp_off, comp_pos = (sites_c.pos, sites_c.strand, sites_c.part_off, sites_c.part_pos,
                                                           sites_c.comp_off, sites_c.comp_pos)
    want = oracle_lib.check_bam(pos, strand, part_off, part_pos, comp_off, comp_pos, reads_c.pos, reads_c.flag,
                                reads_c.cig_off, reads_c.cigar, 0, 0)
    for flags in KERNELS.values():
        got = ctx.count(sites_c, reads_c, 0, 0, flags)
        for g, w in zip(got, want):
            assert np.array_equal(g, w)
    assert int(want[0].sum()) > 0


def test_gpu_empty_and_degenerate_inputs(ctx):
    empty_sites = native.SiteArrays(np.zeros(0), np.zeros(0, np.uint8), np.zeros(1), np.zeros(0), np.zeros(1), np.zeros(0))
    one_read = native.ReadArrays([100], [0], [0, 1], [50 << 4])
    b1, b2, d = ctx.count(empty_sites, one_read)
    assert len(b1) == 0 and len(b2) == 0 and len(d) == 0
    sites_c = native.SiteArrays([120], [ord("+")], [0, 1], [300], [0, 0], np.zeros(0))
    no_reads = native.ReadArrays(np.zeros(0), np.zeros(0), [0], np.zeros(0))
    b1, b2, d = ctx.count(sites_c, no_reads)
    assert b1.tolist() == [0] and b2.tolist() == [0]
    b1, _, _ = ctx.count(sites_c, one_read)
    assert b1.tolist() == [1]
    star = native.ReadArrays([120, 120], [0, 4], [0, 0, 1], [60 << 4])   # CIGAR '*' and unmapped-with-CIGAR at t
    b1, _, _ = ctx.count(sites_c, star)
    assert b1.tolist() == [1]


def test_gpu_rejects_bad_arguments(ctx):
    sites_c = native.SiteArrays([200, 100], [43, 43], [0, 0, 0], np.zeros(0), [0, 0, 0], np.zeros(0))
    reads_c = native.ReadArrays([100], [0], [0, 1], [50 << 4])
    with pytest.raises(native.SpliserNativeError):
        ctx.count(sites_c, reads_c)          # unsorted site table
    ok_sites = native.SiteArrays([100], [43], [0, 0], np.zeros(0), [0, 0], np.zeros(0))
    with pytest.raises(native.SpliserNativeError):
        ctx.count(ok_sites, reads_c, stranded=3)
    far = native.ReadArrays([2147483000], [0], [0, 1], [(1 << 20) << 4])
    with pytest.raises(native.SpliserNativeError) as err:
        ctx.count(ok_sites, far)
    assert err.value.code == -6


def test_process_cli_end_to_end_bam(ctx, tmp_path, oracle_lib):
    """BAM file -> native decoder -> packed shard -> kernels -> .SpliSER.tsv, vs the committed golden."""
    from spliser_amd import cli
    for case, variant in (("random_b", "fr_cryptic"), ("multichrom", "annot"), ("single_gene", "gene")):
        d = os.path.join(helpers.GOLDEN, case)
        opts = dict(__import__("json").load(open(os.path.join(helpers.GOLDEN, "manifest.json")))[case][variant])
        names, sets = samio.read_sam(os.path.join(d, "reads.sam"))
        bam = str(tmp_path / (case + ".bam"))
        samio.write_bam(bam, names, [10 ** 8] * len(names), [(c, sets[c]) for c in names if c in sets], with_seq=True)
        argv = ["process", "-B", bam, "-b", os.path.join(d, "junctions.bed"), "-o", str(tmp_path / case)]
        if opts.get("gff"):
            argv += ["-A", os.path.join(d, "genes.gff")]
        if opts.get("chrom"):
            argv += ["-c", opts["chrom"]]
        if opts.get("gene"):
            argv += ["-g", opts["gene"], "-m", str(opts["max_intron"])]
        if opts.get("stranded"):
            argv += ["--isStranded", "-s", opts["stranded"]]
        if opts.get("cryptic"):
            argv += ["--beta2Cryptic"]
        assert cli.main(argv) == 0
        got = open(str(tmp_path / case) + ".SpliSER.tsv").read()
        assert got == helpers.expected(case, variant)[0]


@pytest.mark.parametrize("seed", range(0, 24))
@pytest.mark.parametrize("stranded", [0, 1, 2])
def test_gpu_query_tables_like_combine(seed, stranded, ctx, oracle_lib):
    """Tables as `combine` asks about them: rows without links between them, partial partner / competitor lists, partners
    that are no rows, rows without strand.  The range kernel's junction table is built from each row's own lists, so these
    take the same path as `process` tables; both modes, against the oracle (and the pair kernel)."""
    import randcase
    arr, rs = randcase.make_case(seed + 300, bool(stranded))
    q = randcase.query_table(arr, seed)
    if not len(q["pos"]) or rs.n == 0:
        pytest.skip("empty case")
    sq = native.SiteArrays(q["pos"], q["strand"], q["part_off"], q["part_pos"], q["comp_off"], q["comp_pos"],
                           part_site=np.full(len(q["part_pos"]), -1, np.int32))
    r = native.ReadArrays(rs.pos, rs.flag, rs.cig_off, rs.cigar)
    for combine in (0, 1):
        want = oracle_lib.check_bam(q["pos"], q["strand"], q["part_off"], q["part_pos"], q["comp_off"], q["comp_pos"], rs.pos, rs.flag,
                                    rs.cig_off, rs.cigar, stranded, combine)
        for flags in KERNELS.values():
            for w, g in zip(want, ctx.count(sq, r, stranded, combine, flags)):
                assert np.array_equal(w, g)
