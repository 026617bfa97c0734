"""``genecounts --fragments`` on the device: ``gene_counts(fragments=True)`` (``spl_gene_count_fragments`` on the mate table of
``spl_mate_table``) against ``matecases.fragment_results`` -- exactly, the sums being integers -- on generated paired sets whose
coverage is asserted, unstranded, fr, rf and moved by a shift; on hand cases whose answers can be read off the rule; with leader and
mate in different waves and workgroups; through every decode, where one paired file goes in as BAM on the device, BAM on the host
threads, SAM text, BGZF SAM text and the BAM shuffled, and the command writes one and the same file; and without the flag, where
everything is what it was."""
import numpy as np
import pytest

import genecases as G
import matecases as M
import samzcases as Z
from spliser_amd import cli, genecounts as gc, native, samio

pytestmark = pytest.mark.gpu

TILE, GRID_MAX = 256, 1024          # csrc/spl_genecount.h: the fragment kernel's geometry is the per-read kernel's
LARGE = 2 * GRID_MAX * TILE + 1
BYTE = {"+": 43, "-": 45, ".": 46}
N_GENES, LENGTH = 9, 6000


@pytest.fixture(scope="module")
def ctx():
    with native.Context(0) as c:
        yield c


def _arrays(features):
    return (np.array([f[0] for f in features], np.int64), np.array([f[1] for f in features], np.int64), np.array([BYTE[f[2]] for f in features], np.uint8),
            np.array([f[3] for f in features], np.int64))


def _device(ctx, rs, keys, n_genes, a, b=None, stranded=0, shift=0, fragments=True):
    with ctx.upload_soa([native.ReadArrays(rs.pos, rs.flag, rs.cig_off, rs.cigar, name_key=np.asarray(keys, np.uint64))], with_keys=True) as soa:
        with ctx.begin_reads() as dr:
            dr.add_soa(soa, 0, shift)
            dr.finish()
            got = dr.gene_counts(n_genes, a, b, stranded, fragments=fragments)
            pairs = dr.mate_table(0)[1]["paired"] // 2
            assert got.dtype == np.int64 and got.shape == (n_genes + 3,) and int(got.sum()) == rs.n - (pairs if fragments else 0)          # rows sum to reads - pairs
            if rs.n:
                assert dr.layout_bytes()[1] == 0          # (the set stays fused)
            return got.tolist()


@pytest.fixture(scope="module")
def content():
    """A generated paired set of every kind -- its coverage asserted -- on random features with their three maps, and the yardstick's
    results per read (unstranded, fr, rf), computed once."""
    rng = np.random.default_rng(20261020)
    features = G.random_features(rng, LENGTH - 1200, N_GENES, 30)
    records, names, kinds = M.paired_records(rng, 1500, LENGTH - 1200)
    rs = samio.ReadSet.from_records(records)
    keys = np.array([M.name_key(n) for n in names], np.uint64)
    M.assert_covers(kinds, rs.flag, rs.pos, np.diff(rs.cig_off.astype(np.int64)), keys)
    a, _ = gc.gene_maps(*_arrays(features))
    plus, minus = gc.gene_maps(*_arrays(features), stranded=True)
    bases = G.bases_of_features(features, LENGTH)
    both = {w: G.bases_of_features(features, LENGTH, w) for w in "+-"}
    mate, counts = M.mate_table_of(rs, keys)
    results = {0: M.fragment_results(rs, keys, bases, mate=mate), 1: M.fragment_results(rs, keys, both, 1, mate=mate), 2: M.fragment_results(rs, keys, both, 2, mate=mate)}
    assert rs.n > 8 * TILE
    return dict(rs=rs, keys=keys, a=a, plus=plus, minus=minus, bases=bases, both=both, mate=mate, counts=counts, results=results)


# ---- generated sets -----------------------------------------------------------------------------------------------------------
def test_generated_pairs_unstranded_and_per_read_as_before(ctx, content):
    rs, keys = content["rs"], content["keys"]
    want = M.counts_of(content["results"][0], N_GENES)
    assert min(want[N_GENES:]) > 0 and sum(1 for c in want[:N_GENES] if c) >= 5
    assert _device(ctx, rs, keys, N_GENES, content["a"]) == want
    # without the flag: today's per-read yardstick, on the very same set
    per_read = G.counts_of(G.results_of(rs, content["bases"]), N_GENES)
    assert per_read != want and sum(per_read) == rs.n
    assert _device(ctx, rs, keys, N_GENES, content["a"], fragments=False) == per_read


@pytest.mark.parametrize("stranded", [1, 2])
def test_generated_pairs_stranded(ctx, content, stranded):
    want = M.counts_of(content["results"][stranded], N_GENES)
    assert want != M.counts_of(content["results"][0], N_GENES) and want != M.counts_of(content["results"][3 - stranded], N_GENES)
    assert _device(ctx, content["rs"], content["keys"], N_GENES, content["plus"], content["minus"], stranded) == want
    assert _device(ctx, content["rs"], content["keys"], N_GENES, content["minus"], content["plus"], 3 - stranded) == want          # rf is fr with the maps exchanged


def test_generated_pairs_moved_into_a_shard(ctx, content):
    a, shift = content["a"], 5000000
    want = M.counts_of(content["results"][0], N_GENES)
    assert _device(ctx, content["rs"], content["keys"], N_GENES, (a[0] + shift, a[1]), shift=shift) == want
    assert _device(ctx, content["rs"], content["keys"], N_GENES, a, shift=shift) != want


@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, TILE - 1, TILE, TILE + 1])
def test_sizes_around_a_wave_and_a_tile(ctx, content, n):
    rs = content["rs"].take(1000, 1000 + n)
    keys = content["keys"][1000:1000 + n]
    want = M.counts_of(M.fragment_results(rs, keys, content["bases"]), N_GENES)
    assert _device(ctx, rs, keys, N_GENES, content["a"]) == want


# ---- hand cases ---------------------------------------------------------------------------------------------------------------
# g0 '+' [100, 200), g1 '-' [300, 400), g2 '-' [100, 200) (under g0, on the other strand), nothing on [200, 300) and from 400 on
HAND_FEATURES = [(100, 200, "+", 0), (300, 400, "-", 1), (100, 200, "-", 2)]
HAND_LENGTH = 1000
# name, (flag, POS, CIGAR) of the first mate, of the second; the answer unstranded (without g2), and under fr with g2
HAND = [
    ("both mates in one gene", (99, 111, "30M"), (147, 151, "30M"), 0, 0),
    ("the mates in two genes", (99, 111, "30M"), (147, 311, "30M"), G.AMBIGUOUS, 0),          # (fr: g1 is on '-', the pair looks at '+')
    ("a gene and an intron", (99, 151, "30M"), (147, 221, "30M"), 0, 0),
    ("both nowhere", (99, 211, "30M"), (147, 451, "30M"), G.NO_FEATURE, G.NO_FEATURE),
    ("one mate spliced over the gap into the other gene", (99, 181, "10M120N10M"), (147, 451, "20M"), G.AMBIGUOUS, 0),
    ("65 / 129 under one exon: the mates see different maps", (65, 111, "30M"), (129, 151, "30M"), 0, G.AMBIGUOUS),
    ("83 / 163 under the same exon: both see the '-' map", (163, 111, "30M"), (83, 151, "30M"), 0, 2),
]


def _hand_set(spread):
    """The hand cases as one set; between a pair's mates ``spread`` reads that count for nothing (unmapped), so that leader and mate
    lie in different waves (spread 70) or workgroups (spread 300)."""
    recs, names = [], []
    for k, (_, first, second, _, _) in enumerate(HAND):
        recs.append(first); names.append(b"hand%d" % k)
        for j in range(spread):
            recs.append((4, 1, "10M")); names.append(b"filler")
        recs.append(second); names.append(b"hand%d" % k)
    return samio.ReadSet.from_records(recs), np.array([M.name_key(n) for n in names], np.uint64)


@pytest.mark.parametrize("spread", [0, 70, 300])
def test_hand_cases_with_the_mates_adjacent_in_other_waves_and_in_other_workgroups(ctx, spread):
    rs, keys = _hand_set(spread)
    unstranded = [f for f in HAND_FEATURES if f[3] != 2]
    a, _ = gc.gene_maps(*_arrays(unstranded))
    plus, minus = gc.gene_maps(*_arrays(HAND_FEATURES), stranded=True)
    mate = M.mate_table_of(rs, keys)[0]
    assert all(mate[k * (spread + 2)] == k * (spread + 2) + spread + 1 for k in range(len(HAND)))
    for stranded, maps, features, column in ((0, (a, None), unstranded, 3), (1, (plus, minus), HAND_FEATURES, 4)):
        bases = {w: G.bases_of_features(features, HAND_LENGTH, w) for w in "+-"} if stranded else G.bases_of_features(features, HAND_LENGTH)
        results = M.fragment_results(rs, keys, bases, stranded, mate=mate)
        leaders = [results[k * (spread + 2)] for k in range(len(HAND))]
        assert leaders == [h[column] for h in HAND], [h[0] for h, r in zip(HAND, leaders) if h[column] != r]          # the rule's text, read off by hand
        want = M.counts_of(results, 3)
        assert sum(want) == rs.n - len(HAND) and want[5] == spread * len(HAND)
        assert _device(ctx, rs, keys, 3, maps[0], maps[1], stranded) == want
    # each case alone: a fragment's answer does not depend on its neighbours
    for k, (name, first, second, answer, _) in enumerate(HAND):
        one = samio.ReadSet.from_records([first, second])
        assert _device(ctx, one, [7, 7], 3, a) == G.counts_of([answer], 3), name


def test_a_set_that_gives_every_workgroup_a_second_step(ctx):
    """LARGE reads of one base in two genes that alternate base by base: neighbours are mates, so every fragment is ambiguous but
    those whose second mate was dropped from pairing (every 1000th: no 0x1)."""
    start = np.arange(1000, 1000 + 2001, dtype=np.int32)
    code = np.where(np.arange(2001) % 2 == 0, 1, 2).astype(np.uint32)
    code[-1] = 0
    a = (start, code)
    i = np.arange(LARGE)
    flag = np.where(i % 2 == 0, 99, 147).astype(np.uint16)
    flag[1::1000] = 16
    keys = ((i // 2 + 1).astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15)) & np.uint64(0xFFFFFFFFFFFFFFFE)
    rs = samio.ReadSet(1001 + (i % 2000), flag, np.arange(LARGE + 1), np.full(LARGE, (1 << 4), np.uint32))
    results = M.fragment_results(rs, keys, G.bases_of_map(*a))
    want = M.counts_of(results, 2)
    assert want[3] > 250000 and want[0] > 200 and want[1] > 200 and want[2] == 0 and want[4] == 0
    assert _device(ctx, rs, keys, 2, a) == want


# ---- the decodes --------------------------------------------------------------------------------------------------------------
NAMES, LENGTHS = ["c1", "c2"], [10 ** 6] * 2
IDS = ["gene%02d" % k for k in range(8)]
SPAN = 20000


@pytest.fixture(scope="module")
def paired_files(tmp_path_factory):
    """Two chromosomes of generated paired reads with names (3000 and more reads each: more than eight BGZF blocks) and MAPQs, one
    pair split over the two, one pair whose second mate has MAPQ 3; genes on both.  The one content as BAM, the BAM shuffled record by
    record, SAM text and BGZF SAM text; the yardstick's answers computed per case."""
    d = tmp_path_factory.mktemp("fdec")
    rng = np.random.default_rng(41)
    sets, names, mapq, features, kinds = [], [], [], {}, set()
    for k, chrom in enumerate(NAMES):
        records, nm, kd = M.paired_records(rng, 1400, SPAN)
        kinds |= kd
        keep = [j for j, r in enumerate(records) if r[1] >= 1]          # (a file has no POS 0 on a reference)
        records, nm = [records[j] for j in keep], [nm[j] for j in keep]
        records += [(99, SPAN + 45, "20M"), ((99, 147)[k], SPAN + 50, "30M"), (147, SPAN + 90, "30M")]          # the MAPQ pair, and between its mates the split pair's mate
        nm += [b"lowq%d" % k, b"split/pair", b"lowq%d" % k]
        sets.append((chrom, samio.ReadSet.from_records(records)))
        names.append(nm)
        q = np.full(len(records), 60, np.int64)
        q[-1] = 3
        mapq.append(q)
        features[chrom] = [(l, r, s, g) for l, r, s, g in G.random_features(rng, SPAN, 8, 40)] + [(SPAN + 40, SPAN + 70, "+", k), (SPAN + 85, SPAN + 130, "+", 2 + k)]
    assert M.KINDS - {"POS 0"} <= kinds
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


def _want(f, stranded=0, fragments=True, min_mapq=0):
    """The yardstick over the file's reads that pass ``min_mapq``: pairing is among the reads the decode keeps."""
    out = [0] * (len(IDS) + 3)
    pairs = 0
    for (chrom, rs), keys, q in zip(f["sets"], f["keys"], f["mapq"]):
        keep = np.flatnonzero(q >= min_mapq)
        n_ops = np.diff(rs.cig_off.astype(np.int64))
        kept = samio.ReadSet.from_records([(int(rs.flag[j]), int(rs.pos[j]), samio.cigar_string(rs.cigar[rs.cig_off[j]:rs.cig_off[j + 1]]) if n_ops[j] else "") for j in keep])
        feats = f["by_chrom"].get(chrom, [])
        bases = {w: G.bases_of_features(feats, SPAN + 2100, w) for w in "+-"} if stranded else G.bases_of_features(feats, SPAN + 2100)
        if fragments:
            mate, counts = M.mate_table_of(kept, keys[keep])
            pairs += counts["paired"] // 2
            got = M.counts_of(M.fragment_results(kept, keys[keep], bases, stranded, mate=mate), len(IDS))
        else:
            got = G.counts_of(G.results_of(kept, bases, stranded), len(IDS))
        out = [x + y for x, y in zip(out, got)]
    return out, pairs


def test_the_command_writes_one_file_for_five_inputs(paired_files, capsys):
    f, d = paired_files, paired_files["dir"]
    want, pairs = _want(f)
    n_reads = sum(rs.n for _, rs in f["sets"])
    assert sum(want) == n_reads - pairs and pairs > 1500
    text = G.file_text(IDS, want)
    runs = [("bam", ["-B", f["bam"]]), ("host", ["-B", f["bam"], "--hostDecode"]), ("sam", ["-B", f["sam"]]), ("samz", ["-B", f["samz"]]), ("shuffled", ["-B", f["shuffled"], "--anyOrder"])]
    logs = {}
    for tag, args in runs:
        assert cli.main(["genecounts", "-A", f["gtf"], "-o", d + "/" + tag, "--fragments"] + args) == 0
        logs[tag] = capsys.readouterr().out
        assert open("%s/%s.genecounts.tsv" % (d, tag)).read() == text, tag
    assert "parsed on the GPU" in logs["sam"] and "parsed on the GPU" in logs["samz"] and "read by the Python reader" not in logs["sam"] + logs["samz"]
    assert ("%d pairs" % pairs) in logs["bam"] and "fragments counted" in logs["bam"] and all("  %s: " % c in logs["bam"] for c in NAMES)
    # the pair split over the two chromosomes counts twice: each mate alone finds its gene
    (c1, rs1), (c2, rs2) = f["sets"]
    for rs, keys in ((rs1, f["keys"][0]), (rs2, f["keys"][1])):
        mate = M.mate_table_of(rs, keys)[0]
        assert mate[rs.n - 2] == M.NONE and mate[rs.n - 3] == rs.n - 1 and (np.diff(rs.pos.astype(np.int64)) >= 0).all()
    # stranded, under a flag filter
    for s, code in (("fr", 1), ("rf", 2)):
        assert cli.main(["genecounts", "-B", f["bam"] if code == 1 else f["sam"], "-A", f["gtf"], "-o", d + "/" + s, "--isStranded", "-s", s, "--fragments"]) == 0
        assert open("%s/%s.genecounts.tsv" % (d, s)).read() == G.file_text(IDS, _want(f, code)[0])
    assert open(d + "/fr.genecounts.tsv").read() != open(d + "/rf.genecounts.tsv").read()


def test_min_mapq_turns_a_pair_into_a_singleton(paired_files, capsys):
    f, d = paired_files, paired_files["dir"]
    want, pairs = _want(f, min_mapq=10)
    all_want, all_pairs = _want(f)
    assert pairs == all_pairs - 2 and sum(want) == sum(all_want) and want != all_want          # two reads fewer, two pairs fewer: as many rows
    for tag, args in (("q_bam", ["-B", f["bam"]]), ("q_sam", ["-B", f["sam"]])):
        assert cli.main(["genecounts", "-A", f["gtf"], "-o", d + "/" + tag, "--fragments", "--minMapQ", "10"] + args) == 0
        assert open("%s/%s.genecounts.tsv" % (d, tag)).read() == G.file_text(IDS, want), tag
    capsys.readouterr()


def test_without_the_flag_the_command_writes_what_it_wrote(paired_files, capsys):
    f, d = paired_files, paired_files["dir"]
    want, _ = _want(f, fragments=False)
    assert sum(want) == sum(rs.n for _, rs in f["sets"])
    for tag, args in (("r_bam", ["-B", f["bam"]]), ("r_sam", ["-B", f["sam"]]), ("r_host", ["-B", f["bam"], "--hostDecode"])):
        assert cli.main(["genecounts", "-A", f["gtf"], "-o", d + "/" + tag] + args) == 0
        assert open("%s/%s.genecounts.tsv" % (d, tag)).read() == G.file_text(IDS, want), tag
    log = capsys.readouterr().out
    assert "reads counted" in log and "pairs" not in log and "fragments" not in log


def test_keys_through_the_device_decodes(ctx, paired_files):
    """What ``spl_reads_add_bam`` picks up: the device decode's keys are the written names' keys, in file order and sorted."""
    f = paired_files
    for path, any_order in ((f["bam"], False), (f["shuffled"], True)):
        bam = native.BamFile(path, threads=2, defer=True, mate_keys=True, any_order=any_order)
        try:
            assert bam.decode_on_device(ctx) is True, bam.decline_reason()
            if any_order:
                assert bam.any_order_sorted() == (sum(rs.n for _, rs in f["sets"]), True)          # the GPU's sort carried the keys
            for (chrom, rs), keys in zip(f["sets"], f["keys"]):
                with ctx.begin_reads() as dr:
                    dr.add_bam(bam, chrom)
                    dr.finish()
                    assert dr.has_mate_keys()
                    mate, counts = dr.mate_table(0, rs.n)
                    want = M.mate_table_of(rs, keys)
                    assert counts == want[1]
                    if not any_order:
                        assert mate.tolist() == want[0]
                got = bam.reads(chrom)          # (the arrays fetched to the host, the keys with them)
                if any_order:
                    assert sorted(zip(got.pos.tolist(), got.flag.tolist(), got.name_key.tolist())) == sorted(zip(rs.pos.tolist(), rs.flag.tolist(), keys.tolist()))
                else:
                    assert np.array_equal(got.name_key, keys) and np.array_equal(got.flag, rs.flag)
        finally:
            bam.close()
    bam = native.BamFile(f["bam"], threads=2, defer=True)
    try:
        assert bam.decode_on_device(ctx) is True
        with ctx.begin_reads() as dr:
            dr.add_bam(bam, "c1")
            dr.finish()
            assert not dr.has_mate_keys()
            with pytest.raises(native.SpliserNativeError, match="name keys"):
                dr.gene_counts(len(IDS), None, fragments=True)
    finally:
        bam.close()
